// Host-only code (no HIP) of the pathwise driver: the option table, the plan of a batch (plan_pathwise) and the per-graph
// tables the driver uploads next to the step tables of rg_steps.cpp.  Part of the sanitizer build (tests/c/host_asan.cpp);
// tests/c/plan_check.cpp states the routes plan_pathwise takes.
#include "rg_path_plan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace rg {

// ---- the option table (RG_OPTIONS, rg_host.hpp) ----
#define RG_OPTION_ROW(name, env, kind, lo, hi, def) {#name, env, #kind[0] == 'B', lo, hi, def, &Options::name},
const OptionDesc kOptionTable[] = {RG_OPTIONS(RG_OPTION_ROW) RG_TUNING_OPTIONS(RG_OPTION_ROW)};
#undef RG_OPTION_ROW
const int kOptionCount = (int)(sizeof kOptionTable / sizeof kOptionTable[0]);

const OptionDesc* find_option(const char* name) {
    if (!name) return nullptr;
    for (const OptionDesc& d : kOptionTable)
        if (!strcmp(name, d.name)) return &d;
    return nullptr;
}
void store_option(Options& o, const OptionDesc& d, long long value) {
    o.*d.slot = d.boolean ? (value ? 1 : 0) : (int)std::max<long long>(d.lo, std::min<long long>(value, d.hi));
}
Options& options() {
    static Options o;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const OptionDesc& d : kOptionTable) {
            const char* v = getenv(d.env);
            if (!v) continue;
            store_option(o, d, d.boolean ? (*v && strcmp(v, "0") != 0) : atoi(v));
        }
    });
    return o;
}

// Host-side admission test: uniform gap cost and every STORED value provably inside the 16-bit budget.
// What the rows hold is z = A - c * g (c: column, g: the gap cost), not A.  A row starts at z = 0 and changes only through
//   U: z + g_i (= z + g, the gap column is uniform)        D: z_diagonal + (s - g)        L: z_left (a copy)
// — whoever chose the move (members follow their alpha), every cell is its chain's start plus one such step per move.  So after
// at most `rows` graph rows and n read bases
//   zlo = -(rows + 2) * |g| - (n + 2) * max(0, g - min s)   <=   z   <=   (n + 2) * max(0, max s - g) = zhi
// (round 4 bounded |A| <= (rows + n) * max|entry| <= 24 000 instead, which refused -X 6 at 1 kbp and every read longer than
// ~1.2 kbp: the all-gap corner of A is -(rows + n) |g|, the same corner of z only -rows |g|).  Required:
//   * zlo above the "minus infinity" of a 16-bit lane (NEG16 = -30 000) with a step of head-room, zhi below +29 000;
//   * zhi - zlo <= 32 000: every difference of two stored values (direction masks from the sign of d - max(d, u), the
//     gather runs' member deltas) fits a signed half;
//   * |A| <= (rows + n + 2) * max|entry| <= 32 000: outputs convert back (A = z + c g) inside key << 16 arithmetic;
//   * gap entries <= 0: the border column (c = 0: z = A = i * g) then holds values <= 0, so that d - max(d, u) of lane 0's
//     column 0 (d = NEG16 + s, u = the border value) stays above -32768 and the U mask keeps its sign.
bool sweep16_admissible(const DevScores& sc, int max_path_rows, int max_n, int C) {
    for (int b = 1; b < 5; ++b) if (sc.t[b * 6 + 5] != sc.t[5]) return false;
    for (int b = 0; b < 5; ++b) if (sc.t[b * 6 + 5] > 0 || sc.t[5 * 6 + b] > 0) return false;
    long long maxabs = 0, smin = INT32_MAX, smax = INT32_MIN;
    for (int x = 0; x < 6; ++x)
        for (int y = 0; y < 6; ++y) {
            if (x == 5 && y == 5) continue;
            const long long v = sc.t[x * 6 + y];
            maxabs = std::max(maxabs, v < 0 ? -v : v);
            if (x < 5 && y < 5) { smin = std::min(smin, v); smax = std::max(smax, v); }
        }
    if (maxabs > 1000) return false;
    const long long g = sc.t[5];                 // <= 0
    const long long rows = max_path_rows + 2, n = max_n + 2;
    const long long zlo = rows * g - n * std::max(0ll, g - smin);
    const long long zhi = n * std::max(0ll, smax - g);
    if (zlo < -29000 || zhi > 29000 || zhi - zlo > 32000) return false;
    if ((rows + n) * maxabs > 32000) return false;                 // |A| of every cell
    if ((long long)(C / 2 + 2) * maxabs > 2000) return false;
    return true;
}

// The affine-gap pathwise modes (the table: rg_gap_modes.hpp): one wave per (read, path) keeps H and Y of the current row in registers,
// C columns per lane (n + 1 <= 64 C), so a read must fit one wave, or as many column stripes of 2048, walked by that one wave, as the
// mode's family allows (gap_long/, gap_xlong/); the only HBM work buffer beside ReadState holds the 4-bit directions of the picked path.
static int plan_pathwise_gap(const rg_params& p, const GapMode& gm, const PathPlanInput& in, PathPlan& o) {
    if (p.gap_open > 0 || p.gap_ext > 0) return fail(RG_ERR_ARG, "gap penalties must be <= 0");
    const GapFamily& f = *gm.family;
    const bool local = gm.rule == GAP_RULE_LOCAL;
    // a both-strands family: both strands is what the mode does (bit 2 is redundant); the vote is a rule of the two modes whose scores
    // can be negative.  Every pass (every stage) of such a batch is planned here, with its own longest read
    if (f.both_strands && local && p.amb_mode == (RG_AMB_BOTH_STRANDS | RG_AMB_STRAND_VOTE))
        return fail(RG_ERR_ARG, "RG_AMB_STRAND_VOTE is not available in the local both-strands mode (-m " + std::to_string(p.mode) +
                                "): no score of a local pass says \"hopeless\", so a vote would have no rule for a second pass");
    if (p.amb_mode != 0 && !(f.both_strands && (p.amb_mode == RG_AMB_BOTH_STRANDS || p.amb_mode == (RG_AMB_BOTH_STRANDS | RG_AMB_STRAND_VOTE))))
        return fail(RG_ERR_ARG, f.amb_text(local));
    if (in.max_n > f.max_read()) return fail(RG_ERR_ARG, f.len_text(local));
    // every value of H, X, Y is a sum of at most (rows + n) steps of at most max(|sc|, |o + e|) each: kept inside +-2^28, so that
    // the NEG sentinel (-2^29) plus any such sum can neither win nor wrap (the striped kernels' z in global columns: their header)
    long long maxabs = std::llabs((long long)p.gap_open + (long long)p.gap_ext);
    for (int x = 0; x < 5; ++x)
        for (int y = 0; y < 5; ++y)
            if (p.scores[x * 6 + y] != RG_SCORE_MISSING) maxabs = std::max<long long>(maxabs, std::llabs((long long)p.scores[x * 6 + y]));
    if ((long long)(in.max_path_rows + in.max_n) * maxabs >= (1ll << 28))
        return fail(RG_ERR_CAPACITY, "scores of this batch can reach 2^28 in magnitude: outside the i32 range of the affine-gap pathwise kernels");
    o.gap = true;
    o.mode = RG_MODE_PATHWISE_GAP;
    o.semi = gm.rule == GAP_RULE_SEMI;
    o.local = local;          // (neither end is pinned; `semi` stays false)
    int C = 4;
    while (C * WAVE < in.max_n + 1 && C < 32) C *= 2;
    o.C = C;
    // a long mode whose longest read fits one wave runs the base mode's kernels on the base mode's plan; beyond that, column stripes
    o.nwv = (in.max_n + 1 + C * WAVE - 1) / (C * WAVE);
    o.wpad = o.nwv * C * WAVE;
    o.gap_words = std::max(1, C / 8);
    o.gdirs_stride = (long long)o.nwv * (in.max_path_rows + 1) * o.gap_words * WAVE;
    o.per_read = (size_t)o.gdirs_stride * 4 + sizeof(ReadState);
    if (o.nwv > 1 && f.one_stripe_dirs) {
        // gap_xlong/rg_path_gap_xlong.hip, whatever the stripe count: direction words of ONE stripe, a checkpoint
        // slot of two ints per row for every stripe but the last, the score pass's boundary buffer and the walk state
        const long long rows1 = in.max_path_rows + 1;
        o.gap_xlong = true;
        o.gdirs_stride = rows1 * o.gap_words * WAVE;
        o.gbnd_stride = 2ll * rows1 * in.P;
        o.gckpt_stride = (long long)(o.nwv - 1) * 2 * rows1;
        o.gwalk_bytes = 32;
        o.per_read = (size_t)o.gdirs_stride * 4 + (size_t)(o.gbnd_stride + o.gckpt_stride) * 4 + o.gwalk_bytes + sizeof(ReadState);
    } else if (o.nwv > 1) {
        o.gbnd_stride = 2ll * (in.max_path_rows + 1) * in.P;
        o.gdbnd_stride = 2ll * (in.max_path_rows + 1);
        o.per_read += (size_t)(o.gbnd_stride + o.gdbnd_stride) * 4;
    }
    for (int x = 0; x < 5; ++x)
        for (int y = 0; y < 5; ++y) o.maxmatch = std::max(o.maxmatch, p.scores[x * 6 + y]);
    return RG_OK;
}

// The edit-distance modes (the table: rg_edit_modes.hpp): the rules of modes 6 / 7 at unit costs, one bit per cell.  One wave per (read,
// path) keeps the whole read in its registers, 32 W columns per lane; the only HBM work buffer beside ReadState holds D0 and Ph of the
// picked path's rows, 2 bits per cell.  That up to 16383 bases in every family; beyond, stripes of 16384 columns (PathPlan::edit_xlong).
int plan_pathwise_edit(const rg_params& p, const PathPlanInput& in, PathPlan& o) {
    const EditMode em = edit_mode(p.mode);
    if (!em.valid) return fail(RG_ERR_ARG, "unsupported mode");
    const EditFamily& f = *em.family;
    if (p.gap_open > 0 || p.gap_ext > 0) return fail(RG_ERR_ARG, "gap penalties must be <= 0");
    bool unit = p.gap_open == 0 && p.gap_ext == -1;
    for (int x = 0; x < 5; ++x)
        for (int y = 0; y < 5; ++y) unit = unit && (p.scores[x * 6 + y] == 0 || p.scores[x * 6 + y] == -1);
    if (!unit) return fail(RG_ERR_ARG, f.score_refusal);
    if (p.amb_mode != 0) return fail(RG_ERR_ARG, f.amb_refusal);
    if (in.max_n > f.max_read) return fail(RG_ERR_ARG, f.len_refusal);
    // mode 16's budget, at max(|sc|, |o + e|) = 1: what it refuses is refused here
    if ((long long)in.max_path_rows + in.max_n >= (1ll << 28))
        return fail(RG_ERR_CAPACITY, "scores of this batch can reach 2^28 in magnitude: outside the i32 range of the affine-gap pathwise kernels");
    o.edit = true;
    o.mode = RG_MODE_PATHWISE_EDIT;
    o.semi = em.semi;
    int W = 1;
    while (2048 * W < in.max_n && W < EDIT_MAX_WORDS) W *= 2;
    o.edit_words = W;
    o.C = 32 * W;                 // columns per lane
    o.nwv = 1;
    o.wpad = 2048 * W;
    o.gdirs_stride = (long long)(in.max_path_rows + 1) * 2 * W * WAVE;
    o.per_read = (size_t)o.gdirs_stride * 4 + sizeof(ReadState);
    if (in.max_n > EDIT_MAX_READ) {
        // edit_xlong/rg_path_edit_xlong.hip: D0 and Ph of ONE stripe (the words above, at W = 8), the boundary slots of every path
        // and stripe but the last, and the walk state
        o.edit_xlong = true;
        // (16384 bases fill one stripe to its last bit: such a batch still runs the striped kernels, its second stripe empty)
        o.nwv = std::max(2, (in.max_n + EDIT_XLONG_STRIPE - 1) / EDIT_XLONG_STRIPE);
        o.wpad = o.nwv * EDIT_XLONG_STRIPE;
        o.edit_slot_words = (2 * ((in.max_path_rows + 63) / 64) + 15) / 16 * 16;
        o.edit_bnd_stride = (long long)in.P * (o.nwv - 1) * o.edit_slot_words;
        o.gwalk_bytes = 32;
        o.per_read += (size_t)o.edit_bnd_stride * 8 + o.gwalk_bytes;
    }
    return RG_OK;
}

// The both-strands edit-distance modes (rg_edit_strands_modes.hpp): the plan of -m 44 / -m 45 for the direction pass and the walk, which
// run once per read on the strand that won; the score pass holds a strand in half a wave, 32 W' columns per lane.  Beside that plan's
// buffers: the picks of the reverse strand (a second ReadState), the read on the winning strand and the strand byte.
int plan_pathwise_edit_strands(const rg_params& p, const PathPlanInput& in, PathPlan& o) {
    const EditStrandsMode em = edit_strands_mode(p.mode);
    if (!em.valid) return fail(RG_ERR_ARG, "unsupported mode");
    if (p.gap_open > 0 || p.gap_ext > 0) return fail(RG_ERR_ARG, "gap penalties must be <= 0");
    bool unit = p.gap_open == 0 && p.gap_ext == -1;
    for (int x = 0; x < 5; ++x)
        for (int y = 0; y < 5; ++y) unit = unit && (p.scores[x * 6 + y] == 0 || p.scores[x * 6 + y] == -1);
    if (!unit) return fail(RG_ERR_ARG, kEditStrandsScoreRefusal);
    // both strands is what the modes do (bit 2 is redundant); the vote would change the rule and save nothing
    if (p.amb_mode != 0 && p.amb_mode != RG_AMB_BOTH_STRANDS) return fail(RG_ERR_ARG, kEditStrandsAmbRefusal);
    if (in.max_n > EDIT_STRANDS_MAX_READ) return fail(RG_ERR_ARG, kEditStrandsLenRefusal);
    // mode 16's budget, at max(|sc|, |o + e|) = 1: what it refuses is refused here
    if ((long long)in.max_path_rows + in.max_n >= (1ll << 28))
        return fail(RG_ERR_CAPACITY, "scores of this batch can reach 2^28 in magnitude: outside the i32 range of the affine-gap pathwise kernels");
    o.edit = true;
    o.edit_strands = true;
    o.mode = RG_MODE_PATHWISE_EDIT;
    o.semi = em.semi;
    int W = 1;
    while (2048 * W < in.max_n && W < EDIT_MAX_WORDS) W *= 2;
    o.edit_words = W;
    int Wp = 1;
    while (1024 * Wp < in.max_n && Wp < EDIT_STRANDS_MAX_WORDS) Wp *= 2;
    o.edit_pair_words = Wp;
    o.C = 32 * W;                 // columns per lane of the direction pass
    o.nwv = 1;
    o.wpad = 2048 * W;
    o.gdirs_stride = (long long)(in.max_path_rows + 1) * 2 * W * WAVE;
    o.edit_orient_bytes = ((size_t)in.max_n + 15) & ~(size_t)15;
    o.per_read = (size_t)o.gdirs_stride * 4 + 2 * sizeof(ReadState) + o.edit_orient_bytes + 1;
    return RG_OK;
}

int plan_gap_stage(PathPlan& o, int stage) {
    if (stage == PATH_STAGE_ALL) return RG_OK;
    if ((stage != PATH_STAGE_PICK && stage != PATH_STAGE_TRACE) || !o.gap || (o.nwv > 1 && !o.gap_xlong))
        return fail(RG_ERR_ARG, "a pick or trace stage needs an affine-gap plan of one wave or of the checkpointed stripes");
    // (only the score pass reads and writes the boundary ints: gap_xlong/ exchanges its stripes through the checkpoint slots)
    const size_t bnd = o.nwv > 1 ? (size_t)o.gbnd_stride * 4 : 0;
    o.stage = stage;
    o.per_read = stage == PATH_STAGE_PICK ? sizeof(ReadState) + bnd : o.per_read - bnd;
    return RG_OK;
}

int plan_pathwise(const rg_params& p, const PathPlanInput& in, const Options& opt, int spec_level, PathPlan& o) {
    o = PathPlan{};
    const GapMode gm = gap_mode(p.mode);
    if (gm.valid) return plan_pathwise_gap(p, gm, in, o);
    if (edit_mode(p.mode).valid) return plan_pathwise_edit(p, in, o);
    if (edit_strands_mode(p.mode).valid) return plan_pathwise_edit_strands(p, in, o);
    const int P = in.P, L = in.L, max_n = in.max_n;
    o.semi = p.mode == RG_MODE_PATHWISE_SEMI || p.mode == RG_MODE_RECOMBINATION_SEMI;
    o.mode = p.mode == RG_MODE_PATHWISE_SEMI ? RG_MODE_PATHWISE : p.mode == RG_MODE_RECOMBINATION_SEMI ? RG_MODE_RECOMBINATION : p.mode;
    const bool recomb = o.mode == RG_MODE_RECOMBINATION, semi = o.semi;
    int C = 4;
    while (C * WAVE < max_n + 1 && C < 32) C *= 2;
    // Reads longer than 2047 bases: column stripes, one wave per stripe in one workgroup of at most 8 waves (k_sweep /
    // k_layer <C, true>): i32 rows, Cand lists; needs a uniform read-gap cost (every matrix the reference's CLI builds).
    // Stripes of 1024 columns (C = 16: rows, keys and thresholds fit the 256 registers) up to 8191 bases; 2048 (C = 32,
    // which spills 800 registers) beyond; RG_STRIPE_C / rg_set_option("stripe_c") overrides (8, 16, 32).
    if (max_n + 1 > 32 * WAVE) {
        C = max_n + 1 <= 8 * 16 * WAVE ? 16 : 32;
        if ((opt.stripe_c == 8 || opt.stripe_c == 16 || opt.stripe_c == 32) && max_n + 1 <= 8 * opt.stripe_c * WAVE) C = opt.stripe_c;
    }
    const int nwv = (max_n + 1 + C * WAVE - 1) / (C * WAVE);
    if (nwv > 8) return fail(RG_ERR_ARG, "reads longer than 16383 bases are not supported by the pathwise kernels");
    if (nwv > 1)
        for (int b = 1; b < 5; ++b)
            if (p.scores[b * 6 + 5] != p.scores[5]) return fail(RG_ERR_ARG, "reads longer than 2047 bases need a uniform read-gap cost");
    o.C = C;
    o.nwv = nwv;
    o.wpad = nwv * C * WAVE;
    o.dir_words = nwv * WAVE * (C <= 16 ? 1 : 2);
    o.recw = 4 + C;
    // packed 16-bit rows (rg_sweep16.hip) whenever the scores of this batch provably fit; RG_SWEEP_I32=1 forces the i32
    // kernel (test hook: the two must agree byte for byte).  One wave per read only: `use16` says both from here on.
    DevScores dsc;
    for (int i = 0; i < 36; ++i) dsc.t[i] = p.scores[i];
    o.use16 = nwv == 1 && !opt.sweep_i32 && sweep16_admissible(dsc, in.max_path_rows, max_n, C);
    if (!o.use16) {
        // the i32 sweep packs (value, path) keys as value * 256 + path in 32 bits: |value| must stay below 2^23
        long long maxabs = 0;
        for (int i = 0; i < 36; ++i) if (i != 35 && p.scores[i] != RG_SCORE_MISSING) maxabs = std::max<long long>(maxabs, std::llabs((long long)p.scores[i]));
        if ((long long)(in.max_path_rows + max_n + 2) * maxabs >= (1ll << 23))
            return fail(RG_ERR_CAPACITY, "scores of this batch can reach 2^23 in magnitude: outside the 32-bit (value, path) keys of the pathwise kernels");
    }
    const bool use16 = o.use16;
    o.layer_stride = (long long)(in.max_path_rows + 2) * o.dir_words;   // traceback decisions: 2 bits per cell
    o.fdirs_stride = (long long)in.fslots * o.dir_words;
    o.rdirs_stride = (long long)in.rslots * o.dir_words;
    // (k_sweep16: P + 2 packed rows per read — two pseudo-rows behind the rolling rows — of wpad / 2 words)
    o.per_read = (size_t)(o.fdirs_stride + (recomb ? o.rdirs_stride : 0)) * 4 + (size_t)o.layer_stride * 4 * (recomb ? 2 : 1) +
                 (size_t)(P + 2) * o.wpad * 4 + (size_t)o.wpad * 20 + sizeof(ReadState);
    // -m 8 pipeline: two sweeps (forward with a loose threshold from the exact path-0 score, then reverse) when
    // every gap entry is <= 0 (then w[.][j] <= (n - j) * max match); three sweeps otherwise / on request
    o.gaps_nonpos = o.gaps_agree = true;
    for (int x = 0; x < 5; ++x) {
        o.gaps_nonpos = o.gaps_nonpos && p.scores[x * 6 + 5] <= 0 && p.scores[5 * 6 + x] <= 0;
        o.gaps_agree = o.gaps_agree && p.scores[5 * 6 + x] == p.scores[x * 6 + 5];
        for (int y = 0; y < 5; ++y) o.maxmatch = std::max(o.maxmatch, p.scores[x * 6 + y]);
    }
    // (striped long reads, nwv > 1, take it too since round 4: k_opt0_striped gives them the forward bound)
    o.two_sweep = recomb && o.gaps_nonpos && !opt.three_sweeps;
    // forward emissions of the two-sweep pipeline are loose (threshold from the path-0 score): k_sweep16 writes them as
    // (row, lane) records that k_expand filters with the final bound; k_sweep writes plain Cand entries
    o.use_rec = o.two_sweep && use16 && !opt.no_frec;
    // more than 64 paths only on packed rows: k_pick votes over up to 256 paths, k_sweep16 retires over several words
    const bool paths_ok = P <= 64 || use16;
    // speculative forward bound (PickArgs in rg_path_kernels.hpp): checked by k_verify, failed reads aligned again by the driver
    // (long reads emit Cand entries, not records: without the speculation their forward lists would hold every cell within
    // ~(seed - path-0 score) / 10 columns of a diagonal — millions per read at 5 kbp)
    // spec_level 1: the sweeps of the failed reads still retire paths and emit few records (a second pass on the provable bound
    // keeps one wave per read busy for two full sweeps and a search over ~40 000 records)
    // (round 5: the i32 sweep of reads that fit one wave takes it as well — score matrices outside the 16-bit budget, HOXD70 /
    // HOXD55 with their -200 gaps, emitted every forward cell within (seed - path-0 score) of a diagonal as a Cand)
    o.spec = o.two_sweep && spec_level < 2 && !semi && paths_ok && !opt.no_spec;
    // (a follower path's sink value lies below its own NW optimum — measured up to 72 at 1 kbp — and the gap grows with the
    // read: long reads scale the margin with their length, or every read would fail the check and run again)
    // The margin is in units of the default scores (match 2): other matrices scale it with their best match (HOXD70: 100 -> x50).
    o.score_scale = std::max(1, o.maxmatch / 2);
    const int per_kbp = (max_n + 999) / 1000;
    o.spec_margin = ((nwv > 1 ? opt.spec_margin * per_kbp : (int)opt.spec_margin) + (spec_level == 1 ? 320 * per_kbp : 0)) *
                    (opt.spec_margin > 0 ? o.score_scale : 1);
    o.pick_two = o.spec && !opt.no_pick2;      // (two-path picks: global mode, which `spec` implies)
    // direction words on demand (k_sweep16, DIRECTION WORDS ON DEMAND): the record variants, first pass
    // only — a read that comes back because its final paths were not the picked ones stores every word the second time
    o.dsel = o.spec && o.use_rec && spec_level == 0 && !opt.no_dsel;
    { const int e = L / std::max(1, (int)opt.dsel_edge); o.dsel_lo = e; o.dsel_hi = L - 1 - e; }      // (an eighth of the rows at the end each sweep starts from)
    o.rec_pen = p.base_rec_cost + (int)std::ceil(p.multi_rec_cost * 8.0f);
    // -m 4 on a speculative bound (round 6): k_pick's path, k_opt0's score against it minus the margin as the bound the sweep retires
    // paths against, direction words for the picked path only; k_verify4 sends a read whose best final score does not reach the bound
    // (or whose best path is not the pick) to a second pass without any of it.  Packed rows, one wave per read, the default scores' sign
    // conditions (gap entries <= 0: the hopeless bound counts on them).
    o.spec4 = o.mode == RG_MODE_PATHWISE && !semi && use16 && o.gaps_nonpos && spec_level == 0 && !opt.no_spec;
    // (the margin: a follower path's final score lies below its own alignment optimum — up to 180 at 1 kbp in config 4, where
    // -m 8's search maximum rarely does: 2.5 x the -m 8 margin; RG_SPEC4_MARGIN_X10 scales it for experiments)
    o.spec4_margin = o.spec_margin * opt.spec4_margin_x10 / 10;
    o.retire4 = o.spec4 && opt.no_retire != 1;
    o.dsel4 = o.spec4 && !opt.no_dsel;
    o.order = !opt.no_order;
    // (packed rows whenever the sweep runs packed: a third of the i32 form's instructions)
    o.opt16 = use16;
    // (packed 16-bit rows whenever the sweep ran packed: the same decisions, ~40 % fewer instructions; `layer_i32` keeps the
    // i32 form for the tests)
    o.layer16 = use16 && o.gaps_agree && !opt.layer_i32;
    // the layers inside a column window around the walk (layer_window/rg_layer_window.hip): packed rows at <= 16 columns per lane, first
    // pass only (the handful of reads of a second pass keep the full-width kernel), and only where every real value of a row
    // stays above LAYER_WINDOW_ZLO, so that the window's "unknown" sentinel plus one step lies clearly below it (zlo as in
    // sweep16_admissible)
    o.layer_window = 0;
    if (o.layer16 && C <= 16 && spec_level == 0 && opt.layer_window >= LAYER_WINDOW_NARROW) {
        long long smin = INT32_MAX;
        for (int x = 0; x < 5; ++x)
            for (int y = 0; y < 5; ++y) smin = std::min<long long>(smin, p.scores[x * 6 + y]);
        const long long g = p.scores[5];
        const long long zlo = (long long)(in.max_path_rows + 2) * g - (long long)(max_n + 2) * std::max(0ll, g - smin);
        if (zlo >= LAYER_WINDOW_ZLO) o.layer_window = opt.layer_window >= LAYER_WINDOW_DEFAULT ? LAYER_WINDOW_DEFAULT : LAYER_WINDOW_NARROW;
    }
    // (gather runs carry differences of two members' stored values: sweep16_admissible bounds every such difference)
    o.gather_ok = use16 && !opt.no_gather;
    // split tables: only where every run between the groups of a row is a register or a gather run of k_sweep16
    o.use_split = o.gather_ok && !semi && C <= 16 && !opt.no_split;
    // path retirement: the record pipelines of -m 8 (global) (round 5: the i32 sweep too — one wave, or stripes of <= 16 columns per lane)
    o.retire = (use16 || nwv == 1 || C <= 16) && paths_ok && !semi && recomb && o.gaps_nonpos && opt.no_retire != 1;
    o.retire_fwd = o.retire && opt.no_retire != 3;
    o.retire_rev = o.retire && opt.no_retire != 2;
    // (round 6: 16 Ki / 8 Ki records of 80 B to start with instead of 64 Ki / 32 Ki — 2 MB per read instead of 7.9; a read that needs
    // more regrows the lists and the chunk runs again, once per handle; batches WITHOUT a speculative bound keep the old sizes: their
    // forward lists hold tens of thousands of records per read, and 128-path tiles ran twice every time a tile's largest read outgrew
    // the last one's.  Config 5 with the two-path pick: forward mean ~11 k)
    o.fcap = (o.two_sweep && !o.use_rec) ? 1u << 20 : 1u << 15;
    o.rcap = o.use_rec ? 1u << 16 : 1u << 19;
    o.frec_cap = o.spec ? 1u << 14 : 1u << 16;
    o.rrec_cap = o.spec ? 1u << 13 : 1u << 15;
    return RG_OK;
}

void build_path_rows(const HostGraph& h, bool fwd, std::vector<int>& poff, std::vector<int>& prow, std::vector<int>& pslot) {
    const std::vector<int32_t>& goff = fwd ? h.fgoff : h.rgoff;
    const std::vector<GroupDesc>& groups = fwd ? h.fgroups : h.rgroups;
    const int P = h.P, L = h.L;
    std::vector<std::vector<std::pair<int, int>>> per(P);
    for (int step = 1; step + 1 < L; ++step) {
        const int i = fwd ? step : L - 1 - step;
        for (int gi = goff[i]; gi < goff[i + 1]; ++gi)
            for (int b = 0; b < 64; ++b)
                if ((groups[gi].mask >> b) & 1) per[groups[gi].page * 64 + b].push_back({i, groups[gi].slot});
    }
    poff.assign(P + 1, 0);
    prow.clear();
    pslot.clear();
    for (int k = 0; k < P; ++k) {
        for (auto& e : per[k]) { prow.push_back(e.first); pslot.push_back(e.second); }
        poff[k + 1] = (int)prow.size();
    }
}

void build_kmer_table(const HostGraph& h, const std::vector<int>& po, const std::vector<int>& pr, std::vector<uint32_t>& keys,
                      std::vector<unsigned long long>& masks) {
    const int P = h.P;
    const size_t NW = (size_t)((P + 63) / 64);
    constexpr int K = 12;
    size_t total = 0;
    for (int k = 0; k < P; ++k) total += (size_t)std::max(0, po[k + 1] - po[k] - K + 1);
    size_t size = 64;
    while (size < 2 * total + 2) size <<= 1;
    keys.assign(size, 0xffffffffu);
    masks.assign(size * NW, 0ull);
    for (int k = 0; k < P; ++k) {
        unsigned key = 0;
        int valid = 0;
        for (int t = po[k]; t < po[k + 1]; ++t) {
            const size_t c = std::string("ACGT").find(h.lnz[pr[t]]);
            if (c == std::string::npos) { valid = 0; key = 0; continue; }
            key = ((key << 2) | (unsigned)c) & 0xffffffu;
            if (++valid < K) continue;
            unsigned hsh = (key * 2654435761u) >> 8;
            for (unsigned probe = 0;; ++probe) {
                const size_t slot = (hsh + probe) & (size - 1);
                if (keys[slot] == 0xffffffffu) keys[slot] = key;
                if (keys[slot] == key) { masks[slot * NW + (size_t)(k >> 6)] |= 1ull << (k & 63); break; }
            }
        }
    }
}

}  // namespace rg
