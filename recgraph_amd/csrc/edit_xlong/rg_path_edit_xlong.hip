// Bit-vector edit-distance pathwise alignment of long reads for gfx950 (-m 94 global, -m 95 semiglobal): the rules of -m 56 / -m 57
// at unit costs for reads of up to 131071 bases, one cell per BIT.  The admission is stated at RG_MODE_PATHWISE_EDIT_XLONG in
// include/recgraph_hip.h; a batch whose longest read has at most 16383 bases never comes here (it runs edit/rg_path_edit.hip).
//
//   k_edit_score_xlong<kSemi>  one wave per (read, path): the last-column value of the path (-m 95: its best over the rows, and the first
//                              row that attains it) -> ReadState::sink_val / path_end_row, as k_edit_score; on the way, the boundary
//                              bits of every stripe but the read's last
//   k_gap_pick                 the kernel of gap/rg_path_gap.hip, unchanged
//   then, for round r = S - 1 down to 0, with no read-back in between:
//   k_edit_redo_xlong          one wave per read whose walk stands in stripe r: the row step again for the picked path, from boundary
//                              slot r - 1, rows 1 to the walk's row only, D0 and Ph into the one-stripe buffer (the layout of k_edit_dirs<8>)
//   k_edit_walk_xlong          the walk of k_edit_trace, resumed from the saved state; a round ends when the column leaves stripe r on
//                              the left (the state is saved) or when the walk is done (the record is written)
//
// STRIPES.  Column j >= 1 of the read is bit t = j - 1; stripe s holds bits 16384 s .. 16384 s + 16383 in the register layout of
// k_edit_score<8, .> (lane t' / 256, word (t' / 32) % 8, bit t' % 32 for the stripe-local t').  Stripes are the OUTER loop and the
// rows the inner one: a stripe's Peq is built when the stripe starts, (Pv, Mv) start as in row 0, and the wave runs down all rows
// before it turns to the next stripe.  What stripe s + 1 needs from stripe s per row is hin in {-1, 0, +1} (THE STRIPED ROW STEP in
// edit/rg_edit_bits.hpp): lane 63 collects the top bit of its unshifted Ph and Mh of 64 rows in two 64-bit masks and stores them,
// plain vector stores; the next stripe loads the two masks once per 64 rows (a per-lane load, lanes 0 and 1 hold them) and hands
// the row's bits out through v_readlane.  Two bits per row instead of the two integers of gap_xlong/: the slots of EVERY path stay,
// so the traceback starts from the picked path's slots and there is no checkpoint pass.
//
// THE SCORE of column n is tracked in the read's last stripe exactly as k_edit_score tracks it.
//
// THE WALK only ever moves left and up, so it enters every stripe at most once, in descending order, and never needs a row below the
// one it entered with: in round r an unfinished walk stands on a cell (i >= 1, j >= 1) of a stripe <= r.  A stripe above the round,
// or a state outside the matrix, ends as ST_WOULD_PANIC.  Row 0 and (global kind) column 0 need no bits: once the walk reaches row 0 it
// runs its L's through every stripe to the left in the same round, so those stripes are never rebuilt.  Round 0 finishes every walk.
// The rebuild and the walk are separate launches: the walk reads what another kernel wrote.
#include <type_traits>

#include "../edit/rg_edit_bits.hpp"
#include "rg_path_edit_xlong.hpp"

namespace rg {

namespace {

#include "../gap/rg_path_gap_common.hpp"           // GNEG, row_index, no_record, write_record

#include "../edit/rg_path_edit_lane.hpp"           // load_match_bits, EditLane<W>, store_row

constexpr int XW = EDIT_MAX_WORDS;
constexpr int XSTRIPE = EDIT_XLONG_STRIPE;
static_assert(XSTRIPE == 32 * XW * WAVE, "a stripe is one wave's vector at W = 8");

// boundary slot s of (read, path)
__device__ __forceinline__ unsigned long long* bnd_slot(const EditXLongArgs& xa, int rd, int k, int s) {
    return xa.bnd + (long long)rd * xa.bnd_stride + ((long long)k * (xa.S - 1) + s) * xa.slot_words;
}

// What a stripe takes from its left neighbour, around the rows of one 64-row block: the two masks of the block (stripe 0: the
// border's constant), and hin of row u of the block
struct HinBlock {
    unsigned long long up, down;
    __device__ __forceinline__ void begin_block(bool first, int border, const unsigned long long* from, int t0, int lane) {
        up = border > 0 ? ~0ull : 0ull;
        down = 0ull;
        if (!first) {
            // (a load per lane, not one the compiler could make scalar: the words were written by vector stores of this kernel)
            const unsigned long long v = from[2 * (t0 >> 6) + (lane & 1)];
            const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
            up = (uint32_t)__builtin_amdgcn_readlane(lo, 0) | ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(hi, 0) << 32);
            down = (uint32_t)__builtin_amdgcn_readlane(lo, 1) | ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(hi, 1) << 32);
        }
    }
    __device__ __forceinline__ int hin(int u) const { return edit_hin_of_masks(up, down, u); }
};

// a walk at the start of `round`: the first round starts it at (end row index + 1, n), every other takes the saved state.  false:
// no walk to go on with (done; the first round: the end row is no row of the path — the walk kernel reports that)
__device__ __forceinline__ bool walk_state(const EditXLongArgs& xa, int rd, int round, const ReadState* rs, int n, int pbeg, int mk, int& i, int& j,
                                           int& nops, int& steps) {
    if (round == xa.S - 1) {
        const int idx = row_index(xa.g.prow + pbeg, mk, rs->end_row);
        i = idx + 1; j = n; nops = 0; steps = 0;
        return idx >= 0;
    }
    const EditWalkState* ws = xa.walk + rd;
    i = ws->i; j = ws->j; nops = ws->nops; steps = ws->steps;
    return ws->done == 0;
}

}  // namespace

template <bool kSemi>
__global__ __launch_bounds__(64) void k_edit_score_xlong(EditXLongArgs xa) {
    constexpr int W = XW;
    __shared__ int mbits[8];
    const GapArgs& a = xa.g;
    const int rd = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    if (a.bad[rd] || n < 1 || n > xa.S * XSTRIPE) return;      // (the pick kernel reports the read)
    const int pbeg = a.poff[k];
    const int mk = a.poff[k + 1] - pbeg;
    const int m = __builtin_amdgcn_readfirstlane(min(mk, xa.rows1 - 1));      // (the slots hold the rows of the longest path)
    load_match_bits(a, lane, mbits);
    const int S = (n + XSTRIPE - 1) / XSTRIPE;
    int cur = n;                                     // the distance of column n, row 0
    int best = GNEG, bt = 0;
    for (int s = 0; s < S; ++s) {
        const bool first = s == 0, last = s == S - 1;
        const int nl = n - s * XSTRIPE;              // the read's bases from the stripe's first column on
        EditLane<W> st;
        st.load(a.reads + ro + (long long)s * XSTRIPE, nl, lane, mbits);
        // the bit of column n: in one word of one lane of the last stripe, 0 everywhere else
        uint32_t nm[W];
#pragma unroll
        for (int w = 0; w < W; ++w) nm[w] = (last && lane == (nl - 1) / (32 * W) && w == ((nl - 1) / 32) % W) ? 1u << ((nl - 1) % 32) : 0u;
        const unsigned long long* from = bnd_slot(xa, rd, k, first ? 0 : s - 1);      // (stripe 0 reads nothing, the last stripe writes nothing)
        unsigned long long* to = bnd_slot(xa, rd, k, last ? 0 : s);
        HinBlock hb;
        for (int t0 = 0; t0 < m; t0 += WAVE) {
            int myb = 4;
            if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
            hb.begin_block(first, kSemi ? 0 : 1, from, t0, lane);
            unsigned long long upo = 0, dno = 0;     // lane 63: what this block leaves
            const int cnt = min(WAVE, m - t0);
            for (int u = 0; u < cnt; ++u) {
                const int b = __builtin_amdgcn_readlane(myb, u);
                const int hin = hb.hin(u);
                uint32_t eq[W], ph[W], mh[W], d0[W];
                st.match(b, eq);
                st.deltas(eq, hin, lane, ph, mh, d0);
                if (last) {
                    uint32_t up = 0, dn = 0;
#pragma unroll
                    for (int w = 0; w < W; ++w) { up |= ph[w] & nm[w]; dn |= mh[w] & nm[w]; }
                    cur += (up != 0 ? 1 : 0) - (dn != 0 ? 1 : 0);
                    if (kSemi && -cur > best) { best = -cur; bt = t0 + u; }      // strictly better: the first row that attains the maximum
                } else {
                    upo |= (unsigned long long)(ph[W - 1] >> 31) << u;
                    dno |= (unsigned long long)(mh[W - 1] >> 31) << u;
                }
                st.finish(eq, hin, ph, mh);
            }
            if (!last && lane == WAVE - 1) {
                to[2 * (t0 >> 6)] = upo;
                to[2 * (t0 >> 6) + 1] = dno;
            }
        }
        __threadfence_block();                       // the next stripe's loads come after this stripe's stores
    }
    const int nl = n - (S - 1) * XSTRIPE;
    if (lane == (nl - 1) / (32 * W)) {
        ReadState* rs = a.state + rd;
        rs->sink_val[k] = kSemi ? best : -cur;
        if (kSemi) rs->path_end_row[k] = m > 0 ? a.prow[pbeg + bt] : 0;
    }
    if (lane == 0) {
        const unsigned long long c = (unsigned long long)mk * (unsigned long long)n;
        atomicAdd(a.cells, c);
        atomicAdd(a.cells + 1, c);
    }
}

// (the kind is a run-time argument: it is the border of stripe 0 alone)
__global__ __launch_bounds__(64) void k_edit_redo_xlong(EditXLongArgs xa, int semi, int round) {
    constexpr int W = XW;
    __shared__ int mbits[8];
    const GapArgs& a = xa.g;
    const int rd = blockIdx.x, lane = threadIdx.x;
    const ReadState* rs = a.state + rd;
    if (rs->status & ST_NO_RECORD) return;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    const int k = __builtin_amdgcn_readfirstlane(rs->fwd_path);
    if (k < 0 || k >= a.P || n < 1 || n > xa.S * XSTRIPE) return;      // (the walk kernel reports it)
    const int pbeg = a.poff[k], mk = a.poff[k + 1] - pbeg;
    int wi, wj, nops, steps;
    if (!walk_state(xa, rd, round, rs, n, pbeg, mk, wi, wj, nops, steps)) return;
    wi = __builtin_amdgcn_readfirstlane(wi);
    wj = __builtin_amdgcn_readfirstlane(wj);
    if (wi <= 0 || wj <= 0 || wj > n || (wj - 1) / XSTRIPE != round) return;      // the walk is not in this stripe (a stripe above the round: the walk kernel reports it)
    const int m = __builtin_amdgcn_readfirstlane(min(min(wi, mk), xa.rows1 - 1));      // rows 1 .. the walk's row
    load_match_bits(a, lane, mbits);
    const bool first = round == 0;
    const int nl = n - round * XSTRIPE;
    EditLane<W> st;
    st.load(a.reads + ro + (long long)round * XSTRIPE, nl, lane, mbits);
    const unsigned long long* from = bnd_slot(xa, rd, k, first ? 0 : round - 1);
    uint32_t* out = a.dirs + (long long)rd * a.dirs_stride;
    HinBlock hb;
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        hb.begin_block(first, semi ? 0 : 1, from, t0, lane);
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            const int hin = hb.hin(u);
            uint32_t eq[W], ph[W], mh[W], d0[W];
            st.match(b, eq);
            st.deltas(eq, hin, lane, ph, mh, d0);
            store_row<W>(out, t0 + u + 1, lane, d0, ph);
            st.finish(eq, hin, ph, mh);
        }
    }
    if (lane == 0 && m > 0) {
        const int cols = min(nl, XSTRIPE);           // the stripe's columns that belong to the read
        atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)cols);
    }
}

// k_edit_trace's loop, one stripe per launch: the two words of a cell — D0 and Ph of (row, word) of the one-stripe buffer — are cached
// while the walk stays on the row and inside the word's 32 columns; every value that steers the walk comes out of a uniform load or a
// readlane, so the state is the same in all lanes; lane 0 writes.  Every iteration emits one op that moves i or j down, from at most
// (rows, n): the iterations of ALL rounds are bounded by rows + n + 2, and a walk that is not at its end by then is ST_WOULD_PANIC
__global__ __launch_bounds__(64) void k_edit_walk_xlong(EditXLongArgs xa, int semi, int round) {
    constexpr int W = XW;
    const GapArgs& a = xa.g;
    const int rd = blockIdx.x, lane = threadIdx.x;
    const ReadState* rs = a.state + rd;
    DevRecord* rec = a.rec + rd;
    EditWalkState* ws = xa.walk + rd;
    const bool start = round == xa.S - 1;
    auto over = [&] { if (lane == 0) ws->done = 1; };      // the record, or its absence, is written
    auto panic = [&] { no_record(rec, lane, ST_WOULD_PANIC); over(); };
    if (rs->status & ST_NO_RECORD) {
        if (start) { no_record(rec, lane, rs->status); over(); }      // (no walk: reported in the first round)
        return;
    }
    const long long ro = a.read_off[rd];
    const int n = (int)(a.read_off[rd + 1] - ro);
    const int k = rs->fwd_path;
    if (k < 0 || k >= a.P || n < 1 || n > xa.S * XSTRIPE) {
        if (start) panic();
        return;
    }
    const int pbeg = a.poff[k], mk = a.poff[k + 1] - pbeg;
    int i, j, nops, steps;
    if (!walk_state(xa, rd, round, rs, n, pbeg, mk, i, j, nops, steps)) {
        if (start) panic();                          // the end row is no row of the picked path
        return;
    }
    // an unfinished walk stands on a cell inside the matrix, in a stripe at or below the round
    if (i < 1 || i > mk || i >= xa.rows1 || j < 1 || j > n || nops < 0 || steps < 0 || (j - 1) / XSTRIPE > round) { panic(); return; }
    const int c0 = round * XSTRIPE;                  // the stripe holds the columns c0 + 1 .. c0 + 16384
    const uint32_t* dirs = a.dirs + (long long)rd * a.dirs_stride;
    const uint8_t* read = a.reads + ro;
    uint8_t* ops = a.ops + (long long)rd * a.ops_stride;
    const int cap = mk + n + 2;
    int have = -1;
    uint32_t d0w = 0, phw = 0;
    auto emit = [&](uint8_t op) { if (lane == 0 && nops < a.ops_stride) ops[nops] = op; ++nops; };
    auto unfinished = [&] { return semi ? j > 0 : (i > 0 || j > 0); };
    while (unfinished() && steps < cap) {
        if (i > 0 && j > 0 && j <= c0) break;        // the column left the stripe on a row that needs its bits
        ++steps;
        if (i == 0) { emit(OP_L); j -= 1; continue; }
        if (j == 0) { emit(OP_U); i -= 1; continue; }
        const int t = j - 1 - c0, word = (t >> 5) & (W - 1);      // 0 <= t < 16384: the checks above
        const int key = i * W + word;
        if (have != key) {
            const uint32_t* row = dirs + (long long)i * (2 * W * WAVE) + lane;
            d0w = row[word * WAVE];
            phw = row[(W + word) * WAVE];
            have = key;
        }
        const int src = __builtin_amdgcn_readfirstlane(t >> 8);
        const uint32_t d0 = ((uint32_t)__builtin_amdgcn_readlane((int)d0w, src) >> (t & 31)) & 1u;
        const uint32_t ph = ((uint32_t)__builtin_amdgcn_readlane((int)phw, src) >> (t & 31)) & 1u;
        bool diag = d0 == 0;                         // a mismatch whose diagonal is one below
        if (!diag) diag = a.sc.t[(int)a.lnz[a.prow[pbeg + i - 1]] * 6 + (read[j - 1] & 7)] == 0;
        if (diag) { emit(OP_D); i -= 1; j -= 1; }
        else if (ph) { emit(OP_U); i -= 1; }
        else { emit(OP_L); j -= 1; }
    }
    if (!unfinished()) {
        if (nops > a.ops_stride) { panic(); return; }
        write_record(rec, lane, rs, n, 0, 0, nops);
        over();
        return;
    }
    if (steps >= cap || round == 0) { panic(); return; }
    if (lane == 0) { ws->i = i; ws->j = j; ws->nops = nops; ws->steps = steps; ws->done = 0; }      // the next stripe's round goes on from here
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static bool geometry_ok(const EditXLongArgs& a) {
    return a.S >= 2 && a.S <= EDIT_XLONG_MAX_STRIPES && a.rows1 >= 1 && a.g.P >= 1 && a.bnd && a.slot_words >= 2 * ((a.rows1 - 1 + 63) / 64) &&
           a.slot_words >= 1 && a.bnd_stride >= (long long)a.g.P * (a.S - 1) * a.slot_words;
}
static bool trace_geometry_ok(const EditXLongArgs& a, int round) {
    return geometry_ok(a) && a.walk && a.g.dirs && a.g.dirs_stride >= (long long)a.rows1 * 2 * XW * WAVE && round >= 0 && round < a.S;
}

const char* launch_edit_score_xlong(const EditXLongArgs& a, int nreads, bool semi, hipStream_t s) {
    if (!geometry_ok(a)) return nullptr;
    const dim3 grid(a.g.P, nreads);
    if (semi) RG_LAUNCH(k_edit_score_xlong, (true), grid, dim3(WAVE), 0, s, a);
    RG_LAUNCH(k_edit_score_xlong, (false), grid, dim3(WAVE), 0, s, a);
}
const char* launch_edit_redo_xlong(const EditXLongArgs& a, int nreads, bool semi, int round, hipStream_t s) {
    if (!trace_geometry_ok(a, round)) return nullptr;
    RG_LAUNCH0(k_edit_redo_xlong, dim3(nreads), dim3(WAVE), 0, s, a, semi ? 1 : 0, round);
}
const char* launch_edit_walk_xlong(const EditXLongArgs& a, int nreads, bool semi, int round, hipStream_t s) {
    if (!trace_geometry_ok(a, round)) return nullptr;
    RG_LAUNCH0(k_edit_walk_xlong, dim3(nreads), dim3(WAVE), 0, s, a, semi ? 1 : 0, round);
}

}  // namespace rg
