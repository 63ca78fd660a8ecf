// Bit-vector edit-distance pathwise alignment for gfx950 (-m 44 global, -m 45 semiglobal): the rules of -m 16 / -m 17
// (RG_MODE_PATHWISE_GAP in include/recgraph_hip.h) at unit costs — match 0, mismatch, inserted and deleted base 1 — with one cell per
// BIT.  The admission, and why the bytes are those of modes 16 / 17, is stated at RG_MODE_PATHWISE_EDIT in include/recgraph_hip.h.
//
//   k_edit_score<W, kSemi>   one wave per (read, path): the last-column value of the path (-m 45: its best over the rows, and the first
//                            row that attains it) -> ReadState::sink_val / path_end_row, as k_gap_score
//   k_gap_pick               the kernel of gap/rg_path_gap.hip, unchanged: the tie rules are its own
//   k_edit_dirs<W, kSemi>    one wave per read: the same row step for the picked path only (-m 45: up to the end row), 2 bits per cell to HBM
//   k_edit_trace             one wave per read walks those bits (the walk's state is wave-uniform) -> ops and the record
//
// LAYOUT.  Column j >= 1 of the read is bit t = j - 1 of a vector of 64 * 32 W bits: lane t / (32 W), word (t / 32) % W, bit t % 32;
// W = 1, 2, 4 or 8 is the smallest with n <= 2048 W for the longest read of the batch, so a read of up to 16383 bases sits whole in one
// wave's registers: no stripes, no boundary buffer.  Per lane: Peq[b][W] for the five path bases (bit t: the score table says
// sc(b, read[t]) == 0, so N follows the table), Pv[W] (all ones: row 0 is 0, 1, 2, ...) and Mv[W] (0).  Nothing per cell goes to HBM
// in k_edit_score.
//
// THE ROW STEP and its three pieces are edit/rg_edit_bits.hpp's.  Across the lanes: the wide addition's carries are one 64-bit scalar
// addition on two ballots (edit_carry_mask), the two shifts take the top bit of the lane to the left through dpp_shr1; lane 0 takes hin,
// +1 in the global kind (column 0 is i) and 0 in the semiglobal kind (column 0 is 0).
//
// THE SCORE of column n is tracked by the lane that owns bit n - 1, as a distance: n in row 0, +1 per row where the bit of Ph is set,
// -1 where the bit of Mh is; the stored score is its negative.  No cross-lane operation per row: the masks of the other lanes are 0.
//
// THE WALK from (end row index, n).  Stop at j == 0 in the semiglobal kind, or at (0, 0).  Row 0: L.  Column 0 (global): U.
// Otherwise, with "match" = sc(path base of row i, read base j) == 0 recomputed from the bases: D if match or not D0[i][j] (a mismatch
// whose diagonal is one below); else U if Ph[i][j] (the cell above is one below); else L — D > U > L, the order of the rule of mode 6,
// whose Y and X states are H itself at o = 0.
#include <type_traits>

#include "rg_edit_bits.hpp"
#include "rg_path_edit.hpp"

namespace rg {

namespace {

#include "../gap/rg_path_gap_common.hpp"           // GNEG, row_index, no_record, write_record, RG_SWITCH_C

#include "rg_path_edit_lane.hpp"                    // load_match_bits, EditLane<W>, store_row

}  // namespace

template <int W, bool kSemi>
__global__ __launch_bounds__(64) void k_edit_score(GapArgs a) {
    __shared__ int mbits[8];
    const int rd = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    if (a.bad[rd] || n < 1 || n > 32 * W * WAVE) return;     // (the pick kernel reports a bad read, the direction pass one that is too long)
    const int pbeg = a.poff[k], m = a.poff[k + 1] - pbeg;
    load_match_bits(a, lane, mbits);
    EditLane<W> st;
    st.load(a.reads + ro, n, lane, mbits);
    // the bit of column n: in one word of one lane, 0 everywhere else
    uint32_t nm[W];
#pragma unroll
    for (int w = 0; w < W; ++w) nm[w] = (lane == (n - 1) / (32 * W) && w == ((n - 1) / 32) % W) ? 1u << ((n - 1) % 32) : 0u;
    int cur = n;                                     // the distance of column n, row 0
    int best = GNEG, bt = 0;
    // the bases of 64 path rows per gather, as gap_score_wave does
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            uint32_t eq[W], ph[W], mh[W], d0[W];
            st.match(b, eq);
            st.deltas(eq, kSemi ? 0 : 1, lane, ph, mh, d0);
            uint32_t up = 0, dn = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) { up |= ph[w] & nm[w]; dn |= mh[w] & nm[w]; }
            cur += (up != 0 ? 1 : 0) - (dn != 0 ? 1 : 0);
            if (kSemi && -cur > best) { best = -cur; bt = t0 + u; }      // strictly better: the first row that attains the maximum
            st.finish(eq, kSemi ? 0 : 1, ph, mh);
        }
    }
    if (lane == (n - 1) / (32 * W)) {
        ReadState* rs = a.state + rd;
        rs->sink_val[k] = kSemi ? best : -cur;
        if (kSemi) rs->path_end_row[k] = m > 0 ? a.prow[pbeg + bt] : 0;
    }
    if (lane == 0) {
        const unsigned long long c = (unsigned long long)m * (unsigned long long)n;
        atomicAdd(a.cells, c);
        atomicAdd(a.cells + 1, c);
    }
}

template <int W, bool kSemi>
__global__ __launch_bounds__(64) void k_edit_dirs(GapArgs a) {
    __shared__ int mbits[8];
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    if (rs->status & ST_NO_RECORD) return;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    const int k = __builtin_amdgcn_readfirstlane(rs->fwd_path);
    const int rows1 = (int)(a.dirs_stride / (2 * W * WAVE));      // (the plan sizes the buffer as rows1 * 2 W * 64 words per read)
    if (n < 1 || n > 32 * W * WAVE || k < 0 || k >= a.P || rows1 < 1) {
        if (lane == 0) rs->status = ST_WOULD_PANIC;
        return;
    }
    const int pbeg = a.poff[k];
    int m = a.poff[k + 1] - pbeg;
    if (kSemi) m = row_index(a.prow + pbeg, m, rs->end_row) + 1;      // the rows up to the end row are all the walk can visit
    m = __builtin_amdgcn_readfirstlane(min(m, rows1 - 1));
    load_match_bits(a, lane, mbits);
    EditLane<W> st;
    st.load(a.reads + ro, n, lane, mbits);
    uint32_t* out = a.dirs + (long long)rd * a.dirs_stride;
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            uint32_t eq[W], ph[W], mh[W], d0[W];
            st.match(b, eq);
            st.deltas(eq, kSemi ? 0 : 1, lane, ph, mh, d0);
            store_row<W>(out, t0 + u + 1, lane, d0, ph);
            st.finish(eq, kSemi ? 0 : 1, ph, mh);
        }
    }
    if (lane == 0 && m > 0) atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)n);
}

// W is a run-time argument here (a power of two: 1, 2, 4, 8).  The two words of a cell — D0 and Ph of (row, word) — are cached while
// the walk stays on the row and inside the word's 32 columns; every value that steers the walk comes out of a uniform load or a
// readlane, so the state is the same in all lanes; lane 0 writes.  Every iteration emits one op that moves i or j down, from at most
// (rows, n): the loop is bounded by rows + n + 2, and a walk that is not at its end by then is ST_WOULD_PANIC with no record, as gap_walk's
__global__ __launch_bounds__(64) void k_edit_trace(GapArgs a, int W, int semi) {
    const int rd = blockIdx.x, lane = threadIdx.x;
    const ReadState* rs = a.state + rd;
    DevRecord* rec = a.rec + rd;
    if (rs->status & ST_NO_RECORD) { no_record(rec, lane, rs->status); return; }
    const long long ro = a.read_off[rd];
    const int n = (int)(a.read_off[rd + 1] - ro);
    const int k = rs->fwd_path;
    const int rows1 = (int)(a.dirs_stride / (2 * W * WAVE));
    if (k < 0 || k >= a.P || n < 1 || n > 32 * W * WAVE) { no_record(rec, lane, ST_WOULD_PANIC); return; }
    const int pbeg = a.poff[k];
    const int idx = row_index(a.prow + pbeg, a.poff[k + 1] - pbeg, rs->end_row);
    if (idx < 0 || idx + 1 >= rows1) { no_record(rec, lane, ST_WOULD_PANIC); return; }
    const uint32_t* dirs = a.dirs + (long long)rd * a.dirs_stride;
    const uint8_t* read = a.reads + ro;
    uint8_t* ops = a.ops + (long long)rd * a.ops_stride;
    const int ws = 31 - __clz(W);                    // (W is a power of two)
    int i = idx + 1, j = n, nops = 0, steps = 0, have = -1;
    const int cap = i + n + 2;
    uint32_t d0w = 0, phw = 0;
    auto emit = [&](uint8_t op) { if (lane == 0 && nops < a.ops_stride) ops[nops] = op; ++nops; };
    while ((semi ? j > 0 : (i > 0 || j > 0)) && steps < cap) {
        ++steps;
        if (i == 0) { emit(OP_L); j -= 1; continue; }
        if (j == 0) { emit(OP_U); i -= 1; continue; }
        const int t = j - 1, word = (t >> 5) & (W - 1);
        const int key = i * W + word;
        if (have != key) {
            const uint32_t* row = dirs + (long long)i * (2 * W * WAVE) + lane;
            d0w = row[word * WAVE];
            phw = row[(W + word) * WAVE];
            have = key;
        }
        const int src = __builtin_amdgcn_readfirstlane(t >> (5 + ws));
        const uint32_t d0 = ((uint32_t)__builtin_amdgcn_readlane((int)d0w, src) >> (t & 31)) & 1u;
        const uint32_t ph = ((uint32_t)__builtin_amdgcn_readlane((int)phw, src) >> (t & 31)) & 1u;
        bool diag = d0 == 0;                         // a mismatch whose diagonal is one below
        if (!diag) diag = a.sc.t[(int)a.lnz[a.prow[pbeg + i - 1]] * 6 + (read[t] & 7)] == 0;
        if (diag) { emit(OP_D); i -= 1; j -= 1; }
        else if (ph) { emit(OP_U); i -= 1; }
        else { emit(OP_L); j -= 1; }
    }
    if ((semi ? j > 0 : (i > 0 || j > 0)) || nops > a.ops_stride) { no_record(rec, lane, ST_WOULD_PANIC); return; }
    write_record(rec, lane, rs, n, 0, 0, nops);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
// the word counts that exist, stated once: every launcher checks W through words_ok, and the dispatch of the two templates lists the same
#define RG_EDIT_WORDS 1, 2, 4, 8
static bool words_ok(int W) { for (const int w : {RG_EDIT_WORDS}) if (w == W) return true; return false; }
static bool geometry_ok(const GapArgs& a, int W) { return words_ok(W) && a.dirs && a.dirs_stride >= 2ll * W * WAVE && a.dirs_stride % (2 * W * WAVE) == 0; }

const char* launch_edit_score(const GapArgs& a, int nreads, int W, bool semi, hipStream_t s) {
    if (!words_ok(W)) return nullptr;
    const dim3 grid(a.P, nreads);
    const int C = W;                                 // (the dispatch macro switches on `C`)
    if (semi) RG_SWITCH_C((RG_EDIT_WORDS), k_edit_score, (, true), grid, dim3(WAVE), 0, s, a);
    else RG_SWITCH_C((RG_EDIT_WORDS), k_edit_score, (, false), grid, dim3(WAVE), 0, s, a);
    return nullptr;
}
const char* launch_edit_dirs(const GapArgs& a, int nreads, int W, bool semi, hipStream_t s) {
    if (!geometry_ok(a, W)) return nullptr;
    const dim3 grid(nreads);
    const int C = W;
    if (semi) RG_SWITCH_C((RG_EDIT_WORDS), k_edit_dirs, (, true), grid, dim3(WAVE), 0, s, a);
    else RG_SWITCH_C((RG_EDIT_WORDS), k_edit_dirs, (, false), grid, dim3(WAVE), 0, s, a);
    return nullptr;
}
const char* launch_edit_trace(const GapArgs& a, int nreads, int W, bool semi, hipStream_t s) {
    if (!geometry_ok(a, W)) return nullptr;
    RG_LAUNCH0(k_edit_trace, dim3(nreads), dim3(WAVE), 0, s, a, W, semi ? 1 : 0);
}

}  // namespace rg
