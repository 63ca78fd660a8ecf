// Local affine-gap pathwise alignment for gfx950 (-m 12): Smith-Waterman-Gotoh of the read against every path on its own.
// The rule (recurrence, choice, traceback) is stated at RG_MODE_PATHWISE_GAP_LOCAL in include/recgraph_hip.h.
//
//   k_gap_score_local<C>   one wave per (read, path): the best H of the path over rows >= 1 and the read's columns, and the first
//                          row that attains it -> ReadState::sink_val / path_end_row
//   k_gap_pick_local       one wave per read: argmax over the paths (value, then smallest row, then lowest path: k_gap_pick's -m 7
//                          order); a best value of 0 is "no local alignment": ST_UNALIGNED
//   k_gap_dirs_local<C>    one wave per read: the same row step for the picked path up to the end row, 4 bits per cell to HBM; at
//                          the end row the smallest column that holds the score -> ReadState::rec_col
//   k_gap_trace_local      one wave per read walks those bits from (end row, end column) until a cell with H == 0
//
// The mapping (lane t owns the C consecutive columns t * C .. t * C + C - 1), the row step with X as one max-plus prefix scan and the
// range argument are those of gap/rg_path_gap.hip; this file is a specialised copy of that row step, so that the code objects of
// -m 6 / -m 7 stay what they are.  What differs:
//   * row 0 and column 0 are H = 0 (X and Y NEG), and H' = max(0, diag, Y).  The scan stays exact with the clamped H':
//     X_j = max_{k < j} (H'_k + o + e (j - k)), by the same argument (o <= 0);
//   * the source field of a direction nibble uses its fourth code: 0 = "H == 0: the walk stops here";
//   * columns past the read (j > n, base code N) depend only on cells to their left, so they cannot disturb real cells — but they
//     CAN hold positive values (X running on, or a matrix whose N entries are positive), so they never compete for the best: every
//     lane compares its columns against a limit (all, the boundary lane's first n % C + 1, none).
#include <type_traits>

#include "rg_path_gap_local.hpp"

namespace rg {

namespace {

#include "../gap/rg_path_gap_common.hpp"      // GNEG, gap_words, ReadCols, DirWords, NoDirs, row_index

// the score table in LDS as [path base][8], and row 0: H = 0 everywhere, Y = NEG
template <int C>
__device__ __forceinline__ void local_setup(const GapArgs& a, int lane, int* sct, int (&H)[C], int (&Y)[C]) {
    if (lane < 40) { const int b = lane >> 3, c = lane & 7; sct[lane] = c < 5 ? a.sc.t[b * 6 + c] : 0; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < C; ++q) { H[q] = 0; Y[q] = GNEG; }
}

// One path row with base b.  Dirs = DirWords<C>: 4 bits per cell: bits 0-1 the source of H (0 none: H == 0, 1 D, 2 U, 3 L), bit 2
// "Y[i][j] was opened from H[i-1][j]", bit 3 "an X run that goes on to column j + 1 opens here" (H[i][j] + o >= X[i][j]).
template <int C, class Dirs, class Cols>
__device__ __forceinline__ void local_row(int (&H)[C], int (&Y)[C], const Cols& rc, const int* sct, int b, int o, int e, int ej0, int lane, Dirs& dw) {
    constexpr bool kDirs = !std::is_same_v<Dirs, NoDirs>;
    const int* srow = sct + b * 8;
    const int oe = o + e;
    int diag = dpp_shr1(H[C - 1], GNEG);           // lane 0: column 0 has no diagonal
    unsigned dm = 0, ym = 0;
    int acc = GNEG;                                // max_q (H'_q + e (C - 1 - q)): the lane's z maximum, taken at its last column
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int hold = H[q], yold = Y[q];
        int y = max(hold + oe, yold + e);
        const int d = diag + srow[rc.get(q)];
        int hp = max(max(d, y), 0);
        if (q == 0) {                               // H[i][0] = 0, Y[i][0] = NEG
            hp = lane == 0 ? 0 : hp;
            y = lane == 0 ? GNEG : y;
        }
        if constexpr (kDirs) {
            // d >= y and hold + o >= yold as sign bits (every difference lies inside +-2^31): a select of the constant 1 << q per
            // column kept two dozen registers of constants
            dm |= ((unsigned)(y - d - 1) >> 31) << q;
            ym |= ((unsigned)(yold - (hold + o) - 1) >> 31) << q;
        }
        diag = hold;
        Y[q] = y;
        H[q] = hp;
        acc = max(acc + e, hp);
    }
    const int zl = dpp_shr1(dpp_incl_max(acc - (ej0 + e * (C - 1)), GNEG), GNEG);
    int x = zl + o + ej0;
    if constexpr (kDirs) {
#pragma unroll
        for (int w = 0; w < gap_words(C); ++w) dw.w[w] = 0;
    }
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int hp = H[q];
        const int h = max(hp, x);
        if constexpr (kDirs) {
            const unsigned t = (unsigned)(x - hp - 1) >> 31;                  // hp >= x
            // L 3; else D 1 if d >= y, U 2 otherwise; and 0, "the walk stops here", where h == 0 (h >= 0).  As arithmetic on sign bits:
            // as selects (with the constants 1 << q of the masks above) k_gap_dirs_local<32> took 238 registers
            const unsigned src = (3u - t - (t & (dm >> q))) & (unsigned)(-h >> 31);
            const unsigned nib = src | (((ym >> q) & 1u) << 2) | (((unsigned)(x - (h + o) - 1) >> 31) << 3);     // h + o >= x
            dw.w[q / 8] |= nib << (4 * (q % 8));
        }
        H[q] = h;
        x = max(x, hp + o) + e;
    }
}

// the last of the lane's columns that belongs to the read (column j = lane * C + q, 1 <= j <= n; column 0 is H = 0 and never wins)
__device__ __forceinline__ int col_limit(int lane, int n, int C) { return min(C - 1, n - lane * C); }

}  // namespace

template <int C>
__global__ __launch_bounds__(64) void k_gap_score_local(GapArgs a) {
    __shared__ int sct[40];
    const int rd = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    if (a.bad[rd] || n + 1 > C * WAVE) return;     // (k_gap_pick_local reports the read)
    const int pbeg = a.poff[k], m = a.poff[k + 1] - pbeg;
    int H[C], Y[C];
    ReadCols<C, false> rc;
    rc.load(a.reads + ro - 1, n, lane);
    local_setup<C>(a, lane, sct, H, Y);
    const int ej0 = a.e * lane * C, qlim = col_limit(lane, n, C);
    int best = 0, bt = 0;                          // per lane, over its own columns
    NoDirs nd;
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            local_row<C>(H, Y, rc, sct, b, a.o, a.e, ej0, lane, nd);
            int v = 0;
#pragma unroll
            for (int q = 0; q < C; ++q) v = max(v, q <= qlim ? H[q] : 0);
            if (v > best) { best = v; bt = t0 + u; }          // strictly better: the first row that attains the lane's maximum
        }
    }
    // the one cross-lane step: highest value, then the smallest row
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const int v = __shfl_xor(best, d, WAVE), t = __shfl_xor(bt, d, WAVE);
        if (v > best || (v == best && t < bt)) { best = v; bt = t; }
    }
    if (lane == 0) {
        ReadState* rs = a.state + rd;
        rs->sink_val[k] = best;
        rs->path_end_row[k] = m > 0 ? a.prow[pbeg + bt] : 0;
        const unsigned long long c = (unsigned long long)m * (unsigned long long)n;
        atomicAdd(a.cells, c);
        atomicAdd(a.cells + 1, c);
    }
}

// (score, end row, path) of the read: highest score, then smallest row, then lowest path; score 0: no local alignment
__global__ __launch_bounds__(64) void k_gap_pick_local(GapArgs a, int wcols) {
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    const int n = (int)(a.read_off[rd + 1] - a.read_off[rd]);
    if (a.bad[rd] || n + 1 > wcols) {
        if (lane == 0) rs->status = a.bad[rd] ? ST_BAD_BASE : ST_WOULD_PANIC;
        return;
    }
    int bv = INT32_MIN, br = INT32_MAX, bk = INT32_MAX;
    auto better = [](int v, int r, int k, int v2, int r2, int k2) { return v != v2 ? v > v2 : r != r2 ? r < r2 : k < k2; };
    for (int k = lane; k < a.P; k += WAVE) {
        const int v = rs->sink_val[k], r = rs->path_end_row[k];
        if (better(v, r, k, bv, br, bk)) { bv = v; br = r; bk = k; }
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const int v = __shfl_xor(bv, d, WAVE), r = __shfl_xor(br, d, WAVE), k = __shfl_xor(bk, d, WAVE);
        if (better(v, r, k, bv, br, bk)) { bv = v; br = r; bk = k; }
    }
    if (lane == 0) {
        if (bv <= 0 || bk < 0 || bk >= a.P) { rs->status = bv == 0 ? ST_UNALIGNED : ST_WOULD_PANIC; return; }
        rs->s0 = bv; rs->bound = bv; rs->trace_score = bv;
        rs->seed_path = bk; rs->fwd_path = bk; rs->rev_path = bk;
        rs->end_row = br; rs->end_row_best = br;
    }
}

template <int C>
__global__ __launch_bounds__(64) void k_gap_dirs_local(GapArgs a) {
    __shared__ int sct[40];
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    if (rs->status & (ST_BAD_BASE | ST_WOULD_PANIC | ST_UNALIGNED)) return;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    const int k = __builtin_amdgcn_readfirstlane(rs->fwd_path);
    const int score = __builtin_amdgcn_readfirstlane(rs->trace_score);
    const int pbeg = a.poff[k];
    // the rows up to the end row are all the walk can visit
    const int m = __builtin_amdgcn_readfirstlane(row_index(a.prow + pbeg, a.poff[k + 1] - pbeg, rs->end_row) + 1);
    if (m <= 0) {
        if (lane == 0) rs->status = ST_WOULD_PANIC;
        return;
    }
    int H[C], Y[C];
    ReadCols<C, true> rc;
    rc.load(a.reads + ro - 1, n, lane);
    local_setup<C>(a, lane, sct, H, Y);
    const int ej0 = a.e * lane * C;
    constexpr int W = gap_words(C);
    uint32_t* out = a.dirs + (long long)rd * a.dirs_stride;
    DirWords<C> dw;
    int c = C;
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            local_row<C>(H, Y, rc, sct, b, a.o, a.e, ej0, lane, dw);
#pragma unroll
            for (int w = 0; w < W; ++w) out[((long long)(t0 + u + 1) * W + w) * WAVE + lane] = dw.w[w];
            if (t0 + u == m - 1) {
                // H is the end row: its smallest column that holds the score (lowest lane, then lowest column of that lane).  No test
                // against the read's end: the score pass found such a column inside the read, so the smallest one is inside it too
                // (checked below).  Inside the loop: behind it, H live out of the loop cost k_gap_dirs_local<32> 10 registers
#pragma unroll
                for (int q = C - 1; q >= 0; --q) c = H[q] == score ? q : c;
            }
        }
    }
    const unsigned long long hit = __ballot(c < C);
    const int l = __builtin_amdgcn_readfirstlane(hit ? __ffsll((long long)hit) - 1 : 0);
    const int cl = __builtin_amdgcn_readlane(c, l);
    if (lane == 0) {
        const int col = l * C + cl;
        if (hit == 0ull || col < 1 || col > n) rs->status = ST_WOULD_PANIC;          // the score pass and this one disagree: never a guess
        else rs->rec_col = col;
        atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)n);
    }
}

// The walk of the rule.  Every value that steers it comes out of a readlane, so the state is the same in all lanes; lane 0 writes.
// The loop is bounded: a wrong direction word ends as ST_WOULD_PANIC, never as a hang.
__global__ __launch_bounds__(64) void k_gap_trace_local(GapArgs a, int C) {
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    DevRecord* rec = a.rec + rd;
    auto no_record = [&](uint32_t st) {
        if (lane == 0) { rec->status = st; rec->n_ops = 0; rec->n_fwd_ops = 0; rec->score = 0; }
    };
    if (rs->status & (ST_BAD_BASE | ST_WOULD_PANIC | ST_UNALIGNED)) { no_record(rs->status); return; }
    const int n = (int)(a.read_off[rd + 1] - a.read_off[rd]);
    const int k = rs->fwd_path;
    const int pbeg = a.poff[k], m = a.poff[k + 1] - pbeg;
    const int idx = row_index(a.prow + pbeg, m, rs->end_row);
    const int end_col = rs->rec_col;
    if (idx < 0 || end_col < 1 || end_col > n) { no_record(ST_WOULD_PANIC); return; }
    const int W = C >= 8 ? C / 8 : 1;
    const uint32_t* dirs = a.dirs + (long long)rd * a.dirs_stride;
    uint8_t* ops = a.ops + (long long)rd * a.ops_stride;
    enum { S_H, S_Y, S_X, S_XARRIVE };
    int i = idx + 1, j = end_col, state = S_H, nops = 0, have = -1;
    // Iterations of a valid walk.  A D is one (H: emit, i and j move).  A U is at most two: "H -> Y", then "Y: emit, i moves".  An L is
    // at most THREE: "H -> X", "X: emit, j moves", "arrive: back to H or on in X" — and with o == 0 every arrival goes back to H
    // (h + o >= x always holds), so a run of g L's takes 3 g.  Every emitted op moves i or j down, from at most (rows, n): at most
    // 2 per row + 3 per column, and one more for the stop.  3 (rows + n) + 3 covers it.
    const int cap = 3 * (m + n) + 3;
    int steps = 0;
    bool stopped = false;
    uint32_t wd[4] = {0, 0, 0, 0};
    auto emit = [&](uint8_t op) { if (lane == 0 && nops < a.ops_stride) ops[nops] = op; ++nops; };
    while (i > 0 && j > 0 && steps < cap) {
        ++steps;
        if (have != i) {
#pragma unroll
            for (int w = 0; w < 4; ++w)
                if (w < W) wd[w] = dirs[((long long)i * W + w) * WAVE + lane];
            have = i;
        }
        const int q = j % C, wsel = q >> 3;
        const uint32_t word = wsel == 0 ? wd[0] : wsel == 1 ? wd[1] : wsel == 2 ? wd[2] : wd[3];
        const uint32_t cell = ((uint32_t)__builtin_amdgcn_readlane((int)word, __builtin_amdgcn_readfirstlane(j / C)) >> (4 * (q & 7))) & 15u;
        if (state == S_XARRIVE) {                   // an L was walked into (i, j): does the run open here?
            state = (cell & 8u) ? S_H : S_X;
        } else if (state == S_H) {
            const uint32_t src = cell & 3u;
            if (src == 0u) { stopped = true; break; }          // H == 0: checked first
            if (src == 1u) { emit(OP_D); i -= 1; j -= 1; }
            else state = src == 2u ? S_Y : S_X;
        } else if (state == S_Y) {
            emit(OP_U);
            i -= 1;
            state = (cell & 4u) ? S_H : S_Y;
        } else {
            emit(OP_L);
            j -= 1;
            state = S_XARRIVE;
        }
    }
    // a border cell is H = 0 (X and Y are NEG there): the walk may arrive in H, or by an L whose run opens on column 0
    const bool border = (i == 0 || j == 0) && (state == S_H || (state == S_XARRIVE && j == 0));
    if (!(stopped || border) || nops < 1 || nops > a.ops_stride) { no_record(ST_WOULD_PANIC); return; }
    if (lane == 0) {
        rec->status = rs->status;
        rec->score = rs->trace_score;
        rec->fscore = 0.f;
        rec->end_row = rs->end_row;
        rec->end_col = end_col;
        rec->stop_row = i > 0 ? a.prow[pbeg + i - 1] : 0;
        rec->stop_col = j;
        rec->best_path = k; rec->rev_path = k;
        rec->fen = 0; rec->rsn = 0; rec->rec_col = 0; rec->displacement = 0;
        rec->n_ops = nops; rec->n_fwd_ops = nops;
        rec->pad = 0;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
#define RG_GAP_LOCAL_DISPATCH(K, grid)                                              \
    const dim3 blk(WAVE);                                                           \
    switch (C) {                                                                    \
        case 4: RG_LAUNCH(K, (4), grid, blk, 0, s, a);                              \
        case 8: RG_LAUNCH(K, (8), grid, blk, 0, s, a);                              \
        case 16: RG_LAUNCH(K, (16), grid, blk, 0, s, a);                            \
        case 32: RG_LAUNCH(K, (32), grid, blk, 0, s, a);                            \
        default: return nullptr;                                                    \
    }

const char* launch_gap_score_local(const GapArgs& a, int nreads, int C, hipStream_t s) {
    const dim3 grid(a.P, nreads);
    RG_GAP_LOCAL_DISPATCH(k_gap_score_local, grid)
    return nullptr;
}
const char* launch_gap_dirs_local(const GapArgs& a, int nreads, int C, hipStream_t s) {
    const dim3 grid(nreads);
    RG_GAP_LOCAL_DISPATCH(k_gap_dirs_local, grid)
    return nullptr;
}
const char* launch_gap_pick_local(const GapArgs& a, int nreads, int C, hipStream_t s) {
    RG_LAUNCH0(k_gap_pick_local, dim3(nreads), dim3(WAVE), 0, s, a, C * WAVE);
}
const char* launch_gap_trace_local(const GapArgs& a, int nreads, int C, hipStream_t s) {
    if (C != 4 && C != 8 && C != 16 && C != 32) return nullptr;
    RG_LAUNCH0(k_gap_trace_local, dim3(nreads), dim3(WAVE), 0, s, a, C);
}

}  // namespace rg
