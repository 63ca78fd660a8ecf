// Affine-gap pathwise alignment for gfx950 (-m 6 global, -m 7 semiglobal): exact Gotoh of the read against every path on its own.
// The rule (recurrence, choice, traceback) is stated at RG_MODE_PATHWISE_GAP in include/recgraph_hip.h.
//
//   k_gap_score<C, kSemi>   one wave per (read, path): the last-column value of the path (-m 7: its best over the rows, and the first
//                           row that attains it) -> ReadState::sink_val / path_end_row
//   k_gap_pick              one wave per read: argmax over the paths by the tie rules -> best path, end row, score
//   k_gap_dirs<C, kSemi>    one wave per read: the same row step for the picked path only, 4 bits per cell to HBM
//   k_gap_trace             one wave per read walks those bits (the walk's state is wave-uniform) -> ops and the record
//
// Mapping: lane t owns the C consecutive columns t * C .. t * C + C - 1 of the (n + 1)-column row (n + 1 <= 64 C).  H and Y of the
// current row live in registers; nothing per cell goes to HBM in k_gap_score.
//
// THE ROW STEP.  With H, Y of row i - 1 in registers, per column j (lane-local, the diagonal's neighbour through dpp_shr1):
//     Y_j  = max(H_j + o + e, Y_j + e)              H'_j = max(H_{j-1} + sc(b_i, s_j), Y_j)
// and X, the only dependency along the row, as ONE max-plus prefix scan.  Unrolling X_j = max(H_{j-1} + o + e, X_{j-1} + e) gives
//     X_j = max_{k < j} (H_k + o + e (j - k)),     H_k = max(H'_k, X_k).
// A term with H_k = X_k opens a gap out of a gap: X_k + o + e (j - k) <= X_k + e (j - k), which the unrolled chain of X_k already
// contains, BECAUSE o <= 0.  So H_k may be replaced by H'_k, which does not depend on X:
//     z_k = H'_k - e k,      X_j = (max_{k < j} z_k) + o + e j,      H_j = max(H'_j, X_j)
// — one dpp_incl_max across the wave over the lanes' z maxima (the z-space trick of RowOps::alpha in rg_pathwise.hip) gives X of a
// lane's first column; inside the lane X runs on as X_{j+1} = max(X_j, H'_j + o) + e, which needs no z or e j per column.  Column 0 has no k < 0: its running maximum is the sentinel and X[i][0] stays below every real value.
//
// RANGE.  The plan admits a batch only when (rows + n) * max(|sc|, |o + e|) < 2^28: every real value and every z lies inside
// +-2^29, and GNEG = -2^29 plus any chain of steps stays below -2^28 (it never wins) and above INT32_MIN (it never wraps).
#include <type_traits>

#include "rg_path_gap.hpp"

namespace rg {

namespace {

#include "rg_path_gap_common.hpp"      // GNEG, gap_words, ReadCols, DirWords, NoDirs, row_index

// what a wave needs besides: the score table in LDS as [path base][8], and row 0
template <int C>
__device__ __forceinline__ void gap_setup(const GapArgs& a, int lane, int* sct, int (&H)[C], int (&Y)[C]) {
    if (lane < 40) { const int b = lane >> 3, c = lane & 7; sct[lane] = c < 5 ? a.sc.t[b * 6 + c] : 0; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int j = lane * C + q;
        H[q] = j == 0 ? 0 : a.o + a.e * j;         // row 0: H = X = o + e j, Y = NEG
        Y[q] = GNEG;
    }
}

// One path row with base b.  Dirs = DirWords<C>: 4 bits per cell: bits 0-1 the source of H (1 D, 2 U, 3 L), bit 2 "Y[i][j] was
// opened from H[i-1][j]", bit 3 "an X run that goes on to column j + 1 opens here" (H[i][j] + o >= X[i][j]).
template <int C, bool kSemi, class Dirs, class Cols>
__device__ __forceinline__ void gap_row(int (&H)[C], int (&Y)[C], const Cols& rc, const int* sct, int b, int o, int e, int ej0, int lane, Dirs& dw) {
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
        int hp = max(d, y);
        if (kSemi && q == 0) {                      // -m 7: H[i][0] = 0, Y[i][0] = NEG (-m 6: the recurrence itself gives o + e i)
            hp = lane == 0 ? 0 : hp;
            y = lane == 0 ? GNEG : y;
        }
        if constexpr (kDirs) {
            dm |= (d >= y ? 1u : 0u) << q;
            ym |= (hold + o >= yold ? 1u : 0u) << q;
        }
        diag = hold;
        Y[q] = y;
        H[q] = hp;
        acc = max(acc + e, hp);
    }
    // z of the lane = acc - e (lane C + C - 1); the exclusive maximum over the lanes to the left gives X of the lane's first column,
    // and inside the lane X runs on as X_{j+1} = max(X_j, H'_j + o) + e — the same values as run + o + e j without a z or an e j per
    // column held in registers across the rows
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
            const unsigned src = hp >= x ? (((dm >> q) & 1u) ? 1u : 2u) : 3u;
            const unsigned nib = src | (((ym >> q) & 1u) << 2) | ((h + o >= x ? 1u : 0u) << 3);
            dw.w[q / 8] |= nib << (4 * (q % 8));
        }
        H[q] = h;
        x = max(x, hp + o) + e;
    }
}

// value of column qn (wave-uniform) of the lane's chunk.  As a maximum over selects with a constant arm: a chain of
// `q == qn ? H[q] : v` is turned into a dynamically indexed array by the compiler, which then moves H out of the registers
template <int C>
__device__ __forceinline__ int pick_col(const int (&H)[C], int qn) {
    int v = INT32_MIN;
#pragma unroll
    for (int q = 0; q < C; ++q) v = max(v, q == qn ? H[q] : INT32_MIN);
    return v;
}

}  // namespace

template <int C, bool kSemi>
__global__ __launch_bounds__(64) void k_gap_score(GapArgs a) {
    __shared__ int sct[40];
    const int rd = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    if (a.bad[rd] || n + 1 > C * WAVE) return;     // (k_gap_pick reports the read)
    const int pbeg = a.poff[k], m = a.poff[k + 1] - pbeg;
    int H[C], Y[C];
    ReadCols<C, false> rc;
    rc.load(a.reads + ro - 1, n, lane);
    gap_setup<C>(a, lane, sct, H, Y);
    const int ln = n / C, qn = n % C, ej0 = a.e * lane * C;
    int best = GNEG, bt = 0;
    NoDirs nd;
    // the bases of 64 path rows per gather (two dependent loads per row would cost more than the row step)
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            gap_row<C, kSemi>(H, Y, rc, sct, b, a.o, a.e, ej0, lane, nd);
            if (kSemi) {
                const int v = pick_col<C>(H, qn);
                if (v > best) { best = v; bt = t0 + u; }      // strictly better: the first row that attains the maximum
            }
        }
    }
    if (lane == ln) {
        ReadState* rs = a.state + rd;
        if (kSemi) {
            rs->sink_val[k] = best;
            rs->path_end_row[k] = m > 0 ? a.prow[pbeg + bt] : 0;
        } else {
            rs->sink_val[k] = pick_col<C>(H, qn);
        }
    }
    if (lane == 0) {
        const unsigned long long c = (unsigned long long)m * (unsigned long long)n;
        atomicAdd(a.cells, c);
        atomicAdd(a.cells + 1, c);
    }
}

// (score, end row, path) of the read: -m 6 highest score, then lowest path; -m 7 highest score, then smallest row, then lowest path
__global__ __launch_bounds__(64) void k_gap_pick(GapArgs a, int wcols, int semi) {
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
        const int v = rs->sink_val[k], r = semi ? rs->path_end_row[k] : 0;
        if (better(v, r, k, bv, br, bk)) { bv = v; br = r; bk = k; }
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const int v = __shfl_xor(bv, d, WAVE), r = __shfl_xor(br, d, WAVE), k = __shfl_xor(bk, d, WAVE);
        if (better(v, r, k, bv, br, bk)) { bv = v; br = r; bk = k; }
    }
    if (lane == 0) {
        const int end = semi ? br : a.prow[a.poff[bk + 1] - 1];
        rs->s0 = bv; rs->bound = bv; rs->trace_score = bv;
        rs->seed_path = bk; rs->fwd_path = bk; rs->rev_path = bk;
        rs->end_row = end; rs->end_row_best = end;
    }
}

template <int C, bool kSemi>
__global__ __launch_bounds__(64) void k_gap_dirs(GapArgs a) {
    __shared__ int sct[40];
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    if (rs->status & (ST_BAD_BASE | ST_WOULD_PANIC)) return;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    const int k = __builtin_amdgcn_readfirstlane(rs->fwd_path);
    const int pbeg = a.poff[k];
    int m = a.poff[k + 1] - pbeg;
    if (kSemi) m = row_index(a.prow + pbeg, m, rs->end_row) + 1;      // the rows up to the end row are all the walk can visit
    m = __builtin_amdgcn_readfirstlane(m);
    int H[C], Y[C];
    ReadCols<C, true> rc;
    rc.load(a.reads + ro - 1, n, lane);
    gap_setup<C>(a, lane, sct, H, Y);
    const int ej0 = a.e * lane * C;
    constexpr int W = gap_words(C);
    uint32_t* out = a.dirs + (long long)rd * a.dirs_stride;
    DirWords<C> dw;
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            gap_row<C, kSemi>(H, Y, rc, sct, b, a.o, a.e, ej0, lane, dw);
#pragma unroll
            for (int w = 0; w < W; ++w) out[((long long)(t0 + u + 1) * W + w) * WAVE + lane] = dw.w[w];
        }
    }
    if (lane == 0 && m > 0) atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)n);
}

// The walk of the rule.  Every value that steers it comes out of a readlane, so the state is the same in all lanes; lane 0 writes.
__global__ __launch_bounds__(64) void k_gap_trace(GapArgs a, int C, int semi) {
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    DevRecord* rec = a.rec + rd;
    if (rs->status & (ST_BAD_BASE | ST_WOULD_PANIC)) {
        if (lane == 0) { rec->status = rs->status; rec->n_ops = 0; rec->n_fwd_ops = 0; rec->score = 0; }
        return;
    }
    const int n = (int)(a.read_off[rd + 1] - a.read_off[rd]);
    const int k = rs->fwd_path;
    const int pbeg = a.poff[k], m = a.poff[k + 1] - pbeg;
    const int idx = row_index(a.prow + pbeg, m, rs->end_row);
    if (idx < 0) {
        if (lane == 0) { rec->status = ST_WOULD_PANIC; rec->n_ops = 0; rec->n_fwd_ops = 0; rec->score = 0; }
        return;
    }
    const int W = C >= 8 ? C / 8 : 1;
    const uint32_t* dirs = a.dirs + (long long)rd * a.dirs_stride;
    uint8_t* ops = a.ops + (long long)rd * a.ops_stride;
    enum { S_H, S_Y, S_X, S_XARRIVE };
    int i = idx + 1, j = n, state = S_H, nops = 0, have = -1;
    uint32_t wd[4] = {0, 0, 0, 0};
    auto emit = [&](uint8_t op) { if (lane == 0) ops[nops] = op; ++nops; };
    while (i > 0 && j > 0) {
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
    // the borders: only one state is finite there
    while (j > 0) { emit(OP_L); j -= 1; }
    while (!semi && i > 0) { emit(OP_U); i -= 1; }
    if (lane == 0) {
        rec->status = rs->status;
        rec->score = rs->trace_score;
        rec->fscore = 0.f;
        rec->end_row = rs->end_row;
        rec->end_col = n;
        rec->stop_row = 0; rec->stop_col = 0;
        rec->best_path = k; rec->rev_path = k;
        rec->fen = 0; rec->rsn = 0; rec->rec_col = 0; rec->displacement = 0;
        rec->n_ops = nops; rec->n_fwd_ops = nops;
        rec->pad = 0;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
#define RG_GAP_DISPATCH(K, grid)                                                    \
    const dim3 blk(WAVE);                                                           \
    if (semi) switch (C) {                                                          \
        case 4: RG_LAUNCH(K, (4, true), grid, blk, 0, s, a);                        \
        case 8: RG_LAUNCH(K, (8, true), grid, blk, 0, s, a);                        \
        case 16: RG_LAUNCH(K, (16, true), grid, blk, 0, s, a);                      \
        case 32: RG_LAUNCH(K, (32, true), grid, blk, 0, s, a);                      \
        default: return nullptr;                                                    \
    }                                                                               \
    switch (C) {                                                                    \
        case 4: RG_LAUNCH(K, (4, false), grid, blk, 0, s, a);                       \
        case 8: RG_LAUNCH(K, (8, false), grid, blk, 0, s, a);                       \
        case 16: RG_LAUNCH(K, (16, false), grid, blk, 0, s, a);                     \
        case 32: RG_LAUNCH(K, (32, false), grid, blk, 0, s, a);                     \
        default: return nullptr;                                                    \
    }

const char* launch_gap_score(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s) {
    const dim3 grid(a.P, nreads);
    RG_GAP_DISPATCH(k_gap_score, grid)
    return nullptr;
}
const char* launch_gap_dirs(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s) {
    const dim3 grid(nreads);
    RG_GAP_DISPATCH(k_gap_dirs, grid)
    return nullptr;
}
const char* launch_gap_pick(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s) {
    RG_LAUNCH0(k_gap_pick, dim3(nreads), dim3(WAVE), 0, s, a, C * WAVE, semi ? 1 : 0);
}
const char* launch_gap_trace(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s) {
    if (C != 4 && C != 8 && C != 16 && C != 32) return nullptr;
    RG_LAUNCH0(k_gap_trace, dim3(nreads), dim3(WAVE), 0, s, a, C, semi ? 1 : 0);
}

}  // namespace rg
