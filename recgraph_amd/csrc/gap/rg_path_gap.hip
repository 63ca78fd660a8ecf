// Affine-gap pathwise alignment for gfx950 (-m 6 global, -m 7 semiglobal): exact Gotoh of the read against every path on its own.
// The rule (recurrence, choice, traceback) is stated at RG_MODE_PATHWISE_GAP in include/recgraph_hip.h.
//
//   k_gap_score<C, kSemi>   one wave per (read, path): the last-column value of the path (-m 7: its best over the rows, and the first
//                           row that attains it) -> ReadState::sink_val / path_end_row
//   k_gap_pick              one wave per read: argmax over the paths by the tie rules -> best path, end row, score
//   k_gap_dirs<C, kSemi>    one wave per read: the same row step for the picked path only, 4 bits per cell to HBM
//   k_gap_trace             one wave per read walks those bits (the walk's state is wave-uniform) -> ops and the record
// k_gap_score, k_gap_pick and k_gap_trace are callers of the family's shared bodies in rg_path_gap_common.hpp (gap_score_wave,
// gap_pick_wave, gap_trace_wave), where the row step (gap_row), the walk (gap_walk) and the record writer live for all four kernel
// files; k_gap_dirs keeps its loop and calls gap_row.
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

#include "rg_path_gap_common.hpp"

}  // namespace

template <int C, bool kSemi>
__global__ __launch_bounds__(64) void k_gap_score(GapArgs a) {
    __shared__ int sct[40];
    gap_score_wave<C, kSemi ? GAP_SEMI : GAP_GLOBAL>(a, sct);
}

__global__ __launch_bounds__(64) void k_gap_pick(GapArgs a, int wcols, int semi) { gap_pick_wave<false>(a, wcols, semi); }

// The loop of the direction pass stands in the kernel itself, around the shared row step: as a device function inlined into
// k_gap_dirs the very same text is allocated 75 registers at C = 8 and 231 at C = 32 (here 59 / 174), and the register pin that
// repairs that costs the pass 3 - 21 % on an MI355X (profiles/gap_family_notes.md)
template <int C, bool kSemi>
__global__ __launch_bounds__(64) void k_gap_dirs(GapArgs a) {
    constexpr int kKind = kSemi ? GAP_SEMI : GAP_GLOBAL;
    __shared__ int sct[40];
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    if (rs->status & ST_NO_RECORD) return;
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
    load_scores(a, lane, sct);
    row0<C, kKind>(H, Y, a.o, a.e, 0, lane);
    const int ej0 = a.e * lane * C;
    constexpr int W = gap_words(C);
    uint32_t* out = a.dirs + (long long)rd * a.dirs_stride;
    DirWords<C> dw;
    // the bases of 64 path rows per gather, as in the score pass
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            gap_row<C, kKind, false>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, lane == 0, GNEG, GNEG, dw);
#pragma unroll
            for (int w = 0; w < W; ++w) out[((long long)(t0 + u + 1) * W + w) * WAVE + lane] = dw.w[w];
        }
    }
    if (lane == 0 && m > 0) atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)n);
}

// (the buffer's rows come from its stride: the plan sizes it as rows1 * words * 64 per read)
__global__ __launch_bounds__(64) void k_gap_trace(GapArgs a, int C, int semi) {
    gap_trace_wave<false>(a, semi, C, 1, (int)(a.dirs_stride / (gap_words(C) * WAVE)));
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
const char* launch_gap_score(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s) {
    const dim3 grid(a.P, nreads);
    if (semi) RG_GAP_SWITCH_C(k_gap_score, (, true), grid, a);
    else RG_GAP_SWITCH_C(k_gap_score, (, false), grid, a);
    return nullptr;
}
const char* launch_gap_dirs(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s) {
    const dim3 grid(nreads);
    if (semi) RG_GAP_SWITCH_C(k_gap_dirs, (, true), grid, a);
    else RG_GAP_SWITCH_C(k_gap_dirs, (, false), grid, a);
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
