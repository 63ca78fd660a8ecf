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
// range argument are those of gap/rg_path_gap.hip, and the kernels are callers of the same bodies in gap/rg_path_gap_common.hpp,
// instantiated for the local kind (k_gap_dirs_local keeps its loop and calls the shared row step).  What the kind changes there:
//   * row 0 and column 0 are H = 0 (X and Y NEG), and H' = max(0, diag, Y).  The scan stays exact with the clamped H':
//     X_j = max_{k < j} (H'_k + o + e (j - k)), by the same argument (o <= 0);
//   * the source field of a direction nibble uses its fourth code: 0 = "H == 0: the walk stops here";
//   * columns past the read (j > n, base code N) never compete for the best (best_own_col).
#include <type_traits>

#include "rg_path_gap_local.hpp"

namespace rg {

namespace {

#include "../gap/rg_path_gap_common.hpp"

}  // namespace

template <int C>
__global__ __launch_bounds__(64) void k_gap_score_local(GapArgs a) {
    __shared__ int sct[40];
    gap_score_wave<C, GAP_LOCAL>(a, sct);
}

__global__ __launch_bounds__(64) void k_gap_pick_local(GapArgs a, int wcols) { gap_pick_wave<true>(a, wcols, 0); }

template <int C>
__global__ __launch_bounds__(64) void k_gap_dirs_local(GapArgs a) {
    // (the loop stands in the kernel, as in k_gap_dirs: see there)
    __shared__ int sct[40];
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    if (rs->status & ST_NO_RECORD) return;
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
    load_scores(a, lane, sct);
    row0<C, GAP_LOCAL>(H, Y, a.o, a.e, 0, lane);
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
            gap_row<C, GAP_LOCAL, false>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, lane == 0, GNEG, GNEG, dw);
#pragma unroll
            for (int w = 0; w < W; ++w) out[((long long)(t0 + u + 1) * W + w) * WAVE + lane] = dw.w[w];
            if (t0 + u == m - 1) c = own_end_col<C>(H, score, c);      // H is the end row
        }
    }
    const int col = wave_end_col<C>(c, 0);
    if (lane == 0) {
        if (col < 1 || col > n) rs->status = ST_WOULD_PANIC;          // the score pass and this one disagree: never a guess
        else rs->rec_col = col;
        atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)n);
    }
}

// (the buffer's rows come from its stride, as in k_gap_trace)
__global__ __launch_bounds__(64) void k_gap_trace_local(GapArgs a, int C) {
    gap_trace_wave<true>(a, 0, C, 1, (int)(a.dirs_stride / (gap_words(C) * WAVE)));
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
const char* launch_gap_score_local(const GapArgs& a, int nreads, int C, hipStream_t s) {
    const dim3 grid(a.P, nreads);
    RG_GAP_SWITCH_C(k_gap_score_local, (), grid, a);
    return nullptr;
}
const char* launch_gap_dirs_local(const GapArgs& a, int nreads, int C, hipStream_t s) {
    const dim3 grid(nreads);
    RG_GAP_SWITCH_C(k_gap_dirs_local, (), grid, a);
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
