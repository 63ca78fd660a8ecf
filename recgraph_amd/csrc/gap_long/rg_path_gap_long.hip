// Affine-gap pathwise alignment of long reads for gfx950 (-m 16 global, -m 17 semiglobal, -m 22 local): the rules of -m 6, -m 7 and
// -m 12 (RG_MODE_PATHWISE_GAP and RG_MODE_PATHWISE_GAP_LOCAL in include/recgraph_hip.h) for reads of up to 16383 bases.
//
//   k_gap_score_long<kind>    one wave per (read, path) -> ReadState::sink_val / path_end_row, as k_gap_score / k_gap_score_local
//   k_gap_pick, k_gap_pick_local   the kernels of gap/ and gap_local/, launched with the striped width
//   k_gap_dirs_long<kind>     one wave per read: the same row step for the picked path, 4 bits per cell to HBM
//   k_gap_trace_long, k_gap_trace_local_long   one wave per read walks those bits
// The row step (gap_row, striped form), the nibble lookup, the walk and the record writer are the family's, in
// gap/rg_path_gap_common.hpp; the stripe geometry and the boundary exchange live in rg_path_gap_long_rows.hpp, which gap_xlong/
// (-m 56 / -m 57 / -m 62: the same stripes with the direction words of one stripe at a time) includes as well.
//
// COLUMN STRIPES, ONE WAVE.  A read of n bases has ceil((n + 1) / 2048) stripes of 2048 columns; inside a stripe lane t owns the 32
// columns s * 2048 + t * 32 .. + 31, and the row step is the one of gap/rg_path_gap.hip with its stripe inputs: H and Y of
// the current row in registers, X as one max-plus prefix scan over z_k = H'_k - e k with k the GLOBAL column.  The wave walks the
// stripes of its (read, path) one after the other, all rows of a stripe before the next.  Per row, a stripe needs two integers from
// everything to its left:
//   * H[i-1][c0-1], the diagonal of its first column (row 1: the closed form of row 0, o + e (c0 - 1), or 0 in the local kind);
//   * max_{k < c0} z_k of row i, which joins the in-wave exclusive prefix: X_j = (max(prefix, saved) ) + o + e j.
// Both live in a boundary buffer of 2 ints per path row, updated in place: a block of 64 rows loads its old values with the base
// gather (lane u holds row t0 + u) BEFORE any of its rows writes, hands them out with v_readlane, collects the new ones into lane u and
// stores them coalesced at the end of the block.  Stripe 0 reads nothing, a read's last stripe writes nothing, so a read of at most
// 2047 bases in a long batch touches no boundary value.
//
// RANGE.  The plan's bound is the one of -m 6: (rows + n) * max(|sc|, |o + e|) < 2^28, so every real H, X, Y lies inside +-2^28.  In
// global columns z_k = H'_k - e k with 0 <= -e k <= |e| n < 2^28 (|e| <= |o + e| because both are <= 0): H'_k <= z_k < 2^29, so a
// real z lies above -2^28 — above the sentinel GNEG = -2^29, which therefore never wins — and below 2^29, and X = z + o + e j with
// j > k is a sum of real steps again.  GNEG plus any chain of steps stays above -2^29 - 2^28 - 2^28: it never wraps.
#include <type_traits>

#include "rg_path_gap_long.hpp"

namespace rg {

namespace {

#include "../gap/rg_path_gap_common.hpp"
#include "rg_path_gap_long_rows.hpp"                // CL, STRIPE, WL, Boundary

}  // namespace

template <int kKind>
__global__ __launch_bounds__(64) void k_gap_score_long(GapLongArgs la) {
    constexpr bool kSemi = kKind == GAP_SEMI, kLocal = kKind == GAP_LOCAL;
    __shared__ int sct[40];
    const GapArgs& a = la.g;
    const int rd = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    if (a.bad[rd] || n + 1 > la.S * STRIPE) return;      // (the pick kernel reports the read)
    const int pbeg = a.poff[k], m = min(a.poff[k + 1] - pbeg, la.rows1 - 1);
    load_scores(a, lane, sct);
    const int S = (n + STRIPE) / STRIPE;                 // the read's own stripes: ceil((n + 1) / 2048)
    Boundary bd;
    bd.h = la.bnd + (long long)rd * la.bnd_stride + 2ll * k * la.rows1;
    bd.z = bd.h + la.rows1;
    int best = kLocal ? 0 : GNEG, bt = 0;
    NoDirs nd;
    for (int s = 0; s < S; ++s) {
        const int c0 = s * STRIPE;
        const bool first = s == 0, last = s == S - 1;
        int H[CL], Y[CL];
        ReadCols<CL, false> rc;
        rc.load(a.reads + ro - 1, n, lane, c0);
        row0<CL, kKind>(H, Y, a.o, a.e, c0, lane);
        const int ej0 = a.e * (c0 + lane * CL);
        const int nl = n - c0;                           // the last stripe: 0 <= nl <= 2047, the read's last column is (ln, qn)
        const int ln = nl / CL, qn = nl % CL;
        const int qlim = min(CL - 1, nl - lane * CL);    // the lane's columns 0 .. qlim belong to the read (none: negative)
        bd.begin_stripe(first, kLocal ? 0 : a.o + a.e * (c0 - 1));      // H[0][c0 - 1]
        for (int t0 = 0; t0 < m; t0 += WAVE) {
            int myb = 4;
            if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
            bd.begin_block(first, t0, m, lane);
            const int cnt = min(WAVE, m - t0);
            for (int u = 0; u < cnt; ++u) {
                const int b = __builtin_amdgcn_readlane(myb, u);
                const int incl = gap_row<CL, kKind, true>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, first && lane == 0, bd.dnext, bd.zin(u), nd);
                bd.after_row(u, lane, H[CL - 1], incl);
                if (kSemi) {
                    const int v = pick_col(H, qn);
                    if (last && v > best) { best = v; bt = t0 + u; }      // strictly better: the first row that attains the maximum
                }
                if (kLocal) {
                    const int v = best_own_col(H, qlim);
                    // rows repeat per stripe: highest value, then the smallest row (column 0 holds 0 and never beats the initial 0)
                    if (v > best || (v == best && t0 + u < bt)) { best = v; bt = t0 + u; }
                }
            }
            bd.end_block(last, t0, m, lane);
        }
        if (!kLocal && last && lane == ln) {
            ReadState* rs = a.state + rd;
            if (kSemi) {
                rs->sink_val[k] = best;
                rs->path_end_row[k] = m > 0 ? a.prow[pbeg + bt] : 0;
            } else {
                rs->sink_val[k] = pick_col(H, qn);
            }
        }
    }
    if (kLocal) {
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) {
            const int v = __shfl_xor(best, d, WAVE), t = __shfl_xor(bt, d, WAVE);
            if (v > best || (v == best && t < bt)) { best = v; bt = t; }
        }
        if (lane == 0) {
            ReadState* rs = a.state + rd;
            rs->sink_val[k] = best;
            rs->path_end_row[k] = m > 0 ? a.prow[pbeg + bt] : 0;
        }
    }
    if (lane == 0) {
        const unsigned long long c = (unsigned long long)m * (unsigned long long)n;
        atomicAdd(a.cells, c);
        atomicAdd(a.cells + 1, c);
    }
}

template <int kKind>
__global__ __launch_bounds__(64) void k_gap_dirs_long(GapLongArgs la) {
    constexpr bool kLocal = kKind == GAP_LOCAL;
    __shared__ int sct[40];
    const GapArgs& a = la.g;
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    if (rs->status & ST_NO_RECORD) return;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    const int k = __builtin_amdgcn_readfirstlane(rs->fwd_path);
    const int score = __builtin_amdgcn_readfirstlane(rs->trace_score);
    const int pbeg = a.poff[k];
    int m = a.poff[k + 1] - pbeg;
    if (kKind != GAP_GLOBAL) m = row_index(a.prow + pbeg, m, rs->end_row) + 1;      // the rows up to the end row are all the walk can visit
    m = __builtin_amdgcn_readfirstlane(min(m, la.rows1 - 1));
    if (n + 1 > la.S * STRIPE || (kLocal && m <= 0)) {
        if (lane == 0) rs->status = ST_WOULD_PANIC;
        return;
    }
    load_scores(a, lane, sct);
    const int S = (n + STRIPE) / STRIPE;
    Boundary bd;
    bd.h = la.dbnd + 2ll * rd * la.rows1;
    bd.z = bd.h + la.rows1;
    uint32_t* out = a.dirs + (long long)rd * a.dirs_stride;
    DirWords<CL> dw;
    int end_col = 0;                                 // local: the smallest global column of the end row that holds the score (0: none yet)
    for (int s = 0; s < S; ++s) {
        const int c0 = s * STRIPE;
        const bool first = s == 0, last = s == S - 1;
        int H[CL], Y[CL];
        ReadCols<CL, true> rc;
        rc.load(a.reads + ro - 1, n, lane, c0);
        row0<CL, kKind>(H, Y, a.o, a.e, c0, lane);
        const int ej0 = a.e * (c0 + lane * CL);
        bd.begin_stripe(first, kLocal ? 0 : a.o + a.e * (c0 - 1));      // H[0][c0 - 1]
        uint32_t* sout = out + (long long)s * la.rows1 * (WL * WAVE);
        int c = CL;
        for (int t0 = 0; t0 < m; t0 += WAVE) {
            int myb = 4;
            if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
            bd.begin_block(first, t0, m, lane);
            const int cnt = min(WAVE, m - t0);
            for (int u = 0; u < cnt; ++u) {
                const int b = __builtin_amdgcn_readlane(myb, u);
                const int incl = gap_row<CL, kKind, true>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, first && lane == 0, bd.dnext, bd.zin(u), dw);
                bd.after_row(u, lane, H[CL - 1], incl);
#pragma unroll
                for (int w = 0; w < WL; ++w) sout[((long long)(t0 + u + 1) * WL + w) * WAVE + lane] = dw.w[w];
                if (kLocal && t0 + u == m - 1) c = own_end_col(H, score, c);      // H is the end row
            }
            bd.end_block(last, t0, m, lane);
        }
        // stripes in ascending order: the first one that holds the score decides
        if (kLocal && end_col == 0) end_col = wave_end_col<CL>(c, c0);
    }
    if (lane == 0) {
        if (kLocal) {
            if (end_col < 1 || end_col > n) rs->status = ST_WOULD_PANIC;          // the score pass and this one disagree: never a guess
            else rs->rec_col = end_col;
        }
        if (m > 0) atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)n);
    }
}

// The walks of k_gap_trace and k_gap_trace_local over striped direction words (gap_trace_wave with S stripes)
__global__ __launch_bounds__(64) void k_gap_trace_long(GapLongArgs la, int semi) { gap_trace_wave<false>(la.g, semi, CL, la.S, la.rows1); }

__global__ __launch_bounds__(64) void k_gap_trace_local_long(GapLongArgs la) { gap_trace_wave<true>(la.g, 0, CL, la.S, la.rows1); }

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static bool geometry_ok(const GapLongArgs& a) { return a.S >= 1 && a.S <= GAP_LONG_MAX_STRIPES && a.rows1 >= 1 && a.bnd && a.dbnd && a.g.dirs; }

const char* launch_gap_score_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s, int max_stripes) {
    // (-m 56 / -m 57 / -m 62 run this pass on up to 64 stripes, without the buffers of the direction pass: the kernel itself has no cap)
    if (max_stripes == GAP_LONG_MAX_STRIPES ? !geometry_ok(a) : !(a.S >= 1 && a.S <= max_stripes && a.rows1 >= 1 && a.bnd)) return nullptr;
    const dim3 grid(a.g.P, nreads);
    RG_GAP_SWITCH_KIND(k_gap_score_long, grid, a);
    return nullptr;
}
const char* launch_gap_dirs_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s) {
    if (!geometry_ok(a)) return nullptr;
    const dim3 grid(nreads);
    RG_GAP_SWITCH_KIND(k_gap_dirs_long, grid, a);
    return nullptr;
}
const char* launch_gap_trace_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s) {
    if (!geometry_ok(a)) return nullptr;
    if (kind == GAP_LOCAL) RG_LAUNCH0(k_gap_trace_local_long, dim3(nreads), dim3(WAVE), 0, s, a);
    if (kind != GAP_GLOBAL && kind != GAP_SEMI) return nullptr;
    RG_LAUNCH0(k_gap_trace_long, dim3(nreads), dim3(WAVE), 0, s, a, kind == GAP_SEMI ? 1 : 0);
}

}  // namespace rg
