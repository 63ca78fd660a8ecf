// Affine-gap pathwise alignment of long reads for gfx950 (-m 16 global, -m 17 semiglobal, -m 22 local): the rules of -m 6, -m 7 and
// -m 12 (RG_MODE_PATHWISE_GAP and RG_MODE_PATHWISE_GAP_LOCAL in include/recgraph_hip.h) for reads of up to 16383 bases.
//
//   k_gap_score_long<kind>    one wave per (read, path) -> ReadState::sink_val / path_end_row, as k_gap_score / k_gap_score_local
//   k_gap_pick, k_gap_pick_local   the kernels of gap/ and gap_local/, launched with the striped width
//   k_gap_dirs_long<kind>     one wave per read: the same row step for the picked path, 4 bits per cell to HBM
//   k_gap_trace_long, k_gap_trace_local_long   one wave per read walks those bits
//
// COLUMN STRIPES, ONE WAVE.  A read of n bases has ceil((n + 1) / 2048) stripes of 2048 columns; inside a stripe lane t owns the 32
// columns s * 2048 + t * 32 .. + 31, and the row step is the one of gap/rg_path_gap.hip (gap_local/ for the local kind): H and Y of
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

#include "../gap/rg_path_gap_common.hpp"      // GNEG, gap_words, ReadCols, DirWords, NoDirs, row_index

constexpr int CL = GAP_LONG_C;
constexpr int STRIPE = GAP_LONG_STRIPE;
constexpr int WL = gap_words(CL);

// the base codes of the lane's columns of the stripe that starts at global column c0 (4 = N for column 0 and the columns past the read)
template <bool kPack>
__device__ __forceinline__ void load_cols(ReadCols<CL, kPack>& rc, const uint8_t* read /* read[1..n] */, int n, int c0, int lane) {
#pragma unroll
    for (int i = 0; i < (kPack ? CL / 4 : CL); ++i) rc.v[i] = 0;
#pragma unroll
    for (int q = 0; q < CL; ++q) {
        const int j = c0 + lane * CL + q;
        const int code = (j >= 1 && j <= n) ? (int)read[j] : 4;
        if (kPack) rc.v[q / 4] |= code << (8 * (q % 4));
        else rc.v[q] = code;
    }
}

__device__ __forceinline__ void load_scores(const GapArgs& a, int lane, int* sct) {
    if (lane < 40) { const int b = lane >> 3, c = lane & 7; sct[lane] = c < 5 ? a.sc.t[b * 6 + c] : 0; }
    __syncthreads();
}

// row 0 of a stripe: H = X = o + e j (0 at column 0; 0 everywhere in the local kind), Y = NEG
template <int kKind>
__device__ __forceinline__ void row0(int (&H)[CL], int (&Y)[CL], int o, int e, int c0, int lane) {
#pragma unroll
    for (int q = 0; q < CL; ++q) {
        const int j = c0 + lane * CL + q;
        H[q] = (kKind == GAP_LONG_LOCAL || j == 0) ? 0 : o + e * j;
        Y[q] = GNEG;
    }
}

// One path row with base b in one stripe.  din: H[i-1][c0-1] (lane 0's diagonal; NEG in stripe 0), zin: the row's z maximum over the
// stripes to the left (NEG in stripe 0), col0: this lane's first column is column 0 of the read (stripe 0, lane 0).  Returns the
// inclusive z maximum up to and including this lane, zin included: lane 63 holds what the next stripe needs.
// Dirs = DirWords<32>: the nibbles of gap/rg_path_gap.hip (the local kind: those of gap_local/, source code 0 = "H == 0: stop"),
// computed on sign bits as k_gap_dirs_local does (every difference lies inside +-2^31).
template <int kKind, class Dirs, class Cols>
__device__ __forceinline__ int long_row(int (&H)[CL], int (&Y)[CL], const Cols& rc, const int* sct, int b, int o, int e, int ej0, bool lane0,
                                        bool col0, int din, int zin, Dirs& dw) {
    constexpr bool kDirs = !std::is_same_v<Dirs, NoDirs>;
    constexpr bool kLocal = kKind == GAP_LONG_LOCAL;
    const int* srow = sct + b * 8;
    const int oe = o + e;
    int diag = dpp_shr1(H[CL - 1], GNEG);
    diag = lane0 ? din : diag;
    unsigned dm = 0, ym = 0;
    int acc = GNEG;                                // max_q (H'_q + e (C - 1 - q)): the lane's z maximum, taken at its last column
#pragma unroll
    for (int q = 0; q < CL; ++q) {
        const int hold = H[q], yold = Y[q];
        int y = max(hold + oe, yold + e);
        const int d = diag + srow[rc.get(q)];
        int hp = max(d, y);
        if (kLocal) hp = max(hp, 0);
        if (kKind != GAP_LONG_GLOBAL && q == 0) {   // -m 17 / -m 22: H[i][0] = 0, Y[i][0] = NEG (-m 16: the recurrence itself gives o + e i)
            hp = col0 ? 0 : hp;
            y = col0 ? GNEG : y;
        }
        if constexpr (kDirs) {
            dm |= ((unsigned)(y - d - 1) >> 31) << q;                     // d >= y
            ym |= ((unsigned)(yold - (hold + o) - 1) >> 31) << q;         // hold + o >= yold
        }
        diag = hold;
        Y[q] = y;
        H[q] = hp;
        acc = max(acc + e, hp);
    }
    if constexpr (kDirs) asm volatile("" : "+v"(dm), "+v"(ym));      // (the masks stay where they are computed: sunk to their use, d, y, hold, yold of every column stay live)
    const int incl = max(dpp_incl_max(acc - (ej0 + e * (CL - 1)), GNEG), zin);
    const int zl = max(dpp_shr1(incl, GNEG), zin);
    int x = zl + o + ej0;
    if constexpr (kDirs) {
#pragma unroll
        for (int w = 0; w < WL; ++w) dw.w[w] = 0;
    }
#pragma unroll
    for (int q = 0; q < CL; ++q) {
        const int hp = H[q];
        const int h = max(hp, x);
        if constexpr (kDirs) {
            const unsigned t = (unsigned)(x - hp - 1) >> 31;                  // hp >= x
            unsigned src = 3u - t - (t & (dm >> q));                          // L 3; else D 1 if d >= y, U 2 otherwise
            if (kLocal) src &= (unsigned)(-h >> 31);                          // 0 where h == 0 (h >= 0)
            const unsigned nib = src | (((ym >> q) & 1u) << 2) | (((unsigned)(x - (h + o) - 1) >> 31) << 3);     // h + o >= x
            dw.w[q / 8] |= nib << (4 * (q % 8));
        }
        H[q] = h;
        x = max(x, hp + o) + e;
    }
    return incl;
}

// value of column qn (wave-uniform) of the lane's chunk (as pick_col of gap/rg_path_gap.hip: a maximum over selects)
__device__ __forceinline__ int pick_col(const int (&H)[CL], int qn) {
    int v = INT32_MIN;
#pragma unroll
    for (int q = 0; q < CL; ++q) v = max(v, q == qn ? H[q] : INT32_MIN);
    return v;
}

// What a stripe takes from and leaves to the boundary buffer, around the rows of one 64-row block (see the file comment).
struct Boundary {
    int* h; int* z;               // [rows]: H of the last column of the stripe before | the z maximum of the stripes before
    int oldh, oldz, newh, newz;   // lane u: row t0 + u
    int dnext;                    // wave-uniform: the diagonal of the next row's first column
    // (no branch on first / last inside a row: in stripe 0 the old values ARE the sentinel, and collecting costs two selects)
    __device__ __forceinline__ void begin_stripe(bool first, int row0_left) { dnext = first ? GNEG : row0_left; }
    __device__ __forceinline__ void begin_block(bool first, int t0, int m, int lane) {
        oldh = GNEG; oldz = GNEG; newh = 0; newz = 0;
        if (!first && t0 + lane < m) { oldh = h[t0 + lane]; oldz = z[t0 + lane]; }
    }
    __device__ __forceinline__ int zin(int u) const { return __builtin_amdgcn_readlane(oldz, u); }
    __device__ __forceinline__ void after_row(int u, int lane, int hlast, int incl) {
        dnext = __builtin_amdgcn_readlane(oldh, u);
        const int hv = __builtin_amdgcn_readlane(hlast, WAVE - 1), zv = __builtin_amdgcn_readlane(incl, WAVE - 1);
        newh = lane == u ? hv : newh;
        newz = lane == u ? zv : newz;
    }
    __device__ __forceinline__ void end_block(bool last, int t0, int m, int lane) {
        if (!last && t0 + lane < m) { h[t0 + lane] = newh; z[t0 + lane] = newz; }
    }
};

}  // namespace

template <int kKind>
__global__ __launch_bounds__(64) void k_gap_score_long(GapLongArgs la) {
    constexpr bool kSemi = kKind == GAP_LONG_SEMI, kLocal = kKind == GAP_LONG_LOCAL;
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
        load_cols<false>(rc, a.reads + ro - 1, n, c0, lane);
        row0<kKind>(H, Y, a.o, a.e, c0, lane);
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
                const int incl = long_row<kKind>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, first && lane == 0, bd.dnext, bd.zin(u), nd);
                bd.after_row(u, lane, H[CL - 1], incl);
                if (kSemi) {
                    const int v = pick_col(H, qn);
                    if (last && v > best) { best = v; bt = t0 + u; }      // strictly better: the first row that attains the maximum
                }
                if (kLocal) {
                    int v = 0;
#pragma unroll
                    for (int q = 0; q < CL; ++q) v = max(v, q <= qlim ? H[q] : 0);
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
    constexpr bool kLocal = kKind == GAP_LONG_LOCAL;
    __shared__ int sct[40];
    const GapArgs& a = la.g;
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    if (rs->status & (ST_BAD_BASE | ST_WOULD_PANIC | ST_UNALIGNED)) return;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    const int k = __builtin_amdgcn_readfirstlane(rs->fwd_path);
    const int score = __builtin_amdgcn_readfirstlane(rs->trace_score);
    const int pbeg = a.poff[k];
    int m = a.poff[k + 1] - pbeg;
    if (kKind != GAP_LONG_GLOBAL) m = row_index(a.prow + pbeg, m, rs->end_row) + 1;      // the rows up to the end row are all the walk can visit
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
        load_cols<true>(rc, a.reads + ro - 1, n, c0, lane);
        row0<kKind>(H, Y, a.o, a.e, c0, lane);
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
                const int incl = long_row<kKind>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, first && lane == 0, bd.dnext, bd.zin(u), dw);
                bd.after_row(u, lane, H[CL - 1], incl);
#pragma unroll
                for (int w = 0; w < WL; ++w) sout[((long long)(t0 + u + 1) * WL + w) * WAVE + lane] = dw.w[w];
                if (kLocal && t0 + u == m - 1) {
                    // H is the end row (inside the loop, as in k_gap_dirs_local: H live out of it costs registers)
#pragma unroll
                    for (int q = CL - 1; q >= 0; --q) c = H[q] == score ? q : c;
                }
            }
            bd.end_block(last, t0, m, lane);
        }
        if (kLocal && end_col == 0) {
            // stripes in ascending order: the first one that holds the score decides (lowest lane, then lowest column of that lane)
            const unsigned long long hit = __ballot(c < CL);
            if (hit) {
                const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)hit) - 1);
                end_col = c0 + l * CL + __builtin_amdgcn_readlane(c, l);
            }
        }
    }
    if (lane == 0) {
        if (kLocal) {
            if (end_col < 1 || end_col > n) rs->status = ST_WOULD_PANIC;          // the score pass and this one disagree: never a guess
            else rs->rec_col = end_col;
        }
        if (m > 0) atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)n);
    }
}

namespace {

// the direction nibble of cell (i, j) of the picked path; the row's words of one stripe are cached per (row, stripe) in `have`
__device__ __forceinline__ uint32_t dir_cell(const uint32_t* dirs, int rows1, int lane, int i, int j, int& have, uint32_t (&wd)[WL]) {
    const int s = j / STRIPE, jl = j % STRIPE;
    const int key = s * rows1 + i;                 // (below 8 * rows1)
    if (have != key) {
#pragma unroll
        for (int w = 0; w < WL; ++w) wd[w] = dirs[((long long)key * WL + w) * WAVE + lane];
        have = key;
    }
    const int q = jl % CL, wsel = q >> 3;
    const uint32_t word = wsel == 0 ? wd[0] : wsel == 1 ? wd[1] : wsel == 2 ? wd[2] : wd[3];
    return ((uint32_t)__builtin_amdgcn_readlane((int)word, __builtin_amdgcn_readfirstlane(jl / CL)) >> (4 * (q & 7))) & 15u;
}

}  // namespace

// The walk of -m 6 / -m 7 (k_gap_trace) over striped direction words.  Every value that steers it comes out of a readlane, so the
// state is the same in all lanes; lane 0 writes.  The loop is bounded: a wrong direction word ends as ST_WOULD_PANIC, never as a hang.
__global__ __launch_bounds__(64) void k_gap_trace_long(GapLongArgs la, int semi) {
    const GapArgs& a = la.g;
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    DevRecord* rec = a.rec + rd;
    auto no_record = [&](uint32_t st) {
        if (lane == 0) { rec->status = st; rec->n_ops = 0; rec->n_fwd_ops = 0; rec->score = 0; }
    };
    if (rs->status & (ST_BAD_BASE | ST_WOULD_PANIC)) { no_record(rs->status); return; }
    const int n = (int)(a.read_off[rd + 1] - a.read_off[rd]);
    const int k = rs->fwd_path;
    const int pbeg = a.poff[k], m = a.poff[k + 1] - pbeg;
    const int idx = row_index(a.prow + pbeg, m, rs->end_row);
    if (idx < 0 || idx + 1 >= la.rows1 || n + 1 > la.S * STRIPE) { no_record(ST_WOULD_PANIC); return; }
    const uint32_t* dirs = a.dirs + (long long)rd * a.dirs_stride;
    uint32_t wd[WL] = {0, 0, 0, 0};
    int have = -1;
    uint8_t* ops = a.ops + (long long)rd * a.ops_stride;
    enum { S_H, S_Y, S_X, S_XARRIVE };
    int i = idx + 1, j = n, state = S_H, nops = 0, steps = 0;
    const int cap = 3 * (m + n) + 3;                // (the count of k_gap_trace_local: at most 2 iterations per row, 3 per column)
    auto emit = [&](uint8_t op) { if (lane == 0 && nops < a.ops_stride) ops[nops] = op; ++nops; };
    while (i > 0 && j > 0 && steps < cap) {
        ++steps;
        const uint32_t cell = dir_cell(dirs, la.rows1, lane, i, j, have, wd);
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
    if (i > 0 && j > 0) { no_record(ST_WOULD_PANIC); return; }
    // the borders: only one state is finite there
    while (j > 0) { emit(OP_L); j -= 1; }
    while (!semi && i > 0) { emit(OP_U); i -= 1; }
    if (nops > a.ops_stride) { no_record(ST_WOULD_PANIC); return; }
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

// The walk of -m 12 (k_gap_trace_local) over striped direction words: from (end row, end column) until a cell with H == 0.
__global__ __launch_bounds__(64) void k_gap_trace_local_long(GapLongArgs la) {
    const GapArgs& a = la.g;
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
    if (idx < 0 || idx + 1 >= la.rows1 || n + 1 > la.S * STRIPE || end_col < 1 || end_col > n) { no_record(ST_WOULD_PANIC); return; }
    const uint32_t* dirs = a.dirs + (long long)rd * a.dirs_stride;
    uint32_t wd[WL] = {0, 0, 0, 0};
    int have = -1;
    uint8_t* ops = a.ops + (long long)rd * a.ops_stride;
    enum { S_H, S_Y, S_X, S_XARRIVE };
    int i = idx + 1, j = end_col, state = S_H, nops = 0, steps = 0;
    const int cap = 3 * (m + n) + 3;                // (counted at k_gap_trace_local)
    bool stopped = false;
    auto emit = [&](uint8_t op) { if (lane == 0 && nops < a.ops_stride) ops[nops] = op; ++nops; };
    while (i > 0 && j > 0 && steps < cap) {
        ++steps;
        const uint32_t cell = dir_cell(dirs, la.rows1, lane, i, j, have, wd);
        if (state == S_XARRIVE) {
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
#define RG_GAP_LONG_DISPATCH(K, grid)                                                       \
    switch (kind) {                                                                         \
        case GAP_LONG_GLOBAL: RG_LAUNCH(K, (0), grid, dim3(WAVE), 0, s, a);                 \
        case GAP_LONG_SEMI: RG_LAUNCH(K, (1), grid, dim3(WAVE), 0, s, a);                   \
        case GAP_LONG_LOCAL: RG_LAUNCH(K, (2), grid, dim3(WAVE), 0, s, a);                  \
        default: return nullptr;                                                            \
    }

static bool geometry_ok(const GapLongArgs& a) { return a.S >= 1 && a.S <= GAP_LONG_MAX_STRIPES && a.rows1 >= 1 && a.bnd && a.dbnd && a.g.dirs; }

const char* launch_gap_score_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s) {
    if (!geometry_ok(a)) return nullptr;
    const dim3 grid(a.g.P, nreads);
    RG_GAP_LONG_DISPATCH(k_gap_score_long, grid)
    return nullptr;
}
const char* launch_gap_dirs_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s) {
    if (!geometry_ok(a)) return nullptr;
    const dim3 grid(nreads);
    RG_GAP_LONG_DISPATCH(k_gap_dirs_long, grid)
    return nullptr;
}
const char* launch_gap_trace_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s) {
    if (!geometry_ok(a)) return nullptr;
    if (kind == GAP_LONG_LOCAL) RG_LAUNCH0(k_gap_trace_local_long, dim3(nreads), dim3(WAVE), 0, s, a);
    if (kind != GAP_LONG_GLOBAL && kind != GAP_LONG_SEMI) return nullptr;
    RG_LAUNCH0(k_gap_trace_long, dim3(nreads), dim3(WAVE), 0, s, a, kind == GAP_LONG_SEMI ? 1 : 0);
}

}  // namespace rg
