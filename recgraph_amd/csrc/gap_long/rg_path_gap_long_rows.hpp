// The row step of the striped affine-gap pathwise kernels and what goes with it: the stripe geometry, the base codes and row 0 of a
// stripe, the boundary values a stripe takes from and leaves to its neighbours, the column pick and the direction-nibble lookup of
// the walkers.  Shared by gap_long/rg_path_gap_long.hip (-m 16 / -m 17 / -m 22) and gap_xlong/rg_path_gap_xlong.hip (-m 56 / -m 57 /
// -m 62), which runs the same recurrence one stripe at a time.  Everything here is inlined into its callers; included inside namespace
// rg, in each file's anonymous namespace, after gap/rg_path_gap_common.hpp and gap_long/rg_path_gap_long.hpp.
#pragma once

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
