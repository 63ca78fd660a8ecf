// What is about column stripes in the striped affine-gap pathwise kernels: the stripe geometry and the boundary values a stripe takes
// from and leaves to its neighbours.  Shared by gap_long/rg_path_gap_long.hip (-m 16 / -m 17 / -m 22) and
// gap_xlong/rg_path_gap_xlong.hip (-m 56 / -m 57 / -m 62), which runs the same recurrence one stripe at a time.  The row step itself
// (gap_row, striped form), row 0, the base codes, the nibble lookup and the walk are the family's, in gap/rg_path_gap_common.hpp.
// Included inside namespace rg, in each file's anonymous namespace, after that header and gap_long/rg_path_gap_long.hpp.
#pragma once

constexpr int CL = GAP_LONG_C;
constexpr int STRIPE = GAP_LONG_STRIPE;
constexpr int WL = gap_words(CL);

// What a stripe takes from and leaves to the boundary buffer, around the rows of one 64-row block (COLUMN STRIPES in
// rg_path_gap_long.hip).
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
