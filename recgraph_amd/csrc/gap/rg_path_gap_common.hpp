// What the kernel files of the affine-gap pathwise family share besides the row step itself (gap/rg_path_gap.hip: -m 6 / -m 7;
// gap_local/rg_path_gap_local.hip: -m 12, whose row step is a specialised copy): the sentinel, the geometry of the direction words,
// the read's base codes per lane, the row lookup of the walkers.  Everything here is inlined into its callers; included inside
// namespace rg, in each file's anonymous namespace.
#pragma once

constexpr int GNEG = -(1 << 29);
constexpr int gap_words(int C) { return C >= 8 ? C / 8 : 1; }

// The base codes of the lane's columns (4 = N for the columns past the read).  kPack: four codes per dword — the direction pass,
// whose masks and packed words compete with the three C-wide arrays for registers, pays one v_bfe per cell for 3 C / 4 registers
template <int C, bool kPack>
struct ReadCols {
    int v[kPack ? C / 4 : C];
    __device__ __forceinline__ void load(const uint8_t* read /* read[1..n] */, int n, int lane) {
#pragma unroll
        for (int i = 0; i < (kPack ? C / 4 : C); ++i) v[i] = 0;
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const int j = lane * C + q;
            const int code = (j >= 1 && j <= n) ? (int)read[j] : 4;
            if (kPack) v[q / 4] |= code << (8 * (q % 4));
            else v[q] = code;
        }
    }
    __device__ __forceinline__ int get(int q) const { return kPack ? (v[kPack ? q / 4 : 0] >> (8 * (q % 4))) & 0xff : v[kPack ? 0 : q]; }
};

// the direction words of one row (k_gap_dirs) / nothing (k_gap_score: the row step then has no direction code at all)
template <int C>
struct DirWords { uint32_t w[gap_words(C)]; };
struct NoDirs {};

// index of `row` among the ascending rows of a path (-1: not there)
__device__ __forceinline__ int row_index(const int* rows, int m, int row) {
    int lo = 0, hi = m - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, r = rows[mid];
        if (r == row) return mid;
        if (r < row) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}
