// Packed 16-bit rows (two DP columns per 32-bit register, z-space: rg_sweep16.hip): the primitives, their constants and the two
// LDS tables every packed kernel builds from the score table — stated once for k_sweep16, k_layer16, k_opt0_16 (rg_sweep16.hip) and
// k_layer_win (layer_window/rg_layer_window.hip).  Device code only.
#pragma once
#include "rg_device.hpp"

namespace rg {

constexpr int NEG16 = -30000;                               // "minus infinity" of a 16-bit lane; real values stay > -24000
constexpr int NEGPAIR = (int)(((unsigned)(NEG16 & 0xffff) << 16) | (unsigned)(NEG16 & 0xffff));
constexpr int ONE2 = 0x00010001;

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int pk_add(int a, int b) {
    return __builtin_bit_cast(int, (s16x2)(__builtin_bit_cast(s16x2, a) + __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ int pk_sub(int a, int b) {
    return __builtin_bit_cast(int, (s16x2)(__builtin_bit_cast(s16x2, a) - __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ int pk_max(int a, int b) {
    return __builtin_bit_cast(int, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ int pk_min(int a, int b) {
    return __builtin_bit_cast(int, __builtin_elementwise_min(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ int pk_minu(int a, int b) {
    return __builtin_bit_cast(int, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// saturating packed difference (v_pk_sub_i16 ... clamp): the sign of each half is the sign of the true difference
__device__ __forceinline__ int pk_sub_sat(int a, int b) {
    return __builtin_bit_cast(int, __builtin_elementwise_sub_sat(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ int pk_add_sat(int a, int b) {
    return __builtin_bit_cast(int, __builtin_elementwise_add_sat(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
// per half: 0xffff where the half of `v` is negative, else 0  (v_pk_ashrrev_i16)
__device__ __forceinline__ int pk_sign(int v) {
    return __builtin_bit_cast(int, (s16x2)(__builtin_bit_cast(s16x2, v) >> (s16x2)(15)));
}
__device__ __forceinline__ int pack16(int lo, int hi) { return (int)(((unsigned)hi << 16) | ((unsigned)lo & 0xffffu)); }
__device__ __forceinline__ int lo16(int v) { return (int)(short)(v & 0xffff); }
__device__ __forceinline__ int hi16(int v) { return v >> 16; }
// per half: mask ? a : b   (mask halves are 0 or 0xffff)
__device__ __forceinline__ int bfi(int mask, int a, int b) {
    return __builtin_amdgcn_bitop3_b32(mask, a, b, 0xCA);   // (mask & a) | (~mask & b) in ONE v_bitop3_b32
}

// The move the reference's traceback takes in the two cells of a register, from d, u and l (= the new row's column c - 1) of its own
// layer: per half 1 = D, 2 = U, 3 = L, D if it attains the maximum, else U, else L.
__device__ __forceinline__ unsigned decide16(int d, int u, int nl) {
    const int mx = pk_max(pk_max(d, u), nl);
    const int nd = pk_sign(pk_sub_sat(d, mx));                  // 0xffff where D does not attain the maximum
    const int nu = pk_sign(pk_sub_sat(u, mx));
    const int b0 = __builtin_amdgcn_bitop3_b32(nd, nu, ONE2, 0x8A);           // bit 1 = nd, bit 0 = (~nd | nu) & 1
    return (unsigned)(b0 | (nd & 0x00020002));
}

// s2[5][64]: the packed (s - g) pairs a diagonal step adds in z-space, by row base li and (code_lo | code_hi << 3) of the two read
// bases a register faces.  sct: the score table in LDS ([36], visible to the wave); the caller puts the barrier behind it.
__device__ __forceinline__ void pair_table(int* s2, const int* sct, int gcost, int lane) {
    for (int e = lane; e < 5 * 64; e += WAVE) {
        const int li = e >> 6, cl = e & 7, ch = (e >> 3) & 7;
        s2[e] = (cl < 6 && ch < 6) ? pack16(sct[li * 6 + cl] - gcost, sct[li * 6 + ch] - gcost) : 0;
    }
}

// Score profile of a read: sprof[(li * 64 + lane) * H + r] = the pair of s2 that register r of the lane (columns lane * 2H + r and
// + H of them; read[1 .. n], mirrored when `rev`) adds in a row whose base is li — one 16-byte LDS read per four registers and row
// instead of a code extraction + table lookup per register.  s2 complete (barrier) before, the caller's barrier behind.  Also sets
// `row` to the gap-only start row (z = 0; NEG16 in the columns outside the read): the same loop over the same columns.
template <int H>
__device__ __forceinline__ void stage_profile(int* sprof, const int* s2, const uint8_t* read, int n, int ncols, bool rev, int lane, int (&row)[H]) {
#pragma unroll
    for (int r = 0; r < H; ++r) {
        const int c0 = lane * 2 * H + r, c1 = c0 + H;
        int k0 = 4, k1 = 4;
        if (c0 >= 1 && c0 < ncols) k0 = rev ? read[n - c0 + 1] : read[c0];
        if (c1 >= 1 && c1 < ncols) k1 = rev ? read[n - c1 + 1] : read[c1];
#pragma unroll
        for (int li = 0; li < 5; ++li) sprof[(li * WAVE + lane) * H + r] = s2[li * 64 + (k0 | (k1 << 3))];
        row[r] = pack16(c0 < ncols ? 0 : NEG16, c1 < ncols ? 0 : NEG16);
    }
}

}  // namespace rg
