// The bit arithmetic of the edit-distance kernels (edit/rg_path_edit.hip), as host and device functions on ONE LANE'S CHUNK of a
// row: W words of 32 bits, word 0 the lowest.  Column j >= 1 of the read is bit t = j - 1 of a 64 * 32 W bit vector; lane t / (32 W)
// owns the chunk, word (t / 32) % W of it, bit t % 32.  No HIP call in here: tests/c/edit_bits_check.cpp runs the very same functions
// over 64 chunks on the host and compares them with a plain wide-integer row step.
//
// THE ROW STEP (Myers 1999, in Hyyro's form with D0) for a path base with match vector Eq, on the vertical state (Pv, Mv) of the row
// above — Pv / Mv bit t: the value of column t + 1 is one more / one less than that of column t:
//     Xv = Eq | Mv
//     Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq                       the one WIDE addition
//     Ph = Mv | ~(Xh | Pv);   Mh = Pv & Xh;   D0 = Xh | Mv      bit t: column t + 1 went up / down by one from the row above; its diagonal is equal
//     Ph <<= 1 (bit 0 |= hin: column 0 went up by one, the global kind);   Mh <<= 1
//     Pv = Mh | ~(Xv | Ph);   Mv = Ph & Xv
// as three pieces with a cross-lane exchange between them:
//     edit_sum      the chunk's addition with carry-in 0: the sum, "it carried out" (g) and "the sum is all ones" (p)
//       -> edit_carry_mask(ballot(g), ballot(p)): the carry into every lane, ONE 64-bit addition
//     edit_deltas   the carry goes in; Ph, Mh (unshifted) and D0 of the chunk
//       -> the top bits of Ph and Mh of the lane to the left
//     edit_finish   the shifts with those bits coming in, and the new (Pv, Mv)
// Bits above the read's last column never influence a bit below them (the addition carries upwards, the shifts move upwards), so
// nothing masks them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RG_EDIT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RG_EDIT_HD inline
#endif
// (the kernels need the loops over the W words unrolled: the words live in registers; a host compiler is told nothing)
#if defined(__clang__)
#define RG_EDIT_UNROLL _Pragma("unroll")
#else
#define RG_EDIT_UNROLL
#endif

namespace rg {

// a + b over the chunk with carry-in 0 -> s; returns the carry out (0 / 1)
template <int W>
RG_EDIT_HD uint32_t edit_chunk_add(const uint32_t (&a)[W], const uint32_t (&b)[W], uint32_t (&s)[W]) {
    uint32_t c = 0;
    RG_EDIT_UNROLL
    for (int k = 0; k < W; ++k) {
        const uint64_t t = (uint64_t)a[k] + b[k] + c;
        s[k] = (uint32_t)t;
        c = (uint32_t)(t >> 32);
    }
    return c;
}

template <int W>
RG_EDIT_HD bool edit_chunk_all_ones(const uint32_t (&s)[W]) {
    uint32_t v = ~0u;
    RG_EDIT_UNROLL
    for (int k = 0; k < W; ++k) v &= s[k];
    return v == ~0u;
}

// s += c (0 / 1) over the chunk; a carry out of the chunk is dropped (the carry mask accounted for it: it happens only where the
// chunk was all ones)
template <int W>
RG_EDIT_HD void edit_chunk_inc(uint32_t (&s)[W], uint32_t c) {
    RG_EDIT_UNROLL
    for (int k = 0; k < W; ++k) {
        const uint64_t t = (uint64_t)s[k] + c;
        s[k] = (uint32_t)t;
        c = (uint32_t)(t >> 32);
    }
}

// x <<= 1 over the chunk, bit 0 from `in` (0 / 1)
template <int W>
RG_EDIT_HD void edit_chunk_shl1(uint32_t (&x)[W], uint32_t in) {
    RG_EDIT_UNROLL
    for (int k = W - 1; k > 0; --k) x[k] = (x[k] << 1) | (x[k - 1] >> 31);
    x[0] = (x[0] << 1) | in;
}

// Bit l: lane l's chunk takes a carry in.  G bit l: lane l's chunk carried out with carry-in 0; P bit l: its sum is all ones (it hands
// a carry on); G & P == 0.  In (G | P) + G a lane with G adds 1 + 1 and always carries on, a lane with P adds 1 + 0 and carries on what
// comes in, the others stop it: the addition's own carry chain IS the chain over the lanes, and its result bit is the carry in, inverted
// where P is set.
RG_EDIT_HD uint64_t edit_carry_mask(uint64_t G, uint64_t P) { return ((G | P) + G) ^ P; }

// (Eq & Pv) + Pv with carry-in 0 -> sum; returns g.  p is edit_chunk_all_ones(sum); the two exclude each other (Eq & Pv is a subset of Pv:
// a sum that carried out is at most 2^(32 W) - 2)
template <int W>
RG_EDIT_HD uint32_t edit_sum(const uint32_t (&eq)[W], const uint32_t (&pv)[W], uint32_t (&sum)[W]) {
    uint32_t a[W];
    RG_EDIT_UNROLL
    for (int k = 0; k < W; ++k) a[k] = eq[k] & pv[k];
    return edit_chunk_add<W>(a, pv, sum);
}

// sum: edit_sum's, the lane's carry `cin` not yet added.  -> Ph, Mh (unshifted) and D0 of the chunk
template <int W>
RG_EDIT_HD void edit_deltas(const uint32_t (&eq)[W], const uint32_t (&pv)[W], const uint32_t (&mv)[W], uint32_t (&sum)[W], uint32_t cin,
                            uint32_t (&ph)[W], uint32_t (&mh)[W], uint32_t (&d0)[W]) {
    edit_chunk_inc<W>(sum, cin);
    RG_EDIT_UNROLL
    for (int k = 0; k < W; ++k) {
        const uint32_t xh = (sum[k] ^ pv[k]) | eq[k];
        ph[k] = mv[k] | ~(xh | pv[k]);
        mh[k] = pv[k] & xh;
        d0[k] = xh | mv[k];
    }
}

// ph, mh: edit_deltas's (changed: shifted in place); pin, nin: the top bits of Ph and Mh of the lane to the left (lane 0: hin and 0)
template <int W>
RG_EDIT_HD void edit_finish(const uint32_t (&eq)[W], uint32_t (&pv)[W], uint32_t (&mv)[W], uint32_t (&ph)[W], uint32_t (&mh)[W], uint32_t pin,
                            uint32_t nin) {
    edit_chunk_shl1<W>(ph, pin);
    edit_chunk_shl1<W>(mh, nin);
    RG_EDIT_UNROLL
    for (int k = 0; k < W; ++k) {
        const uint32_t xv = eq[k] | mv[k];
        pv[k] = mh[k] | ~(xv | ph[k]);
        mv[k] = ph[k] & xv;
    }
}

// ---- THE STRIPED ROW STEP (edit_xlong/rg_path_edit_xlong.hip; tests/c/edit_xlong_bits_check.cpp) ---------------------------------
// A row longer than one vector is cut into stripes of 64 * 32 W bits, each a vector of its own: Myers' block step.  Stripe s > 0
// takes from its left neighbour hin in {-1, 0, +1}: how the stripe's column 0 — the neighbour's last column — changed from the row
// above, i.e. the neighbour's top bit of the UNSHIFTED Ph (+1) / Mh (-1) of this row (edit_hout).  Stripe 0 takes the border: +1 in
// the global kind, 0 in the semiglobal kind.  What hin changes, derived from the cell recurrence with v = value[i-1][c0], the
// stripe's column 0 in the row above (Pv / Mv are differences along the row, so v itself never enters):
//   * hin = -1: value[i][c0] = v - 1, and column c0 + 1 of this row is at most v (one L from there) and at least v (no value lies
//     below its diagonal): it EQUALS its diagonal whatever the bases say.  That is what a match at bit 0 gives, and from bit 0 on
//     the chain "equal to the diagonal, and the row above goes up by one" runs on through the addition exactly as from a match: bit 0
//     of Eq is set FOR THE Xh TERM.  Xv = Eq | Mv keeps the real Eq: whether column c0 + 1 goes DOWN from its left neighbour in the
//     new row follows from Ph / Mh shifted, not from this help bit.
//   * the shift: bit 0 of the shifted Ph / Mh is the vertical change of the column to the LEFT of bit 0, which is column c0: Ph takes
//     (hin > 0), Mh takes (hin < 0).  The unstriped step hard-wires the latter to 0: column 0 of the read never goes down.
//   * the wide addition's carry does not cross a stripe: the carry of a block is the chain above running on past its top bit, and
//     whether it does is exactly what the neighbour's hin = -1 says (a chain that reaches the stripe's last column makes that column
//     equal to its diagonal with the row above going up: the column goes down by one, Mh's top bit).
// Ph, Mh and D0 of edit_deltas keep their meaning bit for bit (D0 bit 0 = 1 for hin = -1 is the equality above), so a walk reads a
// stripe's words as it reads the whole vector's.
RG_EDIT_HD uint32_t edit_hin_eq0(uint32_t eq0, int hin) { return eq0 | (hin < 0 ? 1u : 0u); }
RG_EDIT_HD uint32_t edit_hin_pin(int hin) { return hin > 0 ? 1u : 0u; }
RG_EDIT_HD uint32_t edit_hin_nin(int hin) { return hin < 0 ? 1u : 0u; }
// the hin of the stripe to the right: the top words of the last chunk's UNSHIFTED Ph and Mh (the two bits exclude each other)
RG_EDIT_HD int edit_hout(uint32_t ph_top, uint32_t mh_top) { return (int)(ph_top >> 31) - (int)(mh_top >> 31); }
// the same out of two masks of 64 rows each (bit u: row u of the block went up / down), as the stripes exchange it
RG_EDIT_HD int edit_hin_of_masks(uint64_t up, uint64_t down, int u) { return (int)((up >> u) & 1u) - (int)((down >> u) & 1u); }

}  // namespace rg
