// The two cross-lane pieces of the HALF-WAVE row step (edit_strands/rg_edit_strands.hip: k_edit_score_pair), as host and device functions.
// The wave holds TWO independent bit vectors of 32 * 32 W bits each: the read as given in lanes 0 .. 31, its reverse complement in
// lanes 32 .. 63; within a half the layout is edit/rg_edit_bits.hpp's (bit t: lane-of-half t / (32 W), word (t / 32) % W).  The pieces
// on one lane's chunk — edit_sum, edit_deltas, edit_finish — are that file's, unchanged.  What differs is what crosses the lanes:
//   * the carries of the wide addition are TWO chains of 32 lanes: a carry out of lane 31 never reaches lane 32;
//   * the bits shifted into lane 32 are the border's, as lane 0's: hin (1 global, 0 semiglobal) into Ph, 0 into Mh — not lane 31's
//     top bits.
// No HIP call in here: tests/c/edit_pair_bits_check.cpp runs these over 64 host lanes against two independent wide-integer row steps.
#pragma once
#include "../edit/rg_edit_bits.hpp"

namespace rg {

constexpr int EDIT_PAIR_HALF = 32;      // lanes per strand

// Bit l: lane l's chunk takes a carry in.  G, P: the two ballots of edit_carry_mask.  Each half is the 32-bit addition of that
// function on its own: the carry out of bit 31 of the low half is dropped with the sum's bit 32, and the high half starts with none
RG_EDIT_HD uint64_t edit_pair_carry_mask(uint64_t G, uint64_t P) {
    const uint32_t gl = (uint32_t)G, pl = (uint32_t)P, gh = (uint32_t)(G >> 32), ph = (uint32_t)(P >> 32);
    const uint32_t lo = ((gl | pl) + gl) ^ pl, hi = ((gh | ph) + gh) ^ ph;
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// What a lane shifts into bit 0 of Ph or Mh: `from_left`, the top bit of the lane to its left (whatever the caller got for lane 0), or
// `border` in the first lane of either half
RG_EDIT_HD uint32_t edit_pair_shift_in(uint32_t from_left, int lane, uint32_t border) { return (lane & (EDIT_PAIR_HALF - 1)) == 0 ? border : from_left; }

}  // namespace rg
