// Launchers of the both-strands edit-distance pathwise kernels (-m 64 / -m 65, edit_strands/rg_edit_strands.hip).  The argument block is
// the affine-gap family's (GapArgs, gap/rg_path_gap.hpp; o and e are not read); the pick is that family's launch_gap_pick, the direction
// pass and the walk are edit/rg_path_edit.hpp's.  The driver (rg_path_driver.hip: enqueue_pathwise_edit_strands) reaches the kernels
// through these host functions only.
#pragma once
#include "../gap/rg_path_gap.hpp"

namespace rg {

// W: words of 32 columns per lane (1, 2, 4, 8, 16; n <= 1024 W for every read of the launch: a strand takes 32 lanes); semi: -m 65.
// a.state: [nreads] the read as given; state2: [nreads] its reverse complement.  Both counters take 2 * rows * n per (read, path)
const char* launch_edit_score_pair(const GapArgs& a, ReadState* state2, int nreads, int W, bool semi, hipStream_t s);
// one lane per read: the winner's pick in state[i], strand[i] = 1 where that is the reverse complement's
const char* launch_edit_strands_duel(ReadState* state, const ReadState* state2, uint8_t* strand, int nreads, hipStream_t s);

}  // namespace rg
