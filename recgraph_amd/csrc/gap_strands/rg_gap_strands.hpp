// The gate of the local both-strands mode (-m 32, RG_MODE_PATHWISE_GAP_LOCAL_STRANDS in include/recgraph_hip.h;
// gap_strands/rg_gap_strands.hip).  Modes 26 and 27 join their two passes with the kernels of rg_strand.hip as they are; mode 32
// needs another qualifying test, since a local score is never negative.  The argument block is k_strand_gate's (rg_strand.hpp);
// `recomb` and `first_rev` are not read (a local record prints its integer score, and the mode has no vote).
#pragma once
#include "../rg_strand.hpp"

namespace rg {

const char* launch_gap_strands_gate(const StrandGateArgs& a, hipStream_t s);

}  // namespace rg
