// Launchers of the local affine-gap pathwise kernels (-m 12, gap_local/rg_path_gap_local.hip).  They take the argument block of
// -m 6 / -m 7 (GapArgs, gap/rg_path_gap.hpp); the driver (rg_path_driver.hip: enqueue_pathwise_gap) reaches the kernels through
// these host functions only.
#pragma once
#include "../gap/rg_path_gap.hpp"

namespace rg {

// C: columns per lane (4, 8, 16, 32; n + 1 <= 64 C for every read of the launch)
const char* launch_gap_score_local(const GapArgs& a, int nreads, int C, hipStream_t s);
const char* launch_gap_pick_local(const GapArgs& a, int nreads, int C, hipStream_t s);
const char* launch_gap_dirs_local(const GapArgs& a, int nreads, int C, hipStream_t s);
const char* launch_gap_trace_local(const GapArgs& a, int nreads, int C, hipStream_t s);

}  // namespace rg
