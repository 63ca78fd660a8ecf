// Launchers of the bit-vector edit-distance pathwise kernels (-m 44 / -m 45, edit/rg_path_edit.hip).  The argument block is the
// affine-gap family's (GapArgs, gap/rg_path_gap.hpp; o and e are not read), and the pick between the two passes is that family's
// launch_gap_pick.  The driver (rg_path_driver.hip: enqueue_pathwise_edit) reaches the kernels through these host functions only.
#pragma once
#include "../gap/rg_path_gap.hpp"

namespace rg {

// W: words of 32 columns per lane (1, 2, 4, 8; n <= 2048 W for every read of the launch); semi: -m 45.  a.dirs: [reads][dirs_stride],
// row t of the picked path at ((t + 1) * 2 W + w) * 64 + lane, w < W: D0, W <= w < 2 W: Ph; dirs_stride a multiple of 2 W * 64
const char* launch_edit_score(const GapArgs& a, int nreads, int W, bool semi, hipStream_t s);
const char* launch_edit_dirs(const GapArgs& a, int nreads, int W, bool semi, hipStream_t s);
const char* launch_edit_trace(const GapArgs& a, int nreads, int W, bool semi, hipStream_t s);

}  // namespace rg
