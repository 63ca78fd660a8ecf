// Launchers of the long-read affine-gap pathwise kernels (-m 16 / -m 17 / -m 22, gap_long/rg_path_gap_long.hip) and their argument
// block: the block of -m 6 / -m 7 / -m 12 (GapArgs, gap/rg_path_gap.hpp) plus the stripe geometry and the two boundary buffers.  The
// driver (rg_path_driver.hip: enqueue_pathwise_gap) reaches the kernels through these host functions only.
#pragma once
#include "../gap/rg_path_gap.hpp"

namespace rg {

constexpr int GAP_LONG_C = 32;                        // columns per lane
constexpr int GAP_LONG_STRIPE = GAP_LONG_C * WAVE;    // columns per stripe: 2048
// (GAP_LONG_MAX_STRIPES, the most stripes of a read here: rg_gap_modes.hpp, beside the families that use it)

struct GapLongArgs {
    GapArgs g;                    // g.dirs: [reads][dirs_stride], stripe s, row t of the picked path at ((s * rows1 + t + 1) * 4 + w) * 64 + lane
    int S;                        // stripes of the batch's longest read (a read runs ceil((n + 1) / 2048) of them)
    int rows1;                    // rows of the longest path + 1
    int* bnd;                     // score pass, [reads][P][2][rows1]: per path row, H of the stripe's last column | the row's running z maximum
    long long bnd_stride;         // ints per read: P * 2 * rows1
    int* dbnd;                    // direction pass, [reads][2][rows1]: the same two values for the picked path
};

// kind: GapKind (16: global, 17: semi, 22: local); max_stripes: the host-side cap on a.S, lifted by the plan of gap_xlong/ alone
const char* launch_gap_score_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s, int max_stripes = GAP_LONG_MAX_STRIPES);
const char* launch_gap_dirs_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s);
const char* launch_gap_trace_long(const GapLongArgs& a, int nreads, int kind, hipStream_t s);

}  // namespace rg
