// Launchers of the one-stripe-at-a-time traceback of the affine-gap pathwise family (-m 56 / -m 57 / -m 62,
// gap_xlong/rg_path_gap_xlong.hip) and their argument block: the block of -m 16 / -m 17 / -m 22 (GapLongArgs) plus the checkpoints and
// the walk state.  The score pass and the pick kernels of such a batch are those of gap_long/, gap/ and gap_local/.  The driver
// (rg_path_driver.hip: enqueue_pathwise_gap) reaches the kernels through these host functions only.
#pragma once
#include "../gap_long/rg_path_gap_long.hpp"

namespace rg {

// (GAP_XLONG_MAX_STRIPES: rg_gap_modes.hpp)

// where the walk of a read stands between two rounds (written by k_gap_ckpt_long, then by the walk kernels)
struct GapWalkState {
    int i, j;                     // the cell the walk looks at next: row index + 1 of the picked path, read column
    int state;                    // H, Y, X, X-arrive (the enum of the walk kernels)
    int nops, steps;              // ops written so far | iterations so far, counted against 3 (rows + n) + 3 over all rounds
    int done;                     // the record is written
    int pad[2];
};

struct GapXLongArgs {
    GapLongArgs l;                // l.g.dirs: [reads][dirs_stride], ONE stripe: row t of the picked path at ((t + 1) * 4 + w) * 64 + lane;
                                  // l.S: stripes of the batch's longest read (2 .. 64); l.dbnd is not used
    int* ckpt;                    // [reads][S - 1][2][rows1]: slot s holds what stripe s + 1 takes from its left, per row of the picked
                                  // path: H of stripe s's last column | the row's z maximum over stripes 0 .. s
    long long ckpt_stride;        // ints per read: (S - 1) * 2 * rows1
    GapWalkState* walk;           // [reads]
};

// kind: GapKind (56: global, 57: semi, 62: local); round: the stripe the launch works on, l.S - 1 down to 0
const char* launch_gap_ckpt_long(const GapXLongArgs& a, int nreads, int kind, hipStream_t s);
const char* launch_gap_redo_long(const GapXLongArgs& a, int nreads, int kind, int round, hipStream_t s);
const char* launch_gap_walk_long(const GapXLongArgs& a, int nreads, int kind, int round, hipStream_t s);

}  // namespace rg
