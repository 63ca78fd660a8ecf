// Launchers of the striped bit-vector edit-distance pathwise kernels (-m 94 / -m 95, edit_xlong/rg_path_edit_xlong.hip) and their
// argument block: the block of -m 44 / -m 45 (GapArgs; o and e are not read) plus the stripe count, the boundary slots and the walk
// state.  The pick between the score pass and the traceback is the affine-gap family's launch_gap_pick.  The driver
// (rg_path_driver.hip: enqueue_pathwise_edit_xlong) reaches the kernels through these host functions only.
#pragma once
#include "../gap/rg_path_gap.hpp"
#include "../rg_edit_modes.hpp"

namespace rg {

// where the walk of a read stands between two rounds (written by k_edit_walk_xlong: its first round starts every walk)
struct EditWalkState {
    int i, j;                     // the cell the walk looks at next: row index + 1 of the picked path, read column
    int nops, steps;              // ops written so far | iterations so far, counted against rows + n + 2 over all rounds
    int done;                     // the record is written
    int pad[3];
};

struct EditXLongArgs {
    GapArgs g;                    // g.dirs: [reads][dirs_stride], ONE stripe in the layout of k_edit_dirs<8>: row t of the picked path at
                                  // ((t + 1) * 16 + w) * 64 + lane, w < 8: D0, 8 <= w < 16: Ph
    int S;                        // stripes of the batch's longest read (2 .. 8); a read of n bases has ceil(n / 16384) of them
    int rows1;                    // rows of the longest path + 1
    unsigned long long* bnd;      // [reads][P][S - 1][slot_words]: slot s of a (read, path) holds what stripe s + 1 takes from its left: per
                                  // block of 64 rows two masks, [2 blk] bit u: row 64 blk + u's last column of stripe s went up by one from
                                  // the row above, [2 blk + 1]: down by one
    long long bnd_stride;         // u64 per read: P * (S - 1) * slot_words
    int slot_words;               // u64 per slot: >= 2 * ceil((rows1 - 1) / 64), a multiple of 16 (no two waves share a 128-byte line)
    EditWalkState* walk;          // [reads]
};

// semi: -m 95; round: the stripe the launch works on, S - 1 down to 0
const char* launch_edit_score_xlong(const EditXLongArgs& a, int nreads, bool semi, hipStream_t s);
const char* launch_edit_redo_xlong(const EditXLongArgs& a, int nreads, bool semi, int round, hipStream_t s);
const char* launch_edit_walk_xlong(const EditXLongArgs& a, int nreads, bool semi, int round, hipStream_t s);

}  // namespace rg
