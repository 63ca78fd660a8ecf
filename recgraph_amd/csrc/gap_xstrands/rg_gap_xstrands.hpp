// The four small kernels of the both-strands affine-gap pathwise modes for reads of up to 131071 bases (-m 76 / -m 77 / -m 82,
// RG_MODE_PATHWISE_GAP_XSTRANDS in include/recgraph_hip.h; gap_xstrands/rg_gap_xstrands.hip).  Those modes decide the strand on the
// PICKS of the two strands and run the traceback once, so a pick has to leave the pipeline and come back into it:
//
//   k_gap_pick_out         end of a PICK stage (rg_path_driver.hip): ReadState of a chunk -> the job's records
//   k_gap_xstrands_duel    between the stages (rg_strand_driver.hip): k_strand_merge's decision on two picks, no op copy
//   k_gap_seed_pick        start of a TRACE stage: the job's records -> ReadState of a chunk
//   k_gap_xstrands_mark    behind the TRACE stage: the strand flag of every record (the walk's record writer clears it)
//
// A pick in a DevRecord: status, score, best_path (= rev_path), end_row; every other field 0.  That is all the direction pass and
// the walk read of what the score pass and the pick leave in ReadState (status, trace_score, fwd_path, end_row: the local kinds
// find their end column themselves).
#pragma once
#include "../rg_path_plan.hpp"
#include "../rg_strand.hpp"

namespace rg {

struct GapXStrandsDuelArgs {
    DevRecord* rec;            // [nreads] picks of the first strand (`pad`: the strand of that pick, as the gate left it); the winner's stays
    const DevRecord* rec2;     // [count] picks of the other strand of the qualifying reads
    const int* idx;            // [count] the qualifying reads, ascending
    int count;
    uint8_t* strand;           // [nreads] in: the first strand of every read (1 = reverse); out: the strand that won
};

const char* launch_gap_pick_out(const ReadState* state, DevRecord* rec, int nreads, hipStream_t s);       // one lane per read
const char* launch_gap_seed_pick(const DevRecord* rec, ReadState* state, int nreads, hipStream_t s);      // one lane per read
const char* launch_gap_xstrands_duel(const GapXStrandsDuelArgs& a, hipStream_t s);                        // one lane per qualifying read
const char* launch_gap_xstrands_mark(DevRecord* rec, const uint8_t* strand, int nreads, hipStream_t s);   // one lane per read

}  // namespace rg
