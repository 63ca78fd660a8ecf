// Both strands inside a pathwise batch (RG_AMB_BOTH_STRANDS, include/recgraph_hip.h): the three small kernels between the
// forward pass and the pass over the reverse complements (rg_strand.hip), launched by rg_run_pathwise (rg_abi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "rg_device.hpp"

namespace rg {

constexpr int32_t REC_REVERSE_STRAND = 1;   // DevRecord.pad of a record that came from the reverse-complement pass

struct StrandGateArgs {
    DevRecord* rec;            // [nreads] records of the forward pass; `pad` is cleared here
    const long long* off;      // [nreads + 1] read offsets
    int nreads;
    int recomb;                // -m 8 / -m 9: a record with two paths prints its f32 score
    int* idx;                  // out [<= nreads]: the qualifying reads, ascending
    long long* rc_off;         // out [<= nreads + 1]: offsets of their reverse complements (prefix sum of the lengths)
    int* summary;              // out [2]: {qualifying reads, their largest length}
};
struct RevcompArgs {
    const uint8_t* reads;      // base codes A0 C1 G2 T3 N4
    const long long* off;
    const int* idx;
    const long long* rc_off;
    const int* summary;
    uint8_t* rc;               // out: reverse-complemented codes of the qualifying reads, back to back
};
struct StrandMergeArgs {
    DevRecord* rec;            // forward records / ops: overwritten where the reverse record wins
    uint8_t* ops;
    const DevRecord* rec2;     // [count] records / ops of the reverse-complement pass
    const uint8_t* ops2;
    long long ops_stride;      // a multiple of 16 (both areas 16-byte aligned)
    const int* idx;
    int count;
    int recomb;
};

void launch_strand_gate(const StrandGateArgs& a, hipStream_t s);
void launch_revcomp(const RevcompArgs& a, int nreads, hipStream_t s);      // one wave per read slot; slots >= summary[0] leave
void launch_strand_merge(const StrandMergeArgs& a, hipStream_t s);

}  // namespace rg
