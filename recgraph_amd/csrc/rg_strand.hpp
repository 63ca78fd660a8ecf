// Both strands inside a pathwise batch (RG_AMB_BOTH_STRANDS, include/recgraph_hip.h): the three small kernels between the
// forward pass and the pass over the reverse complements (rg_strand.hip), and the two of the strand vote in front of the first
// pass (rg_strand_vote.hip).  Their host half — buffer sizing and the order of the passes — is rg_strand_driver.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rg_device.hpp"
#include "rg_launch_log.hpp"

namespace rg {

constexpr int32_t REC_REVERSE_STRAND = 1;   // DevRecord.pad of a record that came from the reverse-complement pass

struct StrandGateArgs {
    DevRecord* rec;            // [nreads] records of the first pass; `pad` is cleared here, or preset from `first_rev`
    const long long* off;      // [nreads + 1] read offsets
    int nreads;
    int recomb;                // -m 8 / -m 9: a record with two paths prints its f32 score
    int* idx;                  // out [<= nreads]: the qualifying reads, ascending
    long long* rc_off;         // out [<= nreads + 1]: offsets of their reverse complements (prefix sum of the lengths)
    int* summary;              // out [2]: {qualifying reads, their largest length}
    const uint8_t* first_rev;  // RG_AMB_STRAND_VOTE: [nreads] 1 = the first pass aligned the reverse complement; null without the bit
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
    DevRecord* rec;            // records / ops of the first pass: overwritten where the second pass's record is chosen
    uint8_t* ops;
    const DevRecord* rec2;     // [count] records / ops of the reverse-complement pass
    const uint8_t* ops2;
    long long ops_stride;      // a multiple of 16 (both areas 16-byte aligned)
    const int* idx;
    int count;
    int recomb;
};

// RG_AMB_STRAND_VOTE (rg_strand_vote.hip): which strand the first pass aligns, and that pass's read buffer
struct StrandVoteArgs {
    const uint8_t* reads;      // base codes A0 C1 G2 T3 N4
    const long long* off;      // [nreads + 1]
    const uint8_t* bad;        // [nreads] reads with RG_READ_BAD_BASE vote 0 / 0
    const uint32_t* keys;      // the paths' 12-mers (build_kmer_table): 24-bit keys, 0xffffffff = empty, at most half full
    unsigned table_mask;
    uint8_t* first_rev;        // out [nreads]: 1 iff V_r > V_f
};
struct StrandOrientArgs {
    const uint8_t* reads;
    const long long* off;
    const uint8_t* first_rev;
    uint8_t* out;              // the read, or its reverse complement, at the SAME offset (3 bytes of slack behind the last read)
};

const char* launch_strand_vote(const StrandVoteArgs& a, int nreads, hipStream_t s);        // one wave per read
const char* launch_strand_orient(const StrandOrientArgs& a, int nreads, hipStream_t s);    // one wave per read
const char* launch_strand_gate(const StrandGateArgs& a, hipStream_t s);
const char* launch_revcomp(const RevcompArgs& a, int nreads, hipStream_t s);      // one wave per read slot; slots >= summary[0] leave
const char* launch_strand_merge(const StrandMergeArgs& a, hipStream_t s);

}  // namespace rg
