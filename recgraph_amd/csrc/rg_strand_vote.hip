// The first strand by a 12-mer vote (RG_AMB_STRAND_VOTE, include/recgraph_hip.h): in front of the first pass of
// RG_AMB_BOTH_STRANDS,
//
//   k_strand_vote  ->  k_strand_orient  ->  pass A (path_driver_run over the oriented reads)  ->  k_strand_gate  ->  ...
//
// (launched by rg_run_pathwise, rg_strand_driver.hip: no host synchronisation between the vote and pass A).
// The vote is a pure function of (graph, read): V_f / V_r = how many sampled 12-mers of the read / of its reverse
// complement occur in some path (k_pick's sampling, k_pick's table, membership only).  The first pass aligns the reverse
// complement iff V_r > V_f.
//
// Like the kernels of rg_strand.hip these two run beside other handles' sweeps: at most 64 VGPRs, no scratch, plain
// vector stores (tests/test_strand_vote_cpu.py).
#include "rg_strand.hpp"

namespace rg {

namespace {

constexpr int VOTE_K = 12;
constexpr int VOTE_SAMPLES = 256;

// exact membership: the table is at most half full, so the probe sequence ends at an empty slot
__device__ __forceinline__ bool kmer_present(const uint32_t* keys, unsigned mask, unsigned key) {
    unsigned slot = ((key * 2654435761u) >> 8) & mask;
    for (;;) {
        const unsigned kk = keys[slot];
        if (kk == key) return true;
        if (kk == 0xffffffffu) return false;
        slot = (slot + 1) & mask;
    }
}

// the 12 bases at p as a 24-bit key, first base in the highest pair; false: a base outside ACGT among them
__device__ __forceinline__ bool window_key(const uint8_t* p, unsigned& key) {
    key = 0;
    bool ok = true;
#pragma unroll
    for (int e = 0; e < VOTE_K; ++e) { const unsigned c = p[e]; ok = ok && c < 4; key = (key << 2) | (c & 3u); }
    return ok;
}

// key of the reverse complement of a window: every pair complemented (3 - c = c ^ 3), the twelve pairs in reverse order
__device__ __forceinline__ unsigned revcomp_key(unsigned key) {
    unsigned v = ~key & 0xffffffu;
    v = ((v >> 2) & 0x333333u) | ((v & 0x333333u) << 2);            // pairs inside nibbles
    v = ((v >> 4) & 0x0f0f0fu) | ((v & 0x0f0f0fu) << 4);            // nibbles inside bytes
    return ((v >> 16) & 0xffu) | (v & 0xff00u) | ((v & 0xffu) << 16);   // the three bytes
}

}  // namespace

// ---------------------------------------------------------------------------------
// One wave per read.  Lane l takes the samples t = l, l + 64, ... < nsamp.  Sample t of the read is the window at t * step;
// sample t of the reverse complement, in ITS coordinates, is the complemented, reversed window of the read at
// npos - 1 - t * step: both keys come out of the read as it lies in memory.  Ballot + popcount count the hits.
__global__ __launch_bounds__(WAVE) void k_strand_vote(StrandVoteArgs a) {
    const int rd = blockIdx.x, lane = threadIdx.x;
    const long long ro = a.off[rd];
    const int n = (int)(a.off[rd + 1] - ro);
    const int npos = n - VOTE_K + 1;
    int vf = 0, vr = 0;
    if (!a.bad[rd] && npos >= 1) {
        const int step = (npos + VOTE_SAMPLES - 1) / VOTE_SAMPLES;
        const int nsamp = (npos + step - 1) / step;          // <= 256
        const uint8_t* src = a.reads + ro;
        for (int base = 0; base < nsamp; base += WAVE) {
            const int t = base + lane;
            bool hf = false, hr = false;
            if (t < nsamp) {
                const int q = t * step;
                unsigned key;
                if (window_key(src + q, key)) hf = kmer_present(a.keys, a.table_mask, key);
                if (window_key(src + (npos - 1 - q), key)) hr = kmer_present(a.keys, a.table_mask, revcomp_key(key));
            }
            vf += __popcll(__ballot(hf));
            vr += __popcll(__ballot(hr));
        }
    }
    if (lane == 0) a.first_rev[rd] = vr > vf ? 1 : 0;
}

// ---------------------------------------------------------------------------------
// One wave per read: the read as it is, or its reverse complement (k_revcomp's scheme), into `out` at the read's own
// offset.  The destination goes in aligned dwords; destination bytes j .. j + 3 are the source bytes j .. j + 3, or
// n - 1 - j .. n - 4 - j complemented: four consecutive source bytes out of two aligned source dwords, picked by one
// v_perm_b32 in either order.  Head and tail in front of / behind the aligned dwords go byte by byte.
__global__ __launch_bounds__(WAVE) void k_strand_orient(StrandOrientArgs a) {
    const int rd = blockIdx.x, lane = threadIdx.x;
    const long long ro = a.off[rd];
    const int n = (int)(a.off[rd + 1] - ro);
    const bool rev = a.first_rev[rd] != 0;
    const uint8_t* src = a.reads + ro;
    uint8_t* dst = a.out + ro;
    auto pick = [&](int j) { const int c = rev ? src[n - 1 - j] : src[j]; return (uint8_t)(rev && c < 4 ? 3 - c : c); };
    const int head = min(n, (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
    const int nd = (n - head) / 4;
    if (lane < head) dst[lane] = pick(lane);
    for (int t = lane; t < nd; t += WAVE) {
        const int j = head + 4 * t;
        const uintptr_t p = reinterpret_cast<uintptr_t>(src) + (uintptr_t)(rev ? n - 4 - j : j);
        const unsigned sh = (unsigned)(p & 3);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
        const uint32_t lo = q[0];
        const uint32_t hi = sh ? q[1] : lo;           // (an aligned source needs no second dword: none is read behind the reads)
        // result byte i = byte sh + i of the pair {hi : lo}, or byte sh + 3 - i for the reverse
        uint32_t w = __builtin_amdgcn_perm(hi, lo, (rev ? 0x00010203u : 0x03020100u) + sh * 0x01010101u);
        if (rev) w ^= 3u * (0x01010101u & ~(w >> 2));  // 3 - c in every byte below 4; 4 (N) keeps its value
        *reinterpret_cast<uint32_t*>(dst + j) = w;
    }
    const int tail0 = head + 4 * nd;
    if (lane < n - tail0) dst[tail0 + lane] = pick(tail0 + lane);
}

const char* launch_strand_vote(const StrandVoteArgs& a, int nreads, hipStream_t s) {
    RG_LAUNCH0(k_strand_vote, dim3(nreads), dim3(WAVE), 0, s, a);
}
const char* launch_strand_orient(const StrandOrientArgs& a, int nreads, hipStream_t s) {
    RG_LAUNCH0(k_strand_orient, dim3(nreads), dim3(WAVE), 0, s, a);
}

}  // namespace rg
