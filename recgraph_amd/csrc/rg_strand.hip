// Both strands inside a pathwise batch (RG_AMB_BOTH_STRANDS; an extension the reference does not have: its `-s true`
// covers the POA modes only, main.rs:82-106, and modes 4, 5, 8, 9 ignore it, main.rs:254-313).
//
//   forward pass (path_driver_run)  ->  k_strand_gate  ->  k_revcomp  ->  {count, max_len} to the host
//   ->  path_driver_run over the reverse complements  ->  k_strand_merge
//
// A read QUALIFIES for the second pass when its status has neither ST_BAD_BASE nor ST_WOULD_PANIC and the score its record
// prints is < 0 (the reference's rule for the global POA modes, main.rs:82).  The printed score (rg_gaf.cpp) is the integer
// `score`, or the f32 `fscore` of a record with a recombination (two different paths, -m 8 / -m 9).  Two integer scores are
// compared as integers: in modes 26 / 27 / 32 they reach 2^28, where an f32 cannot tell neighbours apart.  Only where a
// record actually prints `fscore` is the comparison one of f32, and there every integer involved is below 2^24.
// The reverse record replaces the forward one only when its printed score is STRICTLY
// greater; ties keep the forward record.  With RG_AMB_STRAND_VOTE (rg_strand_vote.hip) the first pass aligned each read on
// the strand its 12-mers vote for: the gate presets the strand flag from `first_rev`, and the merge keeps the reverse record
// only when it is strictly greater, whichever pass produced it.
//
// This file holds the kernels and their launchers; rg_strand_driver.hip launches them between the passes.
// The kernels are memory-shaped and small on purpose: they run beside the sweeps of other handles, which leave 64 VGPRs
// per SIMD (tests/test_both_strands_cpu.py holds them to that, without scratch).  Plain vector stores only.
#include "rg_strand.hpp"

namespace rg {

namespace {

constexpr int GATE_THREADS = 256;
constexpr int GATE_WAVES = GATE_THREADS / WAVE;

__device__ __forceinline__ bool prints_fscore(const DevRecord& r, int recomb) { return recomb && r.best_path != r.rev_path; }
__device__ __forceinline__ bool printed_negative(const DevRecord& r, int recomb) {
    return prints_fscore(r, recomb) ? r.fscore < 0.0f : r.score < 0;
}
// printed score of x STRICTLY greater than that of y
__device__ __forceinline__ bool printed_greater(const DevRecord& x, const DevRecord& y, int recomb) {
    const bool fx = prints_fscore(x, recomb), fy = prints_fscore(y, recomb);
    if (!(fx || fy)) return x.score > y.score;
    return (fx ? x.fscore : (float)x.score) > (fy ? y.fscore : (float)y.score);      // (recomb modes: |score| < 2^24, exact as f32)
}
__device__ __forceinline__ bool no_record(uint32_t status) { return (status & (ST_BAD_BASE | ST_WOULD_PANIC)) != 0; }

}  // namespace

// ---------------------------------------------------------------------------------
// ONE workgroup walks the records in blocks of 256: ballot + popcount give a qualifying read its slot inside its wave,
// wave_incl_sum the offset of its reverse complement; the four waves' totals meet in LDS, the running totals of the
// blocks before stay in registers (every thread carries the same).  No atomics: slot k holds the k-th qualifying read in
// read order, whatever the timing.
__global__ __launch_bounds__(GATE_THREADS) void k_strand_gate(StrandGateArgs a) {
    __shared__ int s_cnt[GATE_WAVES], s_len[GATE_WAVES], s_max[GATE_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    int slot_base = 0, max_len = 0;
    long long len_base = 0;
    if (tid == 0) a.rc_off[0] = 0;
    for (int base = 0; base < a.nreads; base += GATE_THREADS) {
        const int i = base + tid;
        bool q = false;
        int len = 0;
        if (i < a.nreads) {
            const DevRecord r = a.rec[i];
            q = !no_record(r.status) && printed_negative(r, a.recomb);
            if (q) len = (int)(a.off[i + 1] - a.off[i]);
            a.rec[i].pad = a.first_rev ? (int32_t)a.first_rev[i] : 0;      // (REC_REVERSE_STRAND: the strand of the record so far)
        }
        const unsigned long long bal = __ballot(q);
        const int rank = __popcll(bal & ((1ull << lane) - 1ull));
        const int incl = wave_incl_sum(len, lane);
        const int wmax = wave_incl_max(len, lane);
        if (lane == WAVE - 1) { s_cnt[wv] = __popcll(bal); s_len[wv] = incl; s_max[wv] = wmax; }
        __syncthreads();
        int cnt_before = 0, len_before = 0, cnt_all = 0, len_all = 0;
#pragma unroll
        for (int w = 0; w < GATE_WAVES; ++w) {
            if (w < wv) { cnt_before += s_cnt[w]; len_before += s_len[w]; }
            cnt_all += s_cnt[w]; len_all += s_len[w];
            max_len = max(max_len, s_max[w]);
        }
        if (q) {
            const int slot = slot_base + cnt_before + rank;
            a.idx[slot] = i;
            a.rc_off[slot + 1] = len_base + len_before + incl;
        }
        slot_base += cnt_all;
        len_base += len_all;
        __syncthreads();
    }
    if (tid == 0) { a.summary[0] = slot_base; a.summary[1] = max_len; }
}

// ---------------------------------------------------------------------------------
// Reverse complement of one read per wave (sequences.rs:65-82 on base codes: the complement of c < 4 is 3 - c, N stays).
// The destination is written in aligned dwords: dword t holds bases j .. j + 3 of the result = bases n - 1 - j .. n - 4 - j
// of the read, four consecutive source bytes that two aligned source dwords contain; one v_perm_b32 picks them out of the
// pair in reverse order.  What lies in front of the first aligned destination dword and behind the last whole one goes
// byte by byte.
__global__ __launch_bounds__(WAVE) void k_revcomp(RevcompArgs a) {
    const int k = blockIdx.x;
    if (k >= a.summary[0]) return;
    const int lane = threadIdx.x;
    const int rd = a.idx[k];
    const uint8_t* src = a.reads + a.off[rd];
    const int n = (int)(a.off[rd + 1] - a.off[rd]);
    uint8_t* dst = a.rc + a.rc_off[k];
    auto comp = [](int c) { return c < 4 ? 3 - c : c; };
    const int head = min(n, (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
    const int nd = (n - head) / 4;
    if (lane < head) dst[lane] = (uint8_t)comp(src[n - 1 - lane]);
    for (int t = lane; t < nd; t += WAVE) {
        const int j = head + 4 * t;
        const uintptr_t p = reinterpret_cast<uintptr_t>(src) + (uintptr_t)(n - 4 - j);
        const unsigned sh = (unsigned)(p & 3);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
        const uint32_t lo = q[0];
        const uint32_t hi = sh ? q[1] : lo;           // (an aligned source needs no second dword: none is read behind the reads)
        // result byte i = source byte 3 - i of the four = byte sh + 3 - i of the pair {hi : lo}
        uint32_t w = __builtin_amdgcn_perm(hi, lo, 0x00010203u + sh * 0x01010101u);
        w ^= 3u * (0x01010101u & ~(w >> 2));           // 3 - c in every byte below 4; 4 (N) keeps its value
        *reinterpret_cast<uint32_t*>(dst + j) = w;
    }
    const int tail0 = head + 4 * nd;
    if (lane < n - tail0) dst[tail0 + lane] = (uint8_t)comp(src[n - 1 - tail0 - lane]);
}

// ---------------------------------------------------------------------------------
// One wave per qualifying read: where the reverse record wins, its 64 bytes (four lanes, 16 bytes each) and its op bytes
// (16 bytes per lane and round) replace the forward ones, and the record is marked REC_REVERSE_STRAND.  A reverse pass that
// produced no record (the reference would panic on the reverse complement) never wins: the forward record stays.
__global__ __launch_bounds__(WAVE) void k_strand_merge(StrandMergeArgs a) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= a.count) return;
    const int rd = a.idx[k];
    const DevRecord r = a.rec2[k];
    if (no_record(r.status)) return;
    const DevRecord f = a.rec[rd];
    // (RG_AMB_STRAND_VOTE: a read whose first pass was the reverse one, `pad` preset by the gate, has its FORWARD record
    // here: it replaces the reverse one unless that is strictly greater.  Without the vote `pad` is 0 on every read.)
    const bool first_rev = (f.pad & REC_REVERSE_STRAND) != 0;
    if (first_rev ? printed_greater(f, r, a.recomb) : !printed_greater(r, f, a.recomb)) return;
    static_assert(sizeof(DevRecord) == 4 * sizeof(int4), "a record is four 16-byte pieces");
    if (lane < 4) {
        int4 v = reinterpret_cast<const int4*>(a.rec2 + k)[lane];
        if (lane == 3) v.w = first_rev ? 0 : REC_REVERSE_STRAND;       // DevRecord::pad
        reinterpret_cast<int4*>(a.rec + rd)[lane] = v;
    }
    const int4* so = reinterpret_cast<const int4*>(a.ops2 + (long long)k * a.ops_stride);
    int4* dn = reinterpret_cast<int4*>(a.ops + (long long)rd * a.ops_stride);
    const int pieces = (int)min((long long)(r.n_ops + 15) / 16, a.ops_stride / 16);
    for (int t = lane; t < pieces; t += WAVE) dn[t] = so[t];
}

const char* launch_strand_gate(const StrandGateArgs& a, hipStream_t s) {
    RG_LAUNCH0(k_strand_gate, dim3(1), dim3(GATE_THREADS), 0, s, a);
}
const char* launch_revcomp(const RevcompArgs& a, int nreads, hipStream_t s) {
    RG_LAUNCH0(k_revcomp, dim3(nreads), dim3(WAVE), 0, s, a);
}
const char* launch_strand_merge(const StrandMergeArgs& a, hipStream_t s) {
    RG_LAUNCH0(k_strand_merge, dim3(a.count), dim3(WAVE), 0, s, a);
}

}  // namespace rg
