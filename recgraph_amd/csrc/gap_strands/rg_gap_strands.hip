// Both strands in the local affine-gap pathwise mode (-m 32): the kernel between the forward pass and the pass over the reverse
// complements.
//
//   forward pass (path_driver_run, pipeline 22)  ->  k_gap_strands_gate  ->  k_revcomp  ->  {count, max_len} to the host
//   ->  path_driver_run over the reverse complements  ->  k_strand_merge
//
// k_strand_gate (rg_strand.hip) sends a read to the second pass when its printed score is < 0.  A local score never is, so here
// a read QUALIFIES when it HAS A RECORD: its status has neither ST_BAD_BASE nor ST_WOULD_PANIC.  A read without a local alignment
// (RG_READ_UNALIGNED) has one, with score 0 and no ops, and qualifies too: its reverse complement may align.  k_strand_merge then
// keeps the reverse record only when its score is strictly greater, so two unaligned strands stay '+', unaligned and without a line.
//
// Everything else is the contract of k_strand_gate: slot k holds the k-th qualifying read in read order (no atomics), rc_off the
// prefix sum of their lengths, summary {count, largest length}, and the strand flag (DevRecord.pad) is cleared on every record.
// Small on purpose, like its siblings: it runs beside the Gotoh waves of other handles (at most 64 VGPRs, no scratch; plain
// vector stores only — tests/test_pathwise_gap_strands_cpu.py).
#include "rg_gap_strands.hpp"

namespace rg {

namespace {

constexpr int GATE_THREADS = 256;
constexpr int GATE_WAVES = GATE_THREADS / WAVE;

}  // namespace

// ONE workgroup walks the records in blocks of 256: ballot + popcount give a qualifying read its slot inside its wave,
// wave_incl_sum the offset of its reverse complement; the four waves' totals meet in LDS, the running totals of the blocks
// before stay in registers (every thread carries the same).  Only the status word and `pad` of a record are touched.
__global__ __launch_bounds__(GATE_THREADS) void k_gap_strands_gate(StrandGateArgs a) {
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
            q = (a.rec[i].status & (ST_BAD_BASE | ST_WOULD_PANIC)) == 0;
            if (q) len = (int)(a.off[i + 1] - a.off[i]);
            a.rec[i].pad = 0;      // (REC_REVERSE_STRAND: every record so far is a forward one)
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

const char* launch_gap_strands_gate(const StrandGateArgs& a, hipStream_t s) {
    RG_LAUNCH0(k_gap_strands_gate, dim3(1), dim3(GATE_THREADS), 0, s, a);
}

}  // namespace rg
