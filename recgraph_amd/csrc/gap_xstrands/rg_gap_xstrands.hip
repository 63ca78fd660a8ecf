// Both strands at up to 131071 bases, traced once (-m 76 / -m 77 / -m 82): the kernels that carry a PICK out of the pipeline of
// -m 56 / -m 57 / -m 62 and back into it, and the one that decides between the picks of the two strands.
//
//   PICK(first strand, all reads)  ->  gate  ->  k_revcomp  ->  {count, max_len} to the host  ->  PICK(other strand, qualifying reads)
//   ->  k_gap_xstrands_duel  ->  k_strand_orient(strand that won)  ->  TRACE(all reads)  ->  k_gap_xstrands_mark
//
// (rg_strand_driver.hip; the stages: rg_path_driver.hip.)  The score that decides is the integer the pick leaves, which no traceback
// changes, so the losing strand is never traced and there is no op area to copy from: the duel moves 64 bytes per read at the most.
//
// All four are memory-shaped and a few instructions long, one lane per read: they run beside the Gotoh waves of other handles.  No
// LDS, no atomics, no scratch, plain vector stores only (tests/test_pathwise_gap_xstrands_cpu.py holds them to 48 VGPRs).
#include "rg_gap_xstrands.hpp"

namespace rg {

namespace {

constexpr int XS_THREADS = 256;
inline dim3 xs_grid(int n) { return dim3((unsigned)((n + XS_THREADS - 1) / XS_THREADS)); }

__device__ __forceinline__ bool no_record(uint32_t status) { return (status & (ST_BAD_BASE | ST_WOULD_PANIC)) != 0; }

}  // namespace

// What gap_pick_wave left of read i, as a record without ops (a read without a pick — bad base, too long, unaligned — left its
// status alone, and the rest of its ReadState is the zeros the chunk started from).
__global__ __launch_bounds__(XS_THREADS) void k_gap_pick_out(const ReadState* state, DevRecord* rec, int nreads) {
    const int i = blockIdx.x * XS_THREADS + threadIdx.x;
    if (i >= nreads) return;
    const ReadState* rs = state + i;
    DevRecord r;
    r.status = rs->status;
    r.score = rs->trace_score;
    r.fscore = 0.f;
    r.end_row = rs->end_row; r.end_col = 0;
    r.stop_row = 0; r.stop_col = 0;
    r.best_path = rs->fwd_path; r.rev_path = rs->fwd_path;
    r.fen = 0; r.rsn = 0; r.rec_col = 0; r.displacement = 0;
    r.n_ops = 0; r.n_fwd_ops = 0;
    r.pad = 0;
    rec[i] = r;
}

// The inverse: the fields gap_pick_wave writes, from the pick in the record (the chunk's ReadState was cleared before).
__global__ __launch_bounds__(XS_THREADS) void k_gap_seed_pick(const DevRecord* rec, ReadState* state, int nreads) {
    const int i = blockIdx.x * XS_THREADS + threadIdx.x;
    if (i >= nreads) return;
    const DevRecord r = rec[i];
    ReadState* rs = state + i;
    rs->status = r.status;
    rs->s0 = r.score; rs->bound = r.score; rs->trace_score = r.score;
    rs->seed_path = r.best_path; rs->fwd_path = r.best_path; rs->rev_path = r.best_path;
    rs->end_row = r.end_row; rs->end_row_best = r.end_row;
}

// k_strand_merge's decision (rg_strand.hip) on two picks: the first strand's pick stays unless the other strand's has a record and
// wins — reverse only when STRICTLY greater, whichever strand went first (an unaligned local pick scores 0).  The winner's pick
// replaces rec[rd], and the read's strand byte says which strand that is.  "Scores 0" is not computed here: k_gap_pick_local leaves
// the ReadState of an unaligned read alone, the stage clears every chunk's ReadState before the pick, and k_gap_pick_out copies
// trace_score — so the comparison below depends on that clearing.
__global__ __launch_bounds__(XS_THREADS) void k_gap_xstrands_duel(GapXStrandsDuelArgs a) {
    const int k = blockIdx.x * XS_THREADS + threadIdx.x;
    if (k >= a.count) return;
    const int rd = a.idx[k];
    const DevRecord* r = a.rec2 + k;
    DevRecord* f = a.rec + rd;
    if (no_record(r->status)) return;
    const bool first_rev = (f->pad & REC_REVERSE_STRAND) != 0;
    const int sf = f->score, sr = r->score;      // (first | other strand)
    if (first_rev ? sf > sr : !(sr > sf)) return;
    // the record as four 16-byte pieces, DevRecord::pad (the last word) set on the way: a copy of the struct that is then modified
    // would be placed in LDS by the compiler
    static_assert(sizeof(DevRecord) == 4 * sizeof(int4), "a record is four 16-byte pieces");
    const int4* src = reinterpret_cast<const int4*>(r);
    int4* dst = reinterpret_cast<int4*>(f);
    const int4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
    dst[0] = v0; dst[1] = v1; dst[2] = v2;
    dst[3] = make_int4(v3.x, v3.y, v3.z, first_rev ? 0 : REC_REVERSE_STRAND);
    a.strand[rd] = first_rev ? 0 : 1;
}

// The strand flag of every record, behind the traceback (write_record and no_record know nothing of strands).
__global__ __launch_bounds__(XS_THREADS) void k_gap_xstrands_mark(DevRecord* rec, const uint8_t* strand, int nreads) {
    const int i = blockIdx.x * XS_THREADS + threadIdx.x;
    if (i >= nreads) return;
    rec[i].pad = strand[i] ? REC_REVERSE_STRAND : 0;
}

const char* launch_gap_pick_out(const ReadState* state, DevRecord* rec, int nreads, hipStream_t s) {
    if (!state || !rec || nreads < 1) return nullptr;
    RG_LAUNCH0(k_gap_pick_out, xs_grid(nreads), dim3(XS_THREADS), 0, s, state, rec, nreads);
}
const char* launch_gap_seed_pick(const DevRecord* rec, ReadState* state, int nreads, hipStream_t s) {
    if (!state || !rec || nreads < 1) return nullptr;
    RG_LAUNCH0(k_gap_seed_pick, xs_grid(nreads), dim3(XS_THREADS), 0, s, rec, state, nreads);
}
const char* launch_gap_xstrands_duel(const GapXStrandsDuelArgs& a, hipStream_t s) {
    if (!a.rec || !a.rec2 || !a.idx || !a.strand || a.count < 1) return nullptr;
    RG_LAUNCH0(k_gap_xstrands_duel, xs_grid(a.count), dim3(XS_THREADS), 0, s, a);
}
const char* launch_gap_xstrands_mark(DevRecord* rec, const uint8_t* strand, int nreads, hipStream_t s) {
    if (!rec || !strand || nreads < 1) return nullptr;
    RG_LAUNCH0(k_gap_xstrands_mark, xs_grid(nreads), dim3(XS_THREADS), 0, s, rec, strand, nreads);
}

}  // namespace rg
