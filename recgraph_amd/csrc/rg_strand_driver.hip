// Batch driver of the pathwise modes (-m 4 to 9 and the affine-gap families of rg_gap_modes.hpp) above the pipeline of
// rg_path_driver.hip: one pass over the reads, or, with RG_AMB_BOTH_STRANDS (-m 4, 5, 8, 9 by the bit; a both-strands family always:
// rg_batch_create sets it on its handles), two passes joined by the small kernels of rg_strand.hip (and opened by those of
// rg_strand_vote.hip under RG_AMB_STRAND_VOTE, which the local rule does not have):
//
//   [k_strand_vote -> k_strand_orient ->]  pass A  [-> k_strand_gate -> k_revcomp -> {count, max_len} to the host
//   -> pass B over the reverse complements of the qualifying reads -> k_strand_merge]
//
// The local rule gates with k_gap_strands_gate (gap_strands/rg_gap_strands.hip) instead: every read that has a record qualifies.  In
// the affine-gap modes each pass is planned by its own longest read, so one may run the striped kernels and the other the base ones.
// Every pass is path_driver_run on the same context; the passes differ in their PathJob alone.  The work buffers are owned by
// PathWork, the strand buffers by the handle (size_strand_buffers).
//
// A staged family (both strands at up to 131071 bases) is not two passes but two PICK stages and one TRACE stage: run_gap_xstrands below.
// The both-strands edit-distance modes (-m 64 / -m 65) are ONE pass: its score kernel holds both strands in one wave, and none of the
// strand buffers here exists on their handles.
#include "gap_strands/rg_gap_strands.hpp"
#include "gap_xstrands/rg_gap_xstrands.hpp"
#include "rg_batch_impl.hpp"

int size_strand_buffers(rg_batch* b, size_t total) {
    const size_t n = (size_t)b->nreads;
    // the second pass's inputs and its record / op area: 64 B + ops_stride per read, worst case every read
    RG_TRY(b->d_sidx.alloc(n));
    RG_TRY(b->d_ssum.alloc(2));
    RG_TRY(b->d_rcoff.alloc(n + 1));
    RG_TRY(b->d_rc.alloc(total + 64));
    RG_TRY(b->d_rcbad.alloc(n));
    RG_TRY(b->d_rec2.alloc(n));
    // (a staged family traces one strand per read, into d_ops: no second op area — at 131071 bases it would be the largest
    // buffer of the handle; its strand byte and its trace input take the vote's two buffers, vote or not)
    const bool staged = gap_mode(b->p.mode).family->staged;
    if (!staged) RG_TRY(b->d_ops2.alloc(n * b->ops_stride));
    RG_TRY(b->h_ssum.alloc(2));
    if (staged || (b->p.amb_mode & RG_AMB_STRAND_VOTE)) {
        RG_TRY(b->d_first_rev.alloc(n));
        RG_TRY(b->d_pa.alloc(total + 64));
    }
    return RG_OK;
}

// ---- what the two runners below share ----

// The first strand of every read, in front of the first job `a`: under RG_AMB_STRAND_VOTE the strand its 12-mers vote for (the answer
// in d_first_rev), each read oriented into d_pa at the input's own offsets, and `a` reads from there; otherwise the reads as given —
// and (`staged`) a strand byte of zero, which the staged runner reads vote or not.  No host synchronisation: the job's first collect
// takes the two vote kernels' times with its own.
static int first_strand(rg_batch* b, bool staged, PathJob& a) {
    const int n = (int)b->nreads;
    KernelTimer& T = b->timer;
    if (!(b->p.amb_mode & RG_AMB_STRAND_VOTE)) {
        if (staged) HIPCHK(hipMemsetAsync(b->d_first_rev.p, 0, (size_t)n, b->stream));
        return RG_OK;
    }
    const uint32_t* keys = nullptr;
    unsigned table_mask = 0;
    RG_TRY(path_driver_vote_table(b->g->h, b->pw, &keys, &table_mask));
    StrandVoteArgs va{b->in.reads, b->in.off, b->in.bad, keys, table_mask, b->d_first_rev.p};
    RG_TRY(T.run("k_strand_vote", [&] { return launch_strand_vote(va, n, b->stream); }));
    StrandOrientArgs oa{b->in.reads, b->in.off, b->d_first_rev.p, b->d_pa.p};
    RG_TRY(T.run("k_strand_orient", [&] { return launch_strand_orient(oa, n, b->stream); }));
    a.reads = b->d_pa.p;
    return RG_OK;
}

static int impossible_gate() { return fail(RG_ERR_HIP, "k_strand_gate returned an impossible read count / length"); }

// The reads that go on to the other strand, from the records (or picks) of the first job in d_rec: the gate (the local rule's: every
// read that has a record; both read status and score only), their reverse complements into d_rc / d_rcoff, and {count, max_len} on
// the host.  A count above n and, where reads qualify, a length outside [1, max_n] are refused here; what a count <= 0 means is the
// caller's.  `first_reads`: what the first job read.
static int other_strand_reads(rg_batch* b, int recomb, const uint8_t* first_reads, int* count, int* max_len) {
    const int n = (int)b->nreads;
    KernelTimer& T = b->timer;
    StrandGateArgs ga{b->d_rec.p, b->in.off, n, recomb, b->d_sidx.p, b->d_rcoff.p, b->d_ssum.p, (b->p.amb_mode & RG_AMB_STRAND_VOTE) ? b->d_first_rev.p : nullptr};
    if (gap_mode(b->p.mode).rule == GAP_RULE_LOCAL) RG_TRY(T.run("k_gap_strands_gate", [&] { return launch_gap_strands_gate(ga, b->stream); }));
    else RG_TRY(T.run("k_strand_gate", [&] { return launch_strand_gate(ga, b->stream); }));
    RevcompArgs ra{first_reads, b->in.off, b->d_sidx.p, b->d_rcoff.p, b->d_ssum.p, b->d_rc.p};
    RG_TRY(T.run("k_revcomp", [&] { return launch_revcomp(ra, n, b->stream); }));
    HIPCHK(hipMemcpyAsync(b->h_ssum.p, b->d_ssum.p, 2 * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    RG_TRY(T.collect(b->stats));
    *count = b->h_ssum.p[0];
    *max_len = b->h_ssum.p[1];
    if (*count > n || (*count > 0 && (*max_len < 1 || *max_len > b->max_n))) return impossible_gate();
    return RG_OK;
}

// The staged families (both strands at up to 131071 bases, the traceback run once per read: include/recgraph_hip.h,
// RG_MODE_PATHWISE_GAP_XSTRANDS).  The strand rule of the two-pass family needs the SCORES of the two strands, and
// those are final after the pick: two PICK stages and one TRACE stage of path_driver_run, each planned by its own longest read,
// joined by the gate and k_revcomp as they are and by the kernels of gap_xstrands/:
//
//   [k_strand_vote -> k_strand_orient ->]  PICK(first strand, all reads) -> d_rec  ->  k_strand_gate | k_gap_strands_gate  ->  k_revcomp
//   ->  {count, max_len} to the host  [->  PICK(other strand, qualifying reads) -> d_rec2  ->  k_gap_xstrands_duel]
//   ->  k_strand_orient(the strand that won)  ->  TRACE(all reads) -> d_rec, d_ops  ->  k_gap_xstrands_mark
//
// The strand byte of a read lives in d_first_rev (the vote's answer, or zeros), flipped by the duel where the other strand wins;
// d_pa is the first PICK's input under the vote and the TRACE's input always (every kernel that read the first is through by then:
// one stream).  The walk's record writer clears DevRecord.pad, so the strand flag goes on behind the TRACE stage.
static int run_gap_xstrands(rg_batch* b) {
    const HostGraph& h = b->g->h;
    const int n = (int)b->nreads;
    KernelTimer& T = b->timer;
    const PathCtx cx{h, b->gt->pgd, b->p, b->pw, b->stream, b->d_cells.p, b->mem_budget, T, b->stats, 0};
    unsigned long long cells[2] = {0, 0};
    auto counters = [&] { b->cells = cells[0]; b->cells_performed = cells[1]; };
    PathJob a{b->in.reads, b->in.off, b->in.bad, n, b->max_n, b->d_rec.p, nullptr, b->ops_stride, PATH_STAGE_PICK};
    RG_TRY(first_strand(b, true, a));
    const int rc_a = path_driver_run(cx, a, cells);
    counters();
    if (rc_a) return rc_a;
    int count = 0, max_len = 0;
    RG_TRY(other_strand_reads(b, 0, a.reads, &count, &max_len));
    if (count < 0) return impossible_gate();
    if (count > 0) {
        HIPCHK(hipMemsetAsync(b->d_rcbad.p, 0, (size_t)count, b->stream));
        const PathJob other{b->d_rc.p, b->d_rcoff.p, b->d_rcbad.p, count, max_len, b->d_rec2.p, nullptr, b->ops_stride, PATH_STAGE_PICK};
        const int rc_b = path_driver_run(cx, other, cells);
        counters();
        if (rc_b) return rc_b;
        GapXStrandsDuelArgs da{b->d_rec.p, b->d_rec2.p, b->d_sidx.p, count, b->d_first_rev.p};
        RG_TRY(T.run("k_gap_xstrands_duel", [&] { return launch_gap_xstrands_duel(da, b->stream); }));
    }
    // every read on the strand that won, at the input's own offsets, and the traceback of those
    StrandOrientArgs oa{b->in.reads, b->in.off, b->d_first_rev.p, b->d_pa.p};
    RG_TRY(T.run("k_strand_orient", [&] { return launch_strand_orient(oa, n, b->stream); }));
    const PathJob trace{b->d_pa.p, b->in.off, b->in.bad, n, b->max_n, b->d_rec.p, b->d_ops.p, b->ops_stride, PATH_STAGE_TRACE};
    const int rc_t = path_driver_run(cx, trace, cells);
    counters();
    if (rc_t) return rc_t;
    RG_TRY(T.run("k_gap_xstrands_mark", [&] { return launch_gap_xstrands_mark(b->d_rec.p, b->d_first_rev.p, n, b->stream); }));
    return T.collect(b->stats);
}

int rg_run_pathwise(rg_batch* b) {
    if (gap_mode(b->p.mode).family->staged) return run_gap_xstrands(b);
    const HostGraph& h = b->g->h;
    const int n = (int)b->nreads;
    KernelTimer& T = b->timer;
    const PathCtx cx{h, b->gt->pgd, b->p, b->pw, b->stream, b->d_cells.p, b->mem_budget, T, b->stats, 0};
    unsigned long long cells[2] = {0, 0};      // counted | performed, summed over the passes (the workload grows with pass B)
    // pass A: the reads as given, or (RG_AMB_STRAND_VOTE) each on the strand its 12-mers vote for, at the same offsets
    PathJob a{b->in.reads, b->in.off, b->in.bad, n, b->max_n, b->d_rec.p, b->d_ops.p, b->ops_stride};
    // -m 64 / -m 65: both strands are scored inside that one pass, which decides and marks the strand itself (rg_path_driver.hip:
    // enqueue_pathwise_edit_strands); it needs the offsets on the host as well
    const bool one_pass = edit_strands_mode(b->p.mode).valid;
    if (one_pass) a.h_off = b->off.data();
    else RG_TRY(first_strand(b, false, a));
    const int rc_a = path_driver_run(cx, a, cells);
    b->cells = cells[0];
    b->cells_performed = cells[1];
    if (rc_a || one_pass || !(b->p.amb_mode & RG_AMB_BOTH_STRANDS)) return rc_a;
    // the qualifying reads once more, on the other strand, in the same work buffers
    const int recomb = b->p.mode == RG_MODE_RECOMBINATION || b->p.mode == RG_MODE_RECOMBINATION_SEMI ? 1 : 0;
    int count = 0, max_len = 0;
    RG_TRY(other_strand_reads(b, recomb, a.reads, &count, &max_len));
    if (count <= 0) return RG_OK;
    HIPCHK(hipMemsetAsync(b->d_rcbad.p, 0, (size_t)count, b->stream));
    const PathJob rev{b->d_rc.p, b->d_rcoff.p, b->d_rcbad.p, count, max_len, b->d_rec2.p, b->d_ops2.p, b->ops_stride};
    RG_TRY(path_driver_run(cx, rev, cells));
    b->cells = cells[0];
    b->cells_performed = cells[1];
    StrandMergeArgs ma{b->d_rec.p, b->d_ops.p, b->d_rec2.p, b->d_ops2.p, b->ops_stride, b->d_sidx.p, count, recomb};
    RG_TRY(T.run("k_strand_merge", [&] { return launch_strand_merge(ma, b->stream); }));
    return T.collect(b->stats);
}
