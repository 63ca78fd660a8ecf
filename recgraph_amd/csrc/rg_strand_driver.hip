// Batch driver of the pathwise modes (-m 4 to 9, 12, 16, 17, 22, and 26, 27, 32) above the pipeline of rg_path_driver.hip: one pass
// over the reads, or, with RG_AMB_BOTH_STRANDS (-m 4, 5, 8, 9 by the bit; -m 26, 27, 32 always: rg_batch_create sets it on their
// handles), two passes joined by the small kernels of rg_strand.hip (and opened by those of rg_strand_vote.hip under
// RG_AMB_STRAND_VOTE, -m 4, 5, 8, 9, 26, 27):
//
//   [k_strand_vote -> k_strand_orient ->]  pass A  [-> k_strand_gate -> k_revcomp -> {count, max_len} to the host
//   -> pass B over the reverse complements of the qualifying reads -> k_strand_merge]
//
// -m 32 gates with k_gap_strands_gate (gap_strands/rg_gap_strands.hip) instead: every read that has a record qualifies.  In the
// affine-gap modes each pass is planned by its own longest read, so one may run the striped kernels and the other the base ones.
// Every pass is path_driver_run on the same context; the passes differ in their PathJob alone.  The work buffers are owned by
// PathWork, the strand buffers by the handle (size_strand_buffers).
#include "gap_strands/rg_gap_strands.hpp"
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
    RG_TRY(b->d_ops2.alloc(n * b->ops_stride));
    RG_TRY(b->h_ssum.alloc(2));
    if (b->p.amb_mode & RG_AMB_STRAND_VOTE) {
        RG_TRY(b->d_first_rev.alloc(n));
        RG_TRY(b->d_pa.alloc(total + 64));
    }
    return RG_OK;
}

int rg_run_pathwise(rg_batch* b) {
    const HostGraph& h = b->g->h;
    const int n = (int)b->nreads;
    const bool vote = (b->p.amb_mode & RG_AMB_STRAND_VOTE) != 0;
    KernelTimer& T = b->timer;
    const PathCtx cx{h, b->gt->pgd, b->p, b->pw, b->stream, b->d_cells.p, b->mem_budget, T, b->stats, 0};
    unsigned long long cells[2] = {0, 0};      // counted | performed, summed over the passes (the workload grows with pass B)
    // pass A: the reads as given, or (RG_AMB_STRAND_VOTE) each on the strand its 12-mers vote for, at the same offsets; no host
    // synchronisation in front of the pass, whose first collect takes the two vote kernels' times with its own
    PathJob a{b->in.reads, b->in.off, b->in.bad, n, b->max_n, b->d_rec.p, b->d_ops.p, b->ops_stride};
    if (vote) {
        const uint32_t* keys = nullptr;
        unsigned table_mask = 0;
        RG_TRY(path_driver_vote_table(h, b->pw, &keys, &table_mask));
        StrandVoteArgs va{b->in.reads, b->in.off, b->in.bad, keys, table_mask, b->d_first_rev.p};
        RG_TRY(T.run("k_strand_vote", [&] { return launch_strand_vote(va, n, b->stream); }));
        StrandOrientArgs oa{b->in.reads, b->in.off, b->d_first_rev.p, b->d_pa.p};
        RG_TRY(T.run("k_strand_orient", [&] { return launch_strand_orient(oa, n, b->stream); }));
        a.reads = b->d_pa.p;
    }
    const int rc_a = path_driver_run(cx, a, cells);
    b->cells = cells[0];
    b->cells_performed = cells[1];
    if (rc_a || !(b->p.amb_mode & RG_AMB_BOTH_STRANDS)) return rc_a;
    // the qualifying reads once more, on the other strand, in the same work buffers
    const int recomb = b->p.mode == RG_MODE_RECOMBINATION || b->p.mode == RG_MODE_RECOMBINATION_SEMI ? 1 : 0;
    StrandGateArgs ga{b->d_rec.p, b->in.off, n, recomb, b->d_sidx.p, b->d_rcoff.p, b->d_ssum.p, vote ? b->d_first_rev.p : nullptr};
    if (b->p.mode == RG_MODE_PATHWISE_GAP_LOCAL_STRANDS) RG_TRY(T.run("k_gap_strands_gate", [&] { return launch_gap_strands_gate(ga, b->stream); }));
    else RG_TRY(T.run("k_strand_gate", [&] { return launch_strand_gate(ga, b->stream); }));
    RevcompArgs ra{a.reads, b->in.off, b->d_sidx.p, b->d_rcoff.p, b->d_ssum.p, b->d_rc.p};
    RG_TRY(T.run("k_revcomp", [&] { return launch_revcomp(ra, n, b->stream); }));
    HIPCHK(hipMemcpyAsync(b->h_ssum.p, b->d_ssum.p, 2 * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    RG_TRY(T.collect(b->stats));
    const int count = b->h_ssum.p[0], max_len = b->h_ssum.p[1];
    if (count <= 0) return RG_OK;
    if (count > n || max_len < 1 || max_len > b->max_n) return fail(RG_ERR_HIP, "k_strand_gate returned an impossible read count / length");
    HIPCHK(hipMemsetAsync(b->d_rcbad.p, 0, (size_t)count, b->stream));
    const PathJob rev{b->d_rc.p, b->d_rcoff.p, b->d_rcbad.p, count, max_len, b->d_rec2.p, b->d_ops2.p, b->ops_stride};
    RG_TRY(path_driver_run(cx, rev, cells));
    b->cells = cells[0];
    b->cells_performed = cells[1];
    StrandMergeArgs ma{b->d_rec.p, b->d_ops.p, b->d_rec2.p, b->d_ops2.p, b->ops_stride, b->d_sidx.p, count, recomb};
    RG_TRY(T.run("k_strand_merge", [&] { return launch_strand_merge(ma, b->stream); }));
    return T.collect(b->stats);
}
