// Pipeline driver of the pathwise modes (-m 4, -m 8): one pass (path_driver_run: a context and a job, rg_path_args.hpp) sizes
// the HBM work buffers, runs the kernel pipeline on the handle's stream in even chunks, timed by the handle's KernelTimer, and
// regrows the candidate lists on overflow.  The passes of a batch are put together by rg_strand_driver.hip.
//
//   -m 4:  sweep(F, dirs) -> seed -> layer(F) -> trace
//   -m 6:  gap_score(every path) -> gap_pick -> gap_dirs(picked path) -> gap_trace          (gap/rg_path_gap.hip; -m 7 likewise)
//   -m 12: the same four steps with the local kernels                                       (gap_local/rg_path_gap_local.hip)
//   the families of these three rules (rg_gap_modes.hpp):
//     long:     the same rules; a batch with a read over 2047 bases runs the striped kernels    (gap_long/rg_path_gap_long.hip)
//     xlong:    gap_score_long -> gap_pick -> gap_ckpt_long -> (gap_redo_long -> gap_walk_long) per stripe, last to first     (gap_xlong/rg_path_gap_xlong.hip)
//     strands:  two passes of the long family, each planned here by its own longest read (the passes: rg_strand_driver.hip)
//     xstrands: the pipeline of the xlong family in STAGES (PathJob::stage): PICK = gap_score[_long] -> gap_pick -> gap_pick_out, run per
//          strand; TRACE = gap_seed_pick -> the rest of the pipeline, run once (gap_xstrands/rg_gap_xstrands.hip; the stages of a batch:
//          rg_strand_driver.hip)
//   -m 44: edit_score(every path) -> gap_pick -> edit_dirs(picked path) -> edit_trace        (edit/rg_path_edit.hip; -m 45 likewise)
//   -m 94: the same up to 16383 bases; a batch with a longer read: edit_score_xlong -> gap_pick -> (edit_redo_xlong -> edit_walk_xlong)
//          per stripe, last to first                                                        (edit_xlong/rg_path_edit_xlong.hip; -m 95 likewise)
//   -m 64: edit_score_pair(every path, both strands in one wave) -> gap_pick(forward) -> gap_pick(reverse) -> edit_strands_duel
//          -> strand_orient(the strand that won) -> edit_dirs -> edit_trace -> gap_xstrands_mark   (edit_strands/rg_edit_strands.hip; -m 65 likewise)
//   -m 8:  sweep(F1: column maxima) -> seed -> thr -> sweep(R: dirs, candidates, column maxima)
//          -> thr -> sweep(F2: dirs, candidates) -> search -> layer(F) -> layer(R) -> trace
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gap/rg_path_gap.hpp"
#include "gap_local/rg_path_gap_local.hpp"
#include "gap_long/rg_path_gap_long.hpp"
#include "gap_xlong/rg_path_gap_xlong.hpp"
#include "gap_xstrands/rg_gap_xstrands.hpp"
#include "edit/rg_path_edit.hpp"
#include "edit_xlong/rg_path_edit_xlong.hpp"
#include "edit_strands/rg_edit_strands.hpp"
#include "rg_kernel_timer.hpp"
#include "rg_path_kernels.hpp"
#include "rg_path_plan.hpp"

namespace rg {

struct PathWorkImpl {
    bool tables = false;
    DevBuf<int> fpoff, fprow, fpslot, rpoff, rprow, rpslot;
    DevBuf<ReadState> state;
    DevBuf<int> roll, mf, wr, mfarg, wrarg, thr, flayer, rlayer;
    DevBuf<uint32_t> fdirs, rdirs, gdirs;
    DevBuf<int> gbnd, gdbnd;            // the long family: the stripe boundaries of the score pass and of the direction pass
    DevBuf<int> gckpt;                  // the xlong family: per stripe but the last, what it leaves to its right neighbour (picked path)
    DevBuf<GapWalkState> gwalk;         // ... and where each read's walk stands between two rounds
    DevBuf<unsigned long long> ebnd;    // -m 94 / -m 95: the boundary bits of every path's stripes but the last
    DevBuf<EditWalkState> ewalk;        // ... and where each read's walk stands between two rounds
    DevBuf<ReadState> state2;           // -m 64 / -m 65: the picks of the reverse strand
    DevBuf<uint8_t> oriented, strand;   // ... the chunk's reads on the strand that won, and which strand that is (1 = reverse)
    DevBuf<Cand> fcand, rcand;
    DevBuf<unsigned> nf, nr, ridx, nrec, nrrec;
    DevBuf<int> frec, rrec;
    unsigned frec_cap = 0, rrec_cap = 0;
    DevBuf<int> lb;
    DevBuf<int4> fsteps, rsteps;
    int nfsteps = 0, nrsteps = 0;
    DevBuf<int4> fsplit, rsplit;         // the same records with TAILs moved behind their register runs (rg_steps.cpp: split_tails)
    DevBuf<unsigned long long> flead, rlead, fslead, rslead;    // PATH RETIREMENT tables of the four step tables (rg_steps.cpp: lead_table)
    int retire_shift = RG_SWEEP16_RETIRE_SHIFT;              // the evaluation period the lead tables were built for
    unsigned long long fmembers = 0, rmembers = 0;           // member rows of the forward / reverse table (sum of the group sizes)
    unsigned fcap = 0, rcap = 0;
    DevBuf<unsigned> need;                 // [NEED_WORDS] per chunk: largest nf, nr, forward / reverse record count of a read (k_need); [4] reads whose
                                        // speculative bound failed (k_verify); [5] NEED_LAYER_FULL; [6], [7] NEED_SILENT_ROWS, NEED_RUN_ROWS; [8] .. [13] NEED_KEY_FOLDS .. NEED_KEY_SAVED_TAIL
    // speculative bound (PickArgs): 12-mer table of the paths, per-read pick, and what aligning the failed reads again needs
    DevBuf<uint32_t> kmer_keys;
    DevBuf<unsigned long long> kmer_masks;
    unsigned kmer_mask = 0;
    DevBuf<int> pick, pick2, order, rt_idx;
    DevBuf<uint8_t> rt_flags, rt_reads, rt_bad, rt_ops;
    DevBuf<long long> rt_off;
    DevBuf<DevRecord> rt_rec;
    DevBuf<unsigned long long> rt_cells;
    PathWork retry;                     // work buffers of that second pass (a handful of reads)
    unsigned long long* h_sum = nullptr;  // pinned: {cell updates of the chunk, need[0 .. NEED_WORDS - 1], cell updates performed} read back once per chunk
    ~PathWorkImpl() { if (h_sum) (void)hipHostFree(h_sum); }
};
PathWork::~PathWork() { delete impl; }

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One call of path_driver_run: what it was given, the plan, and the chunk in flight (reads [done, done + chunk)).
struct Run {
    const HostGraph& h;
    const PathGraphDev& gd;
    const rg_params& p;
    PathWorkImpl& w;
    const PathPlan& plan;
    const uint8_t* d_reads;
    const long long* d_off;
    const uint8_t* d_bad;
    int max_n;
    DevRecord* d_rec;
    uint8_t* d_ops;
    long long ops_stride;
    unsigned long long* d_cells;
    hipStream_t stream;
    KernelStats& stats;
    int spec_level;
    KernelTimer& T;
    bool debug;
    int done = 0, chunk = 0;
    hipError_t async_err = hipSuccess;       // of calls inside timed launches: reported once the chunk is through
    DevScores sc{};
    const long long* h_off = nullptr;        // PathJob::h_off

    const long long* off() const { return d_off + done; }
    const uint8_t* bad() const { return d_bad + done; }
    const unsigned* need() const { return reinterpret_cast<const unsigned*>(w.h_sum + 1); }
    unsigned nretry() const { return (plan.spec || plan.spec4) ? need()[4] : 0u; }

    int alloc_chunk(bool* oom);
    int enqueue_chunk();
    SweepArgs sweep_args() const;
    GapArgs gap_args() const;
    const char* sweep(const SweepArgs& sa);     // (what it launched, like the launchers: rg_launch_log.hpp)
    int enqueue_pathwise(const SweepArgs& sa, const SeedArgs& se);
    int enqueue_pathwise_gap();
    int enqueue_pathwise_edit();
    int enqueue_pathwise_edit_xlong();
    int enqueue_pathwise_edit_strands();
    int read_back();
    int enqueue_recombination(SweepArgs& sa, const SeedArgs& se);
    int enqueue_forward_bounded(SweepArgs& sa, const SeedArgs& se);
    int check_opt0_16(const Opt0Args& oa);
    int enqueue_tail();
    int regrow_lists(bool& redo);
    int dump_list_stats();
    int dump_spec4_retries();
    int dump_dsel_retries();
    int second_pass(unsigned long long& cells_perf);
};

// per-graph tables of a handle, uploaded once: rows of every path, the 12-mer vote table, the step tables of the sweeps
int ensure_tables(const HostGraph& h, PathWorkImpl& w) {
    if (w.tables) return RG_OK;
    int rc;
    std::vector<int> po, pr, ps;
    build_path_rows(h, true, po, pr, ps);
    if ((rc = w.fpoff.upload(po)) || (rc = w.fprow.upload(pr)) || (rc = w.fpslot.upload(ps))) return rc;
    {
        std::vector<uint32_t> keys;
        std::vector<unsigned long long> masks;
        build_kmer_table(h, po, pr, keys, masks);
        if ((rc = w.kmer_keys.upload(keys)) || (rc = w.kmer_masks.upload(masks))) return rc;
        w.kmer_mask = (unsigned)(keys.size() - 1);
    }
    build_path_rows(h, false, po, pr, ps);
    if ((rc = w.rpoff.upload(po)) || (rc = w.rprow.upload(pr)) || (rc = w.rpslot.upload(ps))) return rc;
    // step tables of the sweeps (record layout documented in k_sweep)
    if (h.L >= (1 << 20) || h.fslots >= (1 << 20) || h.rslots >= (1 << 20)) return fail(RG_ERR_GRAPH, "graph too large for the sweep step table");
    // (built on the host by rg_steps.cpp: plain and split tables, the path-retirement tables of either, the member count; the
    // split table: up to 64 paths TAILs behind their register runs, more: the wide-run table)
    StepTables st;
    build_step_tables(h, true, true, st);
    if ((rc = w.fsteps.upload(st.plain)) || (rc = w.flead.upload(st.lead_plain)) || (rc = w.fsplit.upload(st.split)) ||
        (rc = w.fslead.upload(st.lead_split)))
        return rc;
    w.nfsteps = (int)st.plain.size();
    w.fmembers = st.members;
    w.retire_shift = st.retire_shift;
    build_step_tables(h, false, true, st);
    if ((rc = w.rsteps.upload(st.plain)) || (rc = w.rlead.upload(st.lead_plain)) || (rc = w.rsplit.upload(st.split)) ||
        (rc = w.rslead.upload(st.lead_split)))
        return rc;
    w.nrsteps = (int)st.plain.size();
    w.rmembers = st.members;
    w.tables = true;
    return RG_OK;
}

// work buffers of `chunk` reads; *oom: hipMalloc ran out of memory (the caller halves the chunk)
int Run::alloc_chunk(bool* oom) {
    const size_t n = (size_t)chunk, wpad = (size_t)plan.wpad;
    int rc;
    if (plan.edit) {
        if ((rc = w.state.alloc(n, oom)) || (rc = w.gdirs.alloc(n * (size_t)plan.gdirs_stride, oom))) return rc;
        if (plan.edit_strands && ((rc = w.state2.alloc(n, oom)) || (rc = w.oriented.alloc(n * plan.edit_orient_bytes + 64, oom)) || (rc = w.strand.alloc(n, oom)))) return rc;
        if (plan.edit_xlong && ((rc = w.ebnd.alloc(n * (size_t)plan.edit_bnd_stride, oom)) || (rc = w.ewalk.alloc(n, oom)))) return rc;
        return RG_OK;
    }
    if (plan.gap) {
        // (a stage allocates what its kernels touch: plan_gap_stage counted the same buffers)
        const bool score = plan.stage != PATH_STAGE_TRACE, trace = plan.stage != PATH_STAGE_PICK;
        if ((rc = w.state.alloc(n, oom)) || (trace && (rc = w.gdirs.alloc(n * (size_t)plan.gdirs_stride, oom)))) return rc;
        if (plan.gap_xlong) {
            if (score && (rc = w.gbnd.alloc(n * (size_t)plan.gbnd_stride, oom))) return rc;
            if (trace && ((rc = w.gckpt.alloc(n * (size_t)plan.gckpt_stride, oom)) || (rc = w.gwalk.alloc(n, oom)))) return rc;
            return RG_OK;
        }
        if (plan.nwv > 1 && ((rc = w.gbnd.alloc(n * (size_t)plan.gbnd_stride, oom)) || (rc = w.gdbnd.alloc(n * (size_t)plan.gdbnd_stride, oom)))) return rc;
        return RG_OK;
    }
    if ((rc = w.state.alloc(n, oom)) || (rc = w.fdirs.alloc(n * plan.fdirs_stride, oom)) || (rc = w.flayer.alloc(n * plan.layer_stride, oom)) ||
        (rc = w.roll.alloc(n * (h.P + 2) * wpad, oom)))
        return rc;
    if (plan.mode == RG_MODE_RECOMBINATION) {
        if ((rc = w.rdirs.alloc(n * plan.rdirs_stride, oom)) || (rc = w.rlayer.alloc(n * plan.layer_stride, oom)) ||
            (rc = w.mf.alloc(n * wpad, oom)) || (rc = w.wr.alloc(n * wpad, oom)) || (rc = w.mfarg.alloc(n * wpad, oom)) ||
            (rc = w.wrarg.alloc(n * wpad, oom)) || (rc = w.thr.alloc(n * wpad, oom)) || (rc = w.fcand.alloc(n * w.fcap, oom)) ||
            (rc = w.rcand.alloc(n * w.rcap, oom)) || (rc = w.ridx.alloc(n * w.rcap, oom)) || (rc = w.nf.alloc(n, oom)) ||
            (rc = w.nr.alloc(n, oom)) || (rc = w.lb.alloc(n, oom)) || (rc = w.nrec.alloc(n, oom)))
            return rc;
        if (plan.spec && ((rc = w.pick.alloc(n, oom)) || (rc = w.pick2.alloc(n * 2, oom)) || (rc = w.order.alloc(n, oom)) || (rc = w.rt_flags.alloc(n, oom))))
            return rc;
        if (plan.use_rec && ((rc = w.frec.alloc(n * w.frec_cap * plan.recw, oom)) || (rc = w.rrec.alloc(n * w.rrec_cap * plan.recw, oom)) ||
                             (rc = w.nrrec.alloc(n, oom))))
            return rc;
    }
    if (plan.spec4 && ((rc = w.lb.alloc(n, oom)) || (rc = w.pick.alloc(n, oom)) || (rc = w.order.alloc(n, oom)) || (rc = w.rt_flags.alloc(n, oom))))
        return rc;
    return RG_OK;
}

// what every sweep of the chunk shares
SweepArgs Run::sweep_args() const {
    SweepArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.g = gd;
    sa.sc = sc;
    sa.reads = d_reads; sa.read_off = off(); sa.bad = bad(); sa.state = w.state.p; sa.roll = w.roll.p;
    sa.fsteps = w.fsteps.p; sa.rsteps = w.rsteps.p; sa.nfsteps = w.nfsteps; sa.nrsteps = w.nrsteps;
    sa.semi = plan.semi ? 1 : 0;
    sa.nwv = plan.nwv;
    sa.gather_ok = plan.gather_ok ? 1 : 0;
    sa.fsplit = w.fsplit.p; sa.rsplit = w.rsplit.p;
    sa.use_split = plan.use_split ? 1 : 0;
    sa.flead = w.flead.p; sa.rlead = w.rlead.p; sa.fslead = w.fslead.p; sa.rslead = w.rslead.p;
    sa.retire = plan.retire ? 1 : 0;
    sa.retire_shift = w.retire_shift;
    sa.fmembers = w.fmembers; sa.rmembers = w.rmembers;
    sa.maxmatch = plan.maxmatch;      // (both sweeps: the retirement bound; the forward sweep's speculative thresholds)
    sa.dsel_pick = plan.dsel ? w.pick.p : nullptr; sa.dsel_pick2 = plan.dsel && plan.pick_two ? w.pick2.p : nullptr;
    sa.dsel_lo = plan.dsel_lo; sa.dsel_hi = plan.dsel_hi;
    sa.rbw = p.rec_band_width; sa.cand_cap = 0; sa.dir_words = plan.dir_words; sa.cells = d_cells;
    sa.runstat = w.need.p + NEED_SILENT_ROWS;
    return sa;
}

// what the kernels of the affine-gap and edit-distance families take of the chunk (the edit kernels read neither o nor e)
GapArgs Run::gap_args() const {
    GapArgs ga;
    memset(&ga, 0, sizeof ga);
    ga.sc = sc; ga.lnz = gd.lnz; ga.reads = d_reads; ga.read_off = off(); ga.bad = bad(); ga.poff = w.fpoff.p; ga.prow = w.fprow.p;
    ga.P = h.P; ga.o = p.gap_open; ga.e = p.gap_ext; ga.state = w.state.p; ga.dirs = w.gdirs.p; ga.dirs_stride = plan.gdirs_stride;
    ga.cells = d_cells; ga.rec = d_rec + done; ga.ops = d_ops ? d_ops + (long long)done * ops_stride : nullptr; ga.ops_stride = ops_stride;
    return ga;
}

const char* Run::sweep(const SweepArgs& sa) {
    // (striped sweeps advance the candidate counter of a read atomically from several waves: start it at zero)
    if (plan.nwv > 1 && sa.cand && sa.ncand_out) {
        const hipError_t e = hipMemsetAsync(sa.ncand_out, 0, sizeof(unsigned) * chunk, stream);
        if (e != hipSuccess) async_err = e;
    }
    return plan.use16 ? launch_sweep16(sa, chunk, plan.C, stream) : launch_sweep(sa, chunk, plan.C, stream);
}

// -m 4 / -m 5:  [pick -> opt0 ->] sweep(F, dirs) -> seed [-> verify4]
int Run::enqueue_pathwise(const SweepArgs& sa, const SeedArgs& se) {
    SweepArgs f = sa;
    f.rev = 0; f.track_best = 0; f.dirs = w.fdirs.p; f.dirs_stride = plan.fdirs_stride; f.count_cells = 1;
    f.retire = 0;
    if (plan.spec4) {
        PickArgs pa{d_reads, off(), bad(), w.kmer_keys.p, w.kmer_masks.p, w.kmer_mask, h.P, w.pick.p, w.fpoff.p, w.fprow.p, nullptr};
        RG_TRY(T.run("k_pick", [&] { return launch_pick(pa, chunk, stream); }));
        Opt0Args oa{gd, sc, d_reads, off(), bad(), w.fpoff.p, w.fprow.p, w.lb.p, 0, w.pick.p, plan.spec4_margin, plan.nwv, nullptr, 0};
        RG_TRY(T.run("k_opt0", [&] { return launch_opt0_16(oa, chunk, plan.C, stream); }));
        if (plan.retire4) {
            f.retire = 1; f.lb = w.lb.p; f.maxmatch = plan.maxmatch;
            if (plan.order) { RG_TRY(T.inst(launch_order(w.pick.p, nullptr, w.order.p, chunk, stream))); f.order = w.order.p; }
        }
        if (plan.dsel4) { f.dsel_pick = w.pick.p; f.dsel_pick2 = nullptr; f.dsel_lo = 0; f.dsel_hi = h.L; }     // (no recombination: no edge rows)
    }
    RG_TRY(T.run(plan.use16 ? "k_sweep16_fwd" : "k_sweep_fwd", [&] { return sweep(f); }));
    RG_TRY(T.run("k_seed", [&] { return launch_seed(se, stream); }));
    if (plan.spec4) RG_TRY(T.inst(launch_verify4(w.state.p, w.lb.p, w.need.p + 4, w.rt_flags.p, chunk, f.dsel_pick, stream)));
    return RG_OK;
}

// -m 6 / -m 7 / -m 12:  gap_score(every path) -> gap_pick -> gap_dirs(picked path) -> gap_trace -> the chunk's one read-back
int Run::enqueue_pathwise_gap() {
    const GapArgs ga = gap_args();
    const int C = plan.C;
    const bool semi = plan.semi, local = plan.local;
    const int kind = local ? GAP_LOCAL : semi ? GAP_SEMI : GAP_GLOBAL;
    // a step whose local kind has a kernel of its own: (label, launch) of the global / semi kinds, then of the local kind
    auto step = [&](const char* name, auto&& launch, const char* name_local, auto&& launch_local) {
        return local ? T.run(name_local, launch_local) : T.run(name, launch);
    };
    // (the pick kernels are the base modes' in every pipeline: a striped batch tells them the striped width)
    auto pick = [&] {
        return step("k_gap_pick", [&] { return launch_gap_pick(ga, chunk, plan.nwv * C, semi, stream); },
                    "k_gap_pick_local", [&] { return launch_gap_pick_local(ga, chunk, plan.nwv * C, stream); });
    };
    // the stages of the xstrands family: a PICK stage ends behind the pick, which goes out into the job's records; a TRACE stage
    // begins there, with the picks of the records (the whole pipeline runs score, pick and the rest without either)
    const bool score = plan.stage != PATH_STAGE_TRACE;
    auto pick_out = [&] {
        RG_TRY(T.run("k_gap_pick_out", [&] { return launch_gap_pick_out(w.state.p, ga.rec, chunk, stream); }));
        return read_back();
    };
    auto seed_pick = [&] { return T.run("k_gap_seed_pick", [&] { return launch_gap_seed_pick(ga.rec, w.state.p, chunk, stream); }); };
    if (plan.nwv == 1) {
        // single wave: the whole row in one wave's registers
        if (score) {
            RG_TRY(step("k_gap_score", [&] { return launch_gap_score(ga, chunk, C, semi, stream); },
                        "k_gap_score_local", [&] { return launch_gap_score_local(ga, chunk, C, stream); }));
            RG_TRY(pick());
        }
        if (plan.stage == PATH_STAGE_PICK) return pick_out();
        if (plan.stage == PATH_STAGE_TRACE) RG_TRY(seed_pick());
        RG_TRY(step("k_gap_dirs", [&] { return launch_gap_dirs(ga, chunk, C, semi, stream); },
                    "k_gap_dirs_local", [&] { return launch_gap_dirs_local(ga, chunk, C, stream); }));
        RG_TRY(step("k_gap_trace", [&] { return launch_gap_trace(ga, chunk, C, semi, stream); },
                    "k_gap_trace_local", [&] { return launch_gap_trace_local(ga, chunk, C, stream); }));
        return read_back();
    }
    // column stripes (a long mode with a read over 2047 bases); with checkpoints (gap_xlong) the score pass is the same, its stripe cap lifted
    GapLongArgs la;
    memset(&la, 0, sizeof la);
    la.g = ga; la.S = plan.nwv; la.rows1 = h.max_path_rows + 1;
    la.bnd = score ? w.gbnd.p : nullptr; la.bnd_stride = plan.gbnd_stride; la.dbnd = plan.gap_xlong ? nullptr : w.gdbnd.p;
    if (score) {
        RG_TRY(T.run("k_gap_score_long", [&] { return launch_gap_score_long(la, chunk, kind, stream, plan.gap_xlong ? GAP_XLONG_MAX_STRIPES : GAP_LONG_MAX_STRIPES); }));
        RG_TRY(pick());
    }
    if (plan.stage == PATH_STAGE_PICK) return pick_out();
    if (plan.stage == PATH_STAGE_TRACE) RG_TRY(seed_pick());
    if (!plan.gap_xlong) {
        // striped: the direction words of every stripe, one walk
        RG_TRY(T.run("k_gap_dirs_long", [&] { return launch_gap_dirs_long(la, chunk, kind, stream); }));
        RG_TRY(T.run(local ? "k_gap_trace_local_long" : "k_gap_trace_long", [&] { return launch_gap_trace_long(la, chunk, kind, stream); }));
        return read_back();
    }
    // striped with checkpoints: one stripe of direction words: checkpoints first, then per stripe, last to first, the rebuild and the
    // walk (no read-back in between: a read whose walk is elsewhere returns at once)
    static_assert(sizeof(GapWalkState) == 32, "the plan counts 32 bytes of walk state per read");
    GapXLongArgs xa;
    memset(&xa, 0, sizeof xa);
    xa.l = la; xa.ckpt = w.gckpt.p; xa.ckpt_stride = plan.gckpt_stride; xa.walk = w.gwalk.p;
    RG_TRY(T.run("k_gap_ckpt_long", [&] { return launch_gap_ckpt_long(xa, chunk, kind, stream); }));
    for (int round = plan.nwv - 1; round >= 0; --round) {
        RG_TRY(T.run("k_gap_redo_long", [&] { return launch_gap_redo_long(xa, chunk, kind, round, stream); }));
        RG_TRY(T.run(local ? "k_gap_walk_local_long" : "k_gap_walk_long", [&] { return launch_gap_walk_long(xa, chunk, kind, round, stream); }));
    }
    return read_back();
}

// -m 44 / -m 45:  edit_score(every path) -> gap_pick -> edit_dirs(picked path) -> edit_trace -> the chunk's one read-back
int Run::enqueue_pathwise_edit() {
    const GapArgs ga = gap_args();
    const int W = plan.edit_words;
    const bool semi = plan.semi;
    RG_TRY(T.run("k_edit_score", [&] { return launch_edit_score(ga, chunk, W, semi, stream); }));
    // (the pick kernel of modes 6 / 7 refuses a read of more than its width - 1 bases, a width it takes in 64s: 4096 W covers the
    // 2048 W bases of a lane layout that has no column 0; the direction pass reports a read beyond those itself)
    RG_TRY(T.run("k_gap_pick", [&] { return launch_gap_pick(ga, chunk, 64 * W, semi, stream); }));
    RG_TRY(T.run("k_edit_dirs", [&] { return launch_edit_dirs(ga, chunk, W, semi, stream); }));
    RG_TRY(T.run("k_edit_trace", [&] { return launch_edit_trace(ga, chunk, W, semi, stream); }));
    return read_back();
}

// -m 64 / -m 65:  edit_score_pair(every path, both strands) -> gap_pick x 2 -> duel -> strand_orient -> edit_dirs -> edit_trace -> mark
// -> the chunk's one read-back.  No host synchronisation in between: the score decides the strand on the device, and the one strand
// that won is traced, from a buffer that holds the chunk's reads on that strand at the input's offsets minus the chunk's first
int Run::enqueue_pathwise_edit_strands() {
    if (!h_off) return fail(RG_ERR_ARG, "the both-strands edit-distance modes need the read offsets on the host");
    HIPCHK(hipMemsetAsync(w.state2.p, 0, sizeof(ReadState) * chunk, stream));
    GapArgs ga = gap_args();
    const int W = plan.edit_words, Wp = plan.edit_pair_words;
    const bool semi = plan.semi;
    RG_TRY(T.run("k_edit_score_pair", [&] { return launch_edit_score_pair(ga, w.state2.p, chunk, Wp, semi, stream); }));
    // (the pick kernel's width as in enqueue_pathwise_edit; the same reads, offsets and bad flags for either strand)
    GapArgs gr = ga;
    gr.state = w.state2.p;
    RG_TRY(T.run("k_gap_pick", [&] { return launch_gap_pick(ga, chunk, 64 * W, semi, stream); }));
    RG_TRY(T.run("k_gap_pick", [&] { return launch_gap_pick(gr, chunk, 64 * W, semi, stream); }));
    RG_TRY(T.run("k_edit_strands_duel", [&] { return launch_edit_strands_duel(w.state.p, w.state2.p, w.strand.p, chunk, stream); }));
    // (k_strand_orient and the edit kernels address a read as base + offset: the base that puts the chunk's first read at the buffer's start)
    uint8_t* obase = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(w.oriented.p) - (uintptr_t)h_off[done]);
    StrandOrientArgs oa{d_reads, off(), w.strand.p, obase};
    RG_TRY(T.run("k_strand_orient", [&] { return launch_strand_orient(oa, chunk, stream); }));
    ga.reads = obase;
    RG_TRY(T.run("k_edit_dirs", [&] { return launch_edit_dirs(ga, chunk, W, semi, stream); }));
    RG_TRY(T.run("k_edit_trace", [&] { return launch_edit_trace(ga, chunk, W, semi, stream); }));
    // (the walk's record writer clears DevRecord.pad)
    RG_TRY(T.run("k_gap_xstrands_mark", [&] { return launch_gap_xstrands_mark(ga.rec, w.strand.p, chunk, stream); }));
    return read_back();
}

// -m 94 / -m 95 with a read over 16383 bases:  edit_score_xlong(every path) -> gap_pick -> per stripe, last to first, the rebuild and
// the walk (no read-back in between: a read whose walk is elsewhere returns at once) -> the chunk's one read-back
int Run::enqueue_pathwise_edit_xlong() {
    static_assert(sizeof(EditWalkState) == 32, "the plan counts 32 bytes of walk state per read");
    EditXLongArgs xa;
    memset(&xa, 0, sizeof xa);
    xa.g = gap_args(); xa.S = plan.nwv; xa.rows1 = h.max_path_rows + 1;
    xa.bnd = w.ebnd.p; xa.bnd_stride = plan.edit_bnd_stride; xa.slot_words = plan.edit_slot_words; xa.walk = w.ewalk.p;
    const bool semi = plan.semi;
    RG_TRY(T.run("k_edit_score_xlong", [&] { return launch_edit_score_xlong(xa, chunk, semi, stream); }));
    // (the pick kernel's width, in 64s: above the 16384 S bases of a lane layout that has no column 0, as in enqueue_pathwise_edit)
    RG_TRY(T.run("k_gap_pick", [&] { return launch_gap_pick(xa.g, chunk, 64 * EDIT_MAX_WORDS * plan.nwv, semi, stream); }));
    for (int round = plan.nwv - 1; round >= 0; --round) {
        RG_TRY(T.run("k_edit_redo_xlong", [&] { return launch_edit_redo_xlong(xa, chunk, semi, round, stream); }));
        RG_TRY(T.run("k_edit_walk_xlong", [&] { return launch_edit_walk_xlong(xa, chunk, semi, round, stream); }));
    }
    return read_back();
}

// RG_DEBUG: the i32 form of k_opt0 beside the packed one — the two must agree on every read (the bound only steers the pruning,
// so no parity test would notice a wrong one: tests/test_gpu_pathwise.py runs this check)
int Run::check_opt0_16(const Opt0Args& oa) {
    std::vector<int> h16(chunk), h32(chunk);
    HIPCHK(hipMemcpyAsync(h16.data(), w.lb.p, sizeof(int) * chunk, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    RG_TRY(T.inst(launch_opt0(oa, chunk, plan.C, stream)));
    HIPCHK(hipMemcpyAsync(h32.data(), w.lb.p, sizeof(int) * chunk, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int k = 0; k < chunk; ++k)
        if (h16[k] != h32[k]) return fail(RG_ERR_HIP, "k_opt0_16 differs from k_opt0 at read " + std::to_string(k) + ": " + std::to_string(h16[k]) + " vs " + std::to_string(h32[k]));
    return RG_OK;
}

// two-sweep -m 8, first half:  [pick ->] opt0 -> sweep(F: dirs, loose candidates / records) [-> colmax_rec] -> seed
// (sa.order is set here for the reverse sweep as well)
int Run::enqueue_forward_bounded(SweepArgs& sa, const SeedArgs& se) {
    Opt0Args oa{gd, sc, d_reads, off(), bad(), w.fpoff.p, w.fprow.p, w.lb.p, plan.semi ? 1 : 0, nullptr, 0, plan.nwv, nullptr, 0};
    if (plan.spec) {
        PickArgs pa{d_reads, off(), bad(), w.kmer_keys.p, w.kmer_masks.p, w.kmer_mask, h.P, w.pick.p, w.fpoff.p, w.fprow.p,
                    plan.pick_two ? w.pick2.p : nullptr};
        oa.pick2 = pa.pick2;
        oa.rec_pen = plan.rec_pen;
        RG_TRY(T.run("k_pick", [&] { return launch_pick(pa, chunk, stream); }));
        if (plan.retire && plan.order) {
            RG_TRY(T.inst(launch_order(w.pick.p, pa.pick2, w.order.p, chunk, stream)));
            sa.order = w.order.p;
        }
        oa.pick = w.pick.p;
        oa.margin = plan.spec_margin;
    }
    RG_TRY(T.run("k_opt0", [&] { return plan.opt16 ? launch_opt0_16(oa, chunk, plan.C, stream) : launch_opt0(oa, chunk, plan.C, stream); }));
    if (plan.opt16 && debug) {
        const int rc = check_opt0_16(oa);
        if (rc) return rc;
    }
    SweepArgs f = sa;
    f.rev = 0; f.track_best = 1; f.lb = w.lb.p; f.brc = p.base_rec_cost; f.maxmatch = plan.maxmatch;
    f.oob = plan.spec ? 1 : 0;        // tight thresholds: most rows emit nothing (row_end tests the lane maximum first)
    f.colmax_out = w.mf.p; f.colarg_out = w.mfarg.p; f.cand = w.fcand.p; f.cand_cap = w.fcap; f.ncand_out = w.nf.p;
    if (plan.use_rec) {
        // records, and NO column maxima in the sweep (round 5: k_sweep16<.., 0, ..>, the reverse sweep's variant).  What
        // the reverse thresholds and k_expand need per column is the best forward cell that can be a CANDIDATE — a
        // usable cell at or above the forward emission threshold — and every such cell is in the records:
        // k_colmax_rec reads maxima and cells out of them right behind the sweep (columns without a record get
        // "no partner": no reverse emission there at all).  Round 4 tracked packed maxima of ALL cells in the sweep
        // (8 registers, 8 v_pk_max per row) for an upper bound of the same quantity.
        f.cand = nullptr; f.cand_cap = 0; f.frec = w.frec.p; f.frec_cap = w.frec_cap; f.ncand_out = w.nrec.p;
        f.colmax_out = nullptr; f.colarg_out = nullptr;
    }
    f.dirs = w.fdirs.p; f.dirs_stride = plan.fdirs_stride; f.count_cells = 1;
    f.retire = plan.retire_fwd ? 1 : 0;
    RG_TRY(T.run(plan.use16 ? "k_sweep16_fwd" : "k_sweep_fwd", [&] { return sweep(f); }));
    if (plan.use_rec) {
        ExpandArgs fc{w.state.p, w.frec.p, w.frec_cap, w.nrec.p, nullptr, 0, nullptr, nullptr, plan.wpad, p.base_rec_cost, gd.knm, 0, off(),
                      p.rec_band_width, p.scores[5]};
        RG_TRY(T.run("k_colmax_rec_fwd", [&] { return launch_colmax_rec(fc, w.mf.p, w.mfarg.p, chunk, plan.C, stream); }));
    }
    RG_TRY(T.run("k_seed", [&] { return launch_seed(se, stream); }));
    return RG_OK;
}

// -m 8 / -m 9, two sweeps:   (forward half above) -> thr -> sweep(R: dirs, candidates, column maxima) -> bound -> [expand x 2] -> search
//              three sweeps: sweep(F1: column maxima) -> seed -> thr -> sweep(R) -> bound -> thr -> sweep(F2: dirs, candidates) -> search
int Run::enqueue_recombination(SweepArgs& sa, const SeedArgs& se) {
    const int wpad = plan.wpad;
    if (plan.two_sweep) {
        const int rc = enqueue_forward_bounded(sa, se);
        if (rc) return rc;
    } else {
        SweepArgs f1 = sa;
        f1.rev = 0; f1.track_best = 1; f1.colmax_out = w.mf.p; f1.colarg_out = w.mfarg.p; f1.count_cells = 0;
        RG_TRY(T.run(plan.use16 ? "k_sweep16_fwd_colmax" : "k_sweep_fwd_colmax", [&] { return sweep(f1); }));
        RG_TRY(T.run("k_seed", [&] { return launch_seed(se, stream); }));
    }
    ThrArgs t1{w.state.p, w.mf.p, w.thr.p, wpad, p.base_rec_cost, 0, plan.two_sweep ? w.lb.p : nullptr};
    RG_TRY(T.run("k_threshold", [&] { return launch_threshold(t1, chunk, stream); }));
    SweepArgs r = sa;
    r.rev = 1; r.track_best = 1; r.thr = w.thr.p; r.colmax_out = w.wr.p; r.colarg_out = w.wrarg.p; r.cand = w.rcand.p; r.cand_cap = w.rcap; r.ncand_out = w.nr.p;
    if (plan.use_rec) {
        // records instead of Cand entries; the reverse column maxima come from those records (k_colmax_rec)
        r.cand = nullptr; r.cand_cap = 0; r.frec = w.rrec.p; r.frec_cap = w.rrec_cap; r.ncand_out = w.nrrec.p;
        r.colmax_out = nullptr; r.colarg_out = nullptr;
    }
    r.dirs = w.rdirs.p; r.dirs_stride = plan.rdirs_stride; r.count_cells = 1;
    r.retire = plan.retire_rev ? 1 : 0;
    RG_TRY(T.run(plan.use16 ? "k_sweep16_rev" : "k_sweep_rev", [&] { return sweep(r); }));
    if (plan.use_rec) {
        ExpandArgs ec{w.state.p, w.rrec.p, w.rrec_cap, w.nrrec.p, nullptr, 0, nullptr, nullptr, wpad, p.base_rec_cost, gd.knm, 1, off(),
                      p.rec_band_width, p.scores[5]};
        RG_TRY(T.run("k_colmax_rec", [&] { return launch_colmax_rec(ec, w.wr.p, w.wrarg.p, chunk, plan.C, stream); }));
    }
    BoundArgs ba{gd, w.state.p, off(), w.mf.p, w.mfarg.p, w.wr.p, w.wrarg.p, wpad, p.base_rec_cost, p.multi_rec_cost, p.rec_band_width};
    RG_TRY(T.run("k_bound", [&] { return launch_bound(ba, chunk, stream); }));
    if (!plan.two_sweep) {
        ThrArgs t2{w.state.p, w.wr.p, w.thr.p, wpad, p.base_rec_cost, 1, nullptr};
        RG_TRY(T.run("k_threshold", [&] { return launch_threshold(t2, chunk, stream); }));
        SweepArgs f2 = sa;
        f2.rev = 0; f2.track_best = 1; f2.thr = w.thr.p; f2.cand = w.fcand.p; f2.cand_cap = w.fcap; f2.ncand_out = w.nf.p;
        f2.dirs = w.fdirs.p; f2.dirs_stride = plan.fdirs_stride; f2.count_cells = 1;
        RG_TRY(T.run(plan.use16 ? "k_sweep16_fwd" : "k_sweep_fwd", [&] { return sweep(f2); }));
    }
    if (plan.use_rec) {
        HIPCHK(hipMemsetAsync(w.nf.p, 0, sizeof(unsigned) * chunk, stream));
        HIPCHK(hipMemsetAsync(w.nr.p, 0, sizeof(unsigned) * chunk, stream));
        ExpandArgs ea{w.state.p, w.frec.p, w.frec_cap, w.nrec.p, w.fcand.p, w.fcap, w.nf.p, w.wr.p, wpad, p.base_rec_cost, gd.knm, 0, off(), p.rec_band_width, p.scores[5]};
        RG_TRY(T.run("k_expand", [&] { return launch_expand(ea, chunk, plan.C, stream); }));
        ExpandArgs er{w.state.p, w.rrec.p, w.rrec_cap, w.nrrec.p, w.rcand.p, w.rcap, w.nr.p, w.mf.p, wpad, p.base_rec_cost, gd.knm, 1, off(), p.rec_band_width, p.scores[5]};
        RG_TRY(T.run("k_expand", [&] { return launch_expand(er, chunk, plan.C, stream); }));
    }
    SearchArgs sr{gd, w.state.p, w.fcand.p, w.rcand.p, w.nf.p, w.nr.p, w.ridx.p, w.fcap, w.rcap, w.wr.p, wpad, p.base_rec_cost, p.multi_rec_cost};
    RG_TRY(T.run("k_search", [&] { return launch_search(sr, chunk, stream); }));
    // largest list / record counts of the chunk, read back once after the traceback (no host round trip here)
    RG_TRY(T.inst(launch_need(w.state.p, w.nf.p, w.nr.p, plan.use_rec ? w.nrec.p : nullptr, plan.use_rec ? w.nrrec.p : nullptr, w.need.p, chunk, stream)));
    if (plan.spec) RG_TRY(T.inst(launch_verify(w.state.p, w.lb.p, w.need.p + 4, w.rt_flags.p, chunk, sa.dsel_pick, sa.dsel_pick2, sa.dsel_lo, sa.dsel_hi, stream)));
    return RG_OK;
}

// every mode:  layer(F) [-> layer(R)] -> trace -> the chunk's one read-back
int Run::enqueue_tail() {
    const int C = plan.C;
    LayerArgs la;
    memset(&la, 0, sizeof la);
    la.semi = plan.semi ? 1 : 0;
    la.nwv = plan.nwv;
    la.g = gd; la.sc = sc; la.reads = d_reads; la.read_off = off(); la.state = w.state.p; la.dir_words = plan.dir_words; la.dir_fmt = plan.use16 ? 1 : 0;
    la.layer_stride = plan.layer_stride; la.fpoff = w.fpoff.p; la.fprow = w.fprow.p; la.fpslot = w.fpslot.p;
    la.rpoff = w.rpoff.p; la.rprow = w.rprow.p; la.rpslot = w.rpslot.p;
    la.rev = 0; la.dirs = w.fdirs.p; la.dirs_stride = plan.fdirs_stride; la.layer = w.flayer.p;
    // (windowed: layer_window/rg_layer_window.hip rebuilds W columns of every row around the walk)
    const int win = plan.layer_window;
    auto layer = [&]() {
        if (win) return launch_layer_window(la, chunk, C, win, stream);
        return plan.layer16 ? launch_layer16(la, chunk, C, stream) : launch_layer(la, chunk, C, stream);
    };
    auto fwd_side = [&]() { la.rev = 0; la.dirs = w.fdirs.p; la.dirs_stride = plan.fdirs_stride; la.layer = w.flayer.p; };
    auto rev_side = [&]() { la.rev = 1; la.dirs = w.rdirs.p; la.dirs_stride = plan.rdirs_stride; la.layer = w.rlayer.p; };
    // (which windowed kernel ran: a pseudo-statistic of its own, always on, read by tests/test_gpu_layer_window.py)
    const char* family = win ? LAYER_WINDOW_LOG : "inst:";
    RG_TRY(T.run("k_layer_fwd", layer, family, win != 0));
    if (plan.mode == RG_MODE_RECOMBINATION) {
        rev_side();
        RG_TRY(T.run("k_layer_rev", layer, family, win != 0));
    }
    TraceArgs ta;
    memset(&ta, 0, sizeof ta);
    ta.g = gd; ta.sc = sc; ta.reads = d_reads; ta.read_off = off(); ta.state = w.state.p; ta.rec = d_rec + done;
    ta.ops = d_ops + (long long)done * ops_stride; ta.ops_stride = ops_stride; ta.flayer = w.flayer.p;
    ta.rlayer = w.rlayer.p; ta.layer_stride = plan.layer_stride; ta.fpoff = w.fpoff.p; ta.fprow = w.fprow.p;
    ta.rpoff = w.rpoff.p; ta.rprow = w.rprow.p; ta.nreads = chunk; ta.mode = p.mode; ta.semi = plan.semi ? 1 : 0; ta.nwv = plan.nwv;
    ta.window = win; ta.nfull = w.need.p + NEED_LAYER_FULL;
    RG_TRY(T.run("k_trace", [&] { return launch_trace(ta, C, stream); }));
    if (win) {
        // The reads whose walk the window could not serve (k_trace flagged them ST_LAYER_FULL): full-width layers and a second
        // walk, launched whatever their number — no host round trip; the kernels return at the top for every other read
        la.only_full = 1;
        fwd_side();
        RG_TRY(T.run("k_layer_full", [&] { return launch_layer16(la, chunk, C, stream); }));
        if (plan.mode == RG_MODE_RECOMBINATION) {
            rev_side();
            RG_TRY(T.run("k_layer_full", [&] { return launch_layer16(la, chunk, C, stream); }));
        }
        ta.window = 0; ta.only_full = 1;
        RG_TRY(T.run("k_trace_full", [&] { return launch_trace(ta, C, stream); }));
    }
    return read_back();
}

// ONE read-back per chunk: cell updates + overflow summary, through pinned memory on the batch's stream
int Run::read_back() {
    HIPCHK(hipMemcpyAsync(w.h_sum, d_cells, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(w.h_sum + 1 + NEED_WORDS / 2, d_cells + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(w.h_sum + 1, w.need.p, NEED_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    return T.collect(stats);
}

// the whole pipeline of the chunk, enqueued on the stream and waited for
int Run::enqueue_chunk() {
    HIPCHK(hipMemsetAsync(w.state.p, 0, sizeof(ReadState) * chunk, stream));
    if (plan.gap) return enqueue_pathwise_gap();
    if (plan.edit_strands) return enqueue_pathwise_edit_strands();
    if (plan.edit) return plan.edit_xlong ? enqueue_pathwise_edit_xlong() : enqueue_pathwise_edit();
    SweepArgs sa = sweep_args();
    SeedArgs se;
    se.g = gd; se.state = w.state.p; se.nreads = chunk; se.mode = p.mode; se.sc = sc; se.reads = d_reads; se.read_off = off();
    int rc = plan.mode == RG_MODE_PATHWISE ? enqueue_pathwise(sa, se) : enqueue_recombination(sa, se);
    if (rc) return rc;
    return enqueue_tail();
}

int Run::dump_list_stats() {
    const unsigned* nd = need();
    std::vector<unsigned> hn(chunk), hr(chunk);
    HIPCHK(hipMemcpy(hn.data(), w.nf.p, sizeof(unsigned) * chunk, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hr.data(), w.nr.p, sizeof(unsigned) * chunk, hipMemcpyDeviceToHost));
    unsigned long long sf = 0, sr = 0;
    for (int i = 0; i < chunk; ++i) { sf += hn[i]; sr += hr[i]; }
    fprintf(stderr, "[rg] chunk %d reads: fwd cand mean %.1f max %u (cap %u), rev cand mean %.1f max %u (cap %u)\n", chunk,
            (double)sf / chunk, nd[0], w.fcap, (double)sr / chunk, nd[1], w.rcap);
    if (plan.use_rec) {
        HIPCHK(hipMemcpy(hn.data(), w.nrec.p, sizeof(unsigned) * chunk, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hr.data(), w.nrrec.p, sizeof(unsigned) * chunk, hipMemcpyDeviceToHost));
        sf = sr = 0;
        for (int i = 0; i < chunk; ++i) { sf += hn[i]; sr += hr[i]; }
        fprintf(stderr, "[rg] records: forward mean %.1f max %u (cap %u), reverse mean %.1f max %u (cap %u)\n",
                (double)sf / chunk, nd[2], w.frec_cap, (double)sr / chunk, nd[3], w.rrec_cap);
    }
    return RG_OK;
}

// candidate-list / record-list overflow of -m 8: regrow, and the chunk runs again (k_layer / k_trace skipped its reads)
int Run::regrow_lists(bool& redo) {
    redo = false;
    if (plan.mode != RG_MODE_RECOMBINATION) return RG_OK;
    const unsigned needf = need()[0], needr = need()[1], needrec = need()[2], needrrec = need()[3];
    if (debug) {
        const int rc = dump_list_stats();
        if (rc) return rc;
    }
    if (plan.use_rec && (needrrec > w.rrec_cap || needrec > w.frec_cap)) {
        const unsigned long long fullrec = (unsigned long long)h.L * WAVE;
        if ((needrrec > w.rrec_cap && w.rrec_cap >= fullrec) || (needrec > w.frec_cap && w.frec_cap >= fullrec))
            return fail(RG_ERR_CAPACITY, "record list overflow at full size");
        while (w.rrec_cap < needrrec) w.rrec_cap = (unsigned)std::min<unsigned long long>(2ull * w.rrec_cap, fullrec);
        while (w.frec_cap < needrec) w.frec_cap = (unsigned)std::min<unsigned long long>(2ull * w.frec_cap, fullrec);
        redo = true;
    }
    if (needf > w.fcap || needr > w.rcap) {
        const unsigned long long full = (unsigned long long)h.L * plan.wpad;
        if ((needf > w.fcap && w.fcap >= full) || (needr > w.rcap && w.rcap >= full) || needf > full || needr > full)
            return fail(RG_ERR_CAPACITY, "candidate list overflow at full size");
        while (w.fcap < needf) w.fcap = (unsigned)std::min<unsigned long long>(2ull * w.fcap, full);
        while (w.rcap < needr) w.rcap = (unsigned)std::min<unsigned long long>(2ull * w.rcap, full);
        redo = true;
    }
    return RG_OK;
}

int Run::dump_spec4_retries() {
    std::vector<ReadState> hs((size_t)chunk);
    std::vector<int> hp((size_t)chunk), hlb((size_t)chunk);
    HIPCHK(hipMemcpy(hs.data(), w.state.p, sizeof(ReadState) * (size_t)chunk, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hp.data(), w.pick.p, sizeof(int) * (size_t)chunk, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hlb.data(), w.lb.p, sizeof(int) * (size_t)chunk, hipMemcpyDeviceToHost));
    int shown = 0;
    for (int i = 0; i < chunk && shown < 16; ++i)
        if (hs[(size_t)i].status & ST_RETRY) {
            ++shown;
            fprintf(stderr, "[rg]   -m 4 read %d: pick %d, best path %d, best score %d, bound %d\n", i, hp[(size_t)i], hs[(size_t)i].fwd_path, hs[(size_t)i].s0, hlb[(size_t)i]);
        }
    return RG_OK;
}

// which of the second-pass reads are there because of their paths, and what the paths were
int Run::dump_dsel_retries() {
    std::vector<ReadState> hs((size_t)chunk);
    std::vector<int> hp((size_t)chunk), hp2((size_t)chunk * 2, -1);
    std::vector<int> hlb((size_t)chunk);
    HIPCHK(hipMemcpy(hs.data(), w.state.p, sizeof(ReadState) * (size_t)chunk, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hp.data(), w.pick.p, sizeof(int) * (size_t)chunk, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hlb.data(), w.lb.p, sizeof(int) * (size_t)chunk, hipMemcpyDeviceToHost));
    if (plan.pick_two) HIPCHK(hipMemcpy(hp2.data(), w.pick2.p, sizeof(int) * 2 * (size_t)chunk, hipMemcpyDeviceToHost));
    int nb = 0, npath = 0, shown = 0;
    for (int i = 0; i < chunk; ++i) {
        const ReadState& r = hs[(size_t)i];
        if (!(r.status & ST_RETRY)) continue;
        const bool bound_bad = r.fscore < (float)hlb[(size_t)i];
        nb += bound_bad;
        npath += !bound_bad;
        if (!bound_bad && shown < 24) {
            ++shown;
            fprintf(stderr, "[rg]   read %d: picks %d / %d, final paths %d -> %d (rec col %d), score %.1f, bound %d\n", i, hp[(size_t)i], hp2[2 * (size_t)i],
                    r.fwd_path, r.rev_path, r.rec_col, r.fscore, hlb[(size_t)i]);
            fprintf(stderr, "[rg]        fen %d rsn %d of %d rows\n", r.fen, r.rsn, h.L);
        }
    }
    fprintf(stderr, "[rg] second pass: %d for the bound, %d for their paths\n", nb, npath);
    return RG_OK;
}

// The speculative bound of the flagged reads was above what they reach: pairs may have been pruned.  Align them again,
// as a batch of their own, with the provable bound, and put the records in place.
int Run::second_pass(unsigned long long& cells_perf) {
    std::vector<uint8_t> fl((size_t)chunk);
    std::vector<long long> ho((size_t)chunk + 1);
    HIPCHK(hipMemcpy(fl.data(), w.rt_flags.p, (size_t)chunk, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ho.data(), off(), sizeof(long long) * ((size_t)chunk + 1), hipMemcpyDeviceToHost));
    std::vector<int> idx;
    std::vector<long long> so(1, 0);
    for (int i = 0; i < chunk; ++i)
        if (fl[(size_t)i]) { idx.push_back(i); so.push_back(so.back() + (ho[(size_t)i + 1] - ho[(size_t)i])); }
    const int nr = (int)idx.size();
    int rc;
    if ((rc = w.rt_idx.upload(idx)) || (rc = w.rt_off.upload(so)) || (rc = w.rt_reads.alloc((size_t)so.back() + 1)) ||
        (rc = w.rt_bad.alloc((size_t)nr)) || (rc = w.rt_rec.alloc((size_t)nr)) || (rc = w.rt_ops.alloc((size_t)nr * (size_t)ops_stride)) ||
        (rc = w.rt_cells.alloc(2)))
        return rc;
    HIPCHK(hipMemsetAsync(w.rt_bad.p, 0, (size_t)nr, stream));
    RG_TRY(T.inst(launch_gather_reads(d_reads, off(), w.rt_idx.p, w.rt_off.p, w.rt_reads.p, nr, stream)));
    // the same timer and statistics; work buffers and a cell counter of its own, three quarters of what is free now, one level up
    const PathCtx again{h, gd, p, w.retry, stream, w.rt_cells.p, 0, T, stats, spec_level + 1};
    const PathJob failed{w.rt_reads.p, w.rt_off.p, w.rt_bad.p, nr, max_n, w.rt_rec.p, w.rt_ops.p, ops_stride};
    unsigned long long c2[2] = {0, 0};
    RG_TRY(path_driver_run(again, failed, c2));
    RG_TRY(T.inst(launch_scatter_results(w.rt_idx.p, w.rt_rec.p, w.rt_ops.p, d_rec + done, d_ops + (long long)done * ops_stride, ops_stride, nr, stream)));
    HIPCHK(hipStreamSynchronize(stream));
    cells_perf += c2[1];             // the second pass is work the sweeps performed too (the counted figure stays the workload's)
    return T.collect(stats);         // (the labels of the scatter, launched behind the nested pass's last collect: nothing to wait for)
}

}  // namespace

int path_driver_vote_table(const HostGraph& h, PathWork& pw, const uint32_t** keys, unsigned* table_mask) {
    if (!pw.impl) pw.impl = new PathWorkImpl();
    const int rc = ensure_tables(h, *pw.impl);
    if (rc) return rc;
    *keys = pw.impl->kmer_keys.p;
    *table_mask = pw.impl->kmer_mask;
    return RG_OK;
}

int path_driver_run(const PathCtx& c, const PathJob& j, unsigned long long* cells /* [2]: counted | performed, added to */) {
    const HostGraph& h = c.h;
    const rg_params& p = c.p;
    hipStream_t stream = c.stream;
    unsigned long long* d_cells = c.d_cells;
    KernelStats& stats = c.stats;
    const int nreads = j.nreads;
    if (!c.w.impl) c.w.impl = new PathWorkImpl();
    PathWorkImpl& w = *c.w.impl;
    const Options& opt = options();
    PathPlan plan;
    int rc = plan_pathwise(p, PathPlanInput{h.P, h.L, h.fslots, h.rslots, h.max_path_rows, j.max_n}, opt, c.spec_level, plan);
    if (rc || (rc = plan_gap_stage(plan, j.stage))) return rc;
    Run r{h, c.gd, p, w, plan, j.reads, j.off, j.bad, j.max_n, j.rec, j.ops, j.ops_stride, d_cells, stream, stats, c.spec_level, c.T, opt.debug != 0};
    for (int i = 0; i < 36; ++i) r.sc.t[i] = p.scores[i];
    r.h_off = j.h_off;
    if (!w.h_sum) HIPCHK(hipHostMalloc((void**)&w.h_sum, (2 + NEED_WORDS / 2) * sizeof(unsigned long long), hipHostMallocDefault));
    if ((rc = w.need.alloc(NEED_WORDS)) || (rc = ensure_tables(h, w))) return rc;
    if (w.fcap == 0) { w.fcap = plan.fcap; w.rcap = plan.rcap; w.frec_cap = plan.frec_cap; w.rrec_cap = plan.rrec_cap; }
    // reads per chunk: bounded by a memory budget for the per-read work buffers
    size_t budget = (size_t)96 << 30;
    {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget = fr / 4 * 3;
        // a handle of the streaming engine has its own share of the device (what it already holds counts towards it)
        if (c.mem_budget) budget = c.mem_budget;
    }
    unsigned long long cells_done = 0, cells_perf = 0;
    int oom_shift = 0;      // the budget is halved every time a work-buffer allocation fails (other handles / the retry pass took the memory)
    while (r.done < nreads) {
        HIPCHK(hipMemsetAsync(d_cells, 0, 2 * sizeof(unsigned long long), stream));  // cell updates of this chunk attempt (counted | performed)
        HIPCHK(hipMemsetAsync(w.need.p, 0, NEED_WORDS * sizeof(unsigned), stream));
        const size_t per_read_all = plan.per_read_all(w.fcap, w.rcap, w.frec_cap, w.rrec_cap);
        int maxchunk = (int)std::min<size_t>(8192, std::max<size_t>(1, (budget >> oom_shift) / per_read_all));
        if (opt.chunk_reads > 0) maxchunk = std::min<int>(maxchunk, opt.chunk_reads);
        const double dbg_t0 = r.debug ? now_s() : 0;
        const int chunk = r.chunk = (int)even_chunks(nreads - r.done, maxchunk);
        bool oom = false;
        if ((rc = r.alloc_chunk(&oom))) {
            // out of memory (the share was measured before other buffers of the device existed): smaller launches, like run_poa.
            // Any OTHER HIP failure is reported at once (it used to be retried up to twelve times with halved chunks).
            if (rc == RG_ERR_HIP && oom && chunk > 1 && oom_shift < 12) { ++oom_shift; continue; }
            return rc;
        }
        if (r.debug) fprintf(stderr, "[rg] chunk of %d reads: buffers ready after %.1f ms\n", chunk, (now_s() - dbg_t0) * 1e3);
        if ((rc = r.enqueue_chunk())) return rc;
        if (r.debug) fprintf(stderr, "[rg] chunk of %d reads: done after %.1f ms\n", chunk, (now_s() - dbg_t0) * 1e3);
        if (r.async_err != hipSuccess) return fail(RG_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(r.async_err));
        bool redo = false;
        if ((rc = r.regrow_lists(redo))) return rc;
        if (redo) continue;
        const unsigned long long chunk_cells = w.h_sum[0];
        cells_perf += w.h_sum[1 + NEED_WORDS / 2];
        const unsigned nretry = r.nretry();
        if (r.debug && (plan.spec || plan.spec4)) fprintf(stderr, "[rg] speculative bound (margin %d): %u of %d reads did not reach it\n", plan.spec_margin, nretry, chunk);
        if (r.debug && plan.spec4 && nretry && (rc = r.dump_spec4_retries())) return rc;
        if (r.debug && plan.dsel && (rc = r.dump_dsel_retries())) return rc;
        if (plan.layer_window) {
            // reads the column window of the layers could not serve (rebuilt at full width in the same chunk), as a pseudo-stat:
            // the "ms" field holds the READS, summed over the chunks (like the bytes of mem:work_bytes_per_read), "launches" the chunks
            add_stat(stats, "mem:layer_full_reads", (double)r.need()[NEED_LAYER_FULL], 1);
            if (r.debug) fprintf(stderr, "[rg] layer window of %d columns: %u of %d reads took the full-width layers\n", plan.layer_window, r.need()[NEED_LAYER_FULL], chunk);
        }
        if (plan.use_rec) {
            // rows of the silent register runs of both record sweeps and of all their register runs (k_sweep16, SILENT RUNS), as
            // pseudo-stats: "ms" holds the ROWS, summed over the chunks and the passes
            add_stat(stats, "mem:silent_rows", (double)r.need()[NEED_SILENT_ROWS], 1);
            add_stat(stats, "mem:run_rows", (double)r.need()[NEED_RUN_ROWS], 1);
            // ... and the key work of their tails and general-path records: eager member folds, rows closed, rows that wrote a record,
            // member folds left out (k_sweep16, KEY WORK THAT NO RECORD USES)
            add_stat(stats, "mem:key_folds", (double)r.need()[NEED_KEY_FOLDS], 1);
            add_stat(stats, "mem:key_rows", (double)r.need()[NEED_KEY_ROWS], 1);
            add_stat(stats, "mem:key_rows_hit", (double)r.need()[NEED_KEY_ROWS_HIT], 1);
            const unsigned* kn = r.need();
            add_stat(stats, "mem:key_folds_saved", (double)kn[NEED_KEY_SAVED_GATHER] + (double)kn[NEED_KEY_SAVED_GENERAL] + (double)kn[NEED_KEY_SAVED_TAIL], 1);
            add_stat(stats, "mem:key_saved_gather", (double)kn[NEED_KEY_SAVED_GATHER], 1);
            add_stat(stats, "mem:key_saved_general", (double)kn[NEED_KEY_SAVED_GENERAL], 1);
            add_stat(stats, "mem:key_saved_tail", (double)kn[NEED_KEY_SAVED_TAIL], 1);
        }
        if (nretry && (rc = r.second_pass(cells_perf))) return rc;
        cells_done += chunk_cells;
        r.done += chunk;
        // HBM work buffers of one read of this chunk (rolling rows, direction words, layers, candidate and record lists): reported
        // as a pseudo-kernel so that callers see the footprint without another ABI entry ("ms" holds bytes, summed over the chunks)
        add_stat(stats, "mem:work_bytes_per_read", (double)per_read_all, 1);
    }
    cells[0] += cells_done;
    cells[1] += cells_perf;
    return RG_OK;
}

}  // namespace rg
