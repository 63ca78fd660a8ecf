// Batch driver of the six POA modes (-m 0 .. -m 3): one routine over a mode table.  It sizes the arenas from the free HBM,
// launches the mode's kernel over the reads in even launches on the handle's stream (timed by the handle's KernelTimer), and,
// in the banded modes, regrows the band arena when a read's band did not fit.
#include <algorithm>
#include <cstdio>

#include "rg_batch_impl.hpp"

namespace {

// One row per mode.  banded: band arenas + per-row band records (rinfo), an overflow check with arena doubling, and smaller
// launches when an arena allocation fails; otherwise full (L - 1) x W matrices per read.  free_num / free_den: the share of
// the free HBM one launch's arenas may take on a handle without a mem_budget of its own — 45 % in the banded modes, so that a
// second handle of a streaming caller fits beside this one, three quarters in the local ones; a handle of the streaming
// engine has its share of the device instead (mem_budget, at most 90 % of what is free, in every mode).
struct PoaMode {
    int mode;
    const char* kname;         // the kernel's entry in the statistics
    int planes;                // score / path planes per cell (2: m | y and w0 | w1 of the gap modes)
    bool banded;
    size_t free_num, free_den;
    const char* (*launch)(const PoaArgs&, hipStream_t);
};
const PoaMode kPoaModes[] = {
    {RG_MODE_GLOBAL_POA, "k_m0_simd", 1, true, 45, 100, launch_m0_simd},
    {RG_MODE_GLOBAL_POA_SCALAR, "k_m0_scalar", 1, true, 45, 100, launch_m0_scalar},
    {RG_MODE_GAP_POA, "k_m2_gap", 2, true, 45, 100, launch_m2},
    {RG_MODE_LOCAL_POA, "k_m1_local_simd", 1, false, 3, 4, [](const PoaArgs& a, hipStream_t s) { return launch_local(a, 0, s); }},
    {RG_MODE_LOCAL_POA_SCALAR, "k_m1_local_scalar", 1, false, 3, 4, [](const PoaArgs& a, hipStream_t s) { return launch_local(a, 1, s); }},
    {RG_MODE_GAP_LOCAL_POA, "k_m3_gap_local", 2, false, 3, 4, [](const PoaArgs& a, hipStream_t s) { return launch_local(a, 2, s); }},
};
const PoaMode* poa_mode(int mode) {
    for (const PoaMode& m : kPoaModes) if (m.mode == mode) return &m;
    return nullptr;
}

// everything of the argument block but the launch's reads (read_base, nreads)
PoaArgs poa_args(const rg_batch* b) {
    const GraphTables* g = b->gt;
    PoaArgs a;
    a.g = DevLnz{b->g->h.L, g->d_lnz.p, g->d_pred_off.p, g->d_pred_rows.p, g->d_r_values.p, g->d_min_pred.p};
    for (int i = 0; i < 36; ++i) a.sc.t[i] = b->p.scores[i];
    a.reads = b->in.reads; a.read_off = b->in.off; a.bad = b->in.bad; a.bta = b->in.bta; a.col0 = b->d_col0.p; a.rowmeta = b->d_rowmeta.p; a.rowmeta_b = b->d_rowmeta_b.p;
    a.nreads = 0; a.read_base = 0;
    a.gap_open = b->p.gap_open; a.gap_ext = b->p.gap_ext; a.max_n = b->max_n; a.lds_read = b->max_n <= 16000 ? 1 : 0;
    a.cap_cells = b->cap_cells; a.arena_m = b->d_arena_m.p; a.arena_pw = b->d_arena_pw.p; a.rinfo = b->d_rinfo.p;
    a.rec = b->d_rec.p; a.ops = b->d_ops.p; a.oprows = b->d_oprows.p; a.ops_stride = b->ops_stride;
    a.cells = b->d_cells.p;
    return a;
}

// PoaArgs::rowmeta / rowmeta_b: {pred_off[i + 1], r_values[i], third(i), (first listed predecessor + 1) | base code << 24}
template <typename F>
std::vector<int4> row_meta(const HostGraph& h, F&& third) {
    std::vector<int4> rm(h.L, make_int4(0, 0, 0, 0));
    for (int i = 0; i < h.L; ++i) {
        const int pbeg = (int)h.pred_off[i], pend = (int)h.pred_off[i + 1];
        const int p0 = pend > pbeg ? (int)h.pred_rows[pbeg] : -1;
        const int c = (i >= 1 && i + 1 < h.L) ? base_code(h.lnz[i]) : 4;
        rm[i] = make_int4(pend, (int)h.r_values[i], third(i), (p0 + 1) | ((c < 0 ? 4 : c) << 24));
    }
    return rm;
}

}  // namespace

bool is_poa(int mode) { return poa_mode(mode) != nullptr; }

int poa_upload_tables(rg_batch* b) {
    const HostGraph& h = b->g->h;
    const int mode = b->p.mode;
    // column-0 chain of m0 (global_abpoa.rs:36-46)
    std::vector<int> col0(h.L, 0);
    for (int i = 1; i + 1 < h.L; ++i) col0[i] = col0[h.min_pred[i]] + b->p.scores[base_code(h.lnz[i]) * 6 + 5];
    RG_TRY(b->d_col0.upload(col0));
    if (mode == RG_MODE_GLOBAL_POA) return b->d_rowmeta.upload(row_meta(h, [&](int i) { return col0[i]; }));      // k_m0_simd
    if (mode == RG_MODE_GLOBAL_POA_SCALAR || mode == RG_MODE_GAP_POA)                                           // k_poa_banded
        return b->d_rowmeta_b.upload(row_meta(h, [&](int i) { return i > 0 ? (int)h.min_pred[i] : 0; }));
    return RG_OK;
}

int run_poa(rg_batch* b) {
    const HostGraph& h = b->g->h;
    if (!h.has_lnz) return fail(RG_ERR_ARG, "graph has no LnzGraph view");
    const PoaMode& m = *poa_mode(b->p.mode);
    KernelTimer& T = b->timer;
    if (!m.banded) b->cap_cells = (long long)(h.L - 1) * (b->max_n + 1);
    int oom_shift = 0;      // the budget is halved every time an arena allocation fails (other handles / threads took the memory)
    for (int attempt = 0; attempt < 24; ++attempt) {
        const size_t per_read = (size_t)b->cap_cells * m.planes * (sizeof(int) + sizeof(uint32_t)) + (m.banded ? (size_t)h.L * sizeof(int4) : 0);
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        free_b += b->d_arena_m.bytes() + b->d_arena_pw.bytes() + b->d_rinfo.bytes();   // what a previous run holds is reused
        const size_t budget = (b->mem_budget ? std::min(b->mem_budget, free_b / 10 * 9) : free_b / m.free_den * m.free_num) >> oom_shift;
        if (per_read > budget)
            return fail(RG_ERR_CAPACITY, m.banded ? "band arena of one read exceeds the free HBM" : "local POA: one read's L x W matrices exceed the free HBM");
        long long maxchunk = (long long)std::min<size_t>((size_t)b->nreads, budget / per_read);
        if (options().chunk_reads > 0) maxchunk = std::min<long long>(maxchunk, options().chunk_reads);
        const long long chunk = even_chunks(b->nreads, maxchunk);      // (arena slots are launch-relative: the split changes no result)
        if (options().debug) fprintf(stderr, "[rg] run_poa attempt %d: cap_cells %lld, budget %.1f GB, per read %.2f MB, chunk %lld of %lld reads\n", attempt,
                                     b->cap_cells, budget / 1e9, per_read / 1e6, chunk, (long long)b->nreads);
        int rc;
        if ((rc = b->d_arena_m.alloc((size_t)chunk * b->cap_cells * m.planes)) || (rc = b->d_arena_pw.alloc((size_t)chunk * b->cap_cells * m.planes)) ||
            (m.banded && (rc = b->d_rinfo.alloc((size_t)chunk * h.L)))) {
            // Out of memory: smaller launches.  Banded modes only: their 45 % leaves room that other handles may take between the
            // measurement and the allocation; a full-matrix launch that does not fit what was just measured as free is reported.
            if (m.banded && rc == RG_ERR_HIP && chunk > 1 && oom_shift < 8) { ++oom_shift; continue; }
            return rc;
        }
        HIPCHK(hipMemsetAsync(b->d_cells.p, 0, sizeof(unsigned long long), b->stream));
        PoaArgs a = poa_args(b);
        for (long long base = 0; base < b->nreads; base += chunk) {
            a.read_base = (int)base;
            a.nreads = (int)std::min<long long>(chunk, b->nreads - base);
            RG_TRY(T.run(m.kname, [&] { return m.launch(a, b->stream); }));
        }
        RG_TRY(T.collect(b->stats));
        if (m.banded) {
            // overflow check: a read whose band cells did not fit asks for a bigger arena
            b->rec.resize(b->nreads);
            HIPCHK(hipMemcpy(b->rec.data(), b->d_rec.p, sizeof(DevRecord) * b->nreads, hipMemcpyDeviceToHost));
            if (std::any_of(b->rec.begin(), b->rec.end(), [](const DevRecord& r) { return (r.status & ST_OVERFLOW) != 0; })) {
                const long long full = (long long)h.L * (b->max_n + 1);
                if (b->cap_cells >= full) return fail(RG_ERR_CAPACITY, "band arena overflow at full size");
                b->cap_cells = std::min(full, b->cap_cells * 2);
                reset_stats(b->stats);      // a regrown run reports its last attempt only
                continue;
            }
        }
        unsigned long long c = 0;
        HIPCHK(hipMemcpy(&c, b->d_cells.p, sizeof c, hipMemcpyDeviceToHost));
        b->cells = b->cells_performed = c;      // (the POA kernels evaluate exactly the cells they count)
        return RG_OK;
    }
    return fail(RG_ERR_CAPACITY, "band arena overflow");
}
