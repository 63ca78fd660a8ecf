// extern "C" surface of librecgraph_hip (see include/recgraph_hip.h): handle creation and validation, the read loader (uploads
// the reads, sizes the per-read buffers), the result accessors and the GAF text assembly.  The kernels are launched by the batch
// drivers: rg_poa_driver.hip (POA modes), rg_strand_driver.hip over rg_path_driver.hip (pathwise modes).
//
// There is deliberately NO CPU fallback: without a usable HIP device every batch call returns
// RG_ERR_NO_DEVICE.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include <unistd.h>

#include <cstdio>
#include <cstdlib>

#include "rg_batch_impl.hpp"
#include "rg_path_plan.hpp"

void rg_batch_destroy_impl(rg_batch* b) {
    if (!b) return;
    DevGuard dg(b->dev);            // buffers and stream are freed on the device that owns them
    delete b;
}

namespace rg {
int wait_stream_sleeping(void* stream, void* ev, bool spin) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (spin || options().spin_wait || !ev) return (int)hipStreamSynchronize(s);
    hipEvent_t e = static_cast<hipEvent_t>(ev);
    hipError_t rc = hipEventRecord(e, s);
    if (rc != hipSuccess) return (int)rc;
    for (unsigned spins = 0;; ++spins) {
        rc = hipEventQuery(e);
        if (rc != hipErrorNotReady) return (int)rc;
        (void)hipGetLastError();                         // hipErrorNotReady is sticky in hipGetLastError
        usleep(50);                                      // ~100 us per poll with the timer slack: a few % of one CPU per thread
    }
}
}  // namespace rg

// Text of read i exactly as the reference prints it (warning lines + GAFStruct::to_string), appended to `out`.
extern "C" {
static bool build_fields(const rg_batch* b, int64_t i, const char* name, GafFields& out);
}
static uint32_t public_status(uint32_t s) { return s & 0xffu; }
// the record of read i as the host formatter takes it
static void fill_record(const rg_batch* b, int64_t i, ReadRecord& r) {
    const DevRecord& d = b->rec[i];
    r.status = public_status(d.status); r.score = d.score; r.fscore = d.fscore; r.end_row = d.end_row; r.end_col = d.end_col;
    r.stop_row = d.stop_row; r.stop_col = d.stop_col; r.best_path = d.best_path; r.rev_path = d.rev_path; r.fen = d.fen;
    r.rsn = d.rsn; r.rec_col = d.rec_col; r.displacement = d.displacement; r.n_ops = d.n_ops; r.n_fwd_ops = d.n_fwd_ops;
    r.ops = b->ops.data() + (size_t)i * b->ops_stride;
    r.rows = is_poa(b->p.mode) ? b->oprows.data() + (size_t)i * b->ops_stride : nullptr;
}
// RG_AMB_BOTH_STRANDS (set by rg_batch_create on every handle of a both-strands family): the record of read i came from the
// reverse-complement pass (DevRecord.pad is written by that mode's kernels only)
static bool reverse_won(const rg_batch* b, int64_t i) {
    return (b->p.amb_mode & RG_AMB_BOTH_STRANDS) && !is_poa(b->p.mode) && (b->rec[i].pad & REC_REVERSE_STRAND);
}
// ... and the base codes that record aligns: the reverse complement of the read (sequences.rs:65-82), built for the chosen reads only
static const uint8_t* revcomp_codes(const rg_batch* b, int64_t i, std::vector<uint8_t>& buf) {
    const size_t lo = (size_t)b->off[i], n = (size_t)(b->off[i + 1] - b->off[i]);
    buf.resize(n);
    for (size_t k = 0; k < n; ++k) { const uint8_t c = b->codes[lo + n - 1 - k]; buf[k] = c < 4 ? (uint8_t)(3 - c) : c; }
    return buf.data();
}
bool amb_take_rev(int mode, int32_t fwd_score, int32_t rev_score) {
    if (mode == RG_MODE_LOCAL_POA || mode == RG_MODE_LOCAL_POA_SCALAR) return !(fwd_score < rev_score);   // main.rs:160-164 (sic)
    return rev_score > fwd_score;
}
static void append_gaf(const rg_batch* b, int64_t i, const char* name, int64_t seq_index, std::string& out, const AmbRetry* amb = nullptr) {
    const DevRecord& d = b->rec[i];
    GafFields f;
    // seq_name.1 == 0 means "score only" in the POA modes alone (global_abpoa.rs:241, :411; gap_global_abpoa.rs:229;
    // local_poa.rs / gap_local_poa.rs likewise).  The pathwise modes take no seq_name: main.rs:260,268,311 hand `i` to
    // write_gaf only, and read 0 gets its record like every other read.
    const bool score_only = seq_index == 0 && is_poa(b->p.mode);
    const int64_t k = amb && amb->rb && amb->rev_index ? amb->rev_index[i] : -1;
    if (k >= 0 && !score_only && !(amb->rb->rec[(size_t)k].status & ST_NO_RECORD)) {
        // both exec calls print their warning lines while they run; write_gaf then prints the record the comparison picks
        GafFields r;
        if (build_fields(b, i, name, f) && build_fields(amb->rb, k, name, r)) {
            out += f.pre;
            out += r.pre;
            out += amb_take_rev(b->p.mode, d.score, amb->rb->rec[(size_t)k].score) ? r.line() : f.line();
            out += '\n';
            return;
        }
    }
    if (!score_only && !is_poa(b->p.mode) && !(d.status & ST_NO_RECORD)) {
        // the pathwise modes: straight into the buffer (the same bytes as build_fields(..).text(): tests/test_gpu_stream.py
        // holds the stream's text, written here, equal to rg_result_gaf's, written there)
        ReadRecord r;
        fill_record(b, i, r);
        static thread_local std::vector<uint8_t> rcbuf;
        const bool rev = reverse_won(b, i);
        append_pathwise_text(b->g->h, rev ? revcomp_codes(b, i, rcbuf) : b->codes + (size_t)b->off[i], (int)(b->off[i + 1] - b->off[i]),
                             name ? name : "", r, b->p.mode, out, rev ? '-' : '+');
        return;
    }
    if (!score_only && build_fields(b, i, name, f)) out += f.text();
    else if ((d.status & ST_NO_RECORD) == 0 && (d.status & ST_BAND_WARNING))
        out += "Band length probably too short, maybe try with larger b and f\n";
}

// All GAF text of a fetched batch in input order, formatted by `nthreads` host threads (contiguous blocks of reads per
// thread, concatenated).  Name of read i: names[i], or "read<name_base + i>".  offs (optional): nreads + 1 offsets of the
// reads' texts inside `out`.
void format_batch(const rg_batch* b, const char* const* names, int64_t name_base, int64_t seq_index_base, int nthreads,
                  std::string& out, std::vector<int64_t>* offs, const AmbRetry* amb) {
    const int64_t n = b->nreads;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > n) nthreads = (int)std::max<int64_t>(1, n);
    std::vector<std::string> parts((size_t)nthreads);
    std::vector<int64_t> lens((size_t)n);
    auto work = [&](int t) {
        const int64_t lo = n * t / nthreads, hi = n * (t + 1) / nthreads;
        std::string& o = parts[(size_t)t];
        o.reserve((size_t)(hi - lo) * 2304);
        std::string nm;
        for (int64_t i = lo; i < hi; ++i) {
            const size_t before = o.size();
            const char* name;
            if (names) name = names[i];
            else { nm = "read" + std::to_string(name_base + i); name = nm.c_str(); }
            append_gaf(b, i, name, seq_index_base + i, o, amb);
            lens[(size_t)i] = (int64_t)(o.size() - before);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& t : th) t.join();
    size_t total = 0;
    for (auto& s : parts) total += s.size();
    out.clear();
    out.reserve(total + 1);
    for (auto& s : parts) out += s;
    if (offs) {
        offs->resize((size_t)n + 1);
        int64_t acc = 0;
        for (int64_t i = 0; i < n; ++i) { (*offs)[(size_t)i] = acc; acc += lens[(size_t)i]; }
        (*offs)[(size_t)n] = acc;
    }
}

// Results of a fetched batch as a handle of their own (host records only): the device handle is free for the next
// read set while a caller still reads this one through the rg_result_* accessors.
rg_batch* rg_batch_detach_results(rg_batch* b) {
    auto r = std::make_unique<rg_batch>();
    r->g = b->g;
    r->p = b->p;
    r->nreads = b->nreads;
    r->dev = -1;
    r->off = b->off;
    r->codes_own.assign(b->codes, b->codes + (size_t)b->off[(size_t)b->nreads]);
    r->codes = r->codes_own.data();
    r->rec = std::move(b->rec);
    r->ops = std::move(b->ops);
    r->oprows = std::move(b->oprows);
    r->ops_stride = b->ops_stride;
    r->cells = b->cells;
    r->cells_performed = b->cells_performed;
    r->stats = b->stats;
    r->fetched = true;
    b->fetched = false;
    return r.release();
}

extern "C" {

const char* rg_last_error(void) { return g_last_error.c_str(); }

int32_t rg_set_option(const char* name, int64_t value) {
    const OptionDesc* d = find_option(name);
    if (!d) return fail(RG_ERR_ARG, std::string("unknown option ") + (name ? name : "(null)"));
    store_option(options(), *d, value);
    return RG_OK;
}
int64_t rg_get_option(const char* name) {
    const OptionDesc* d = find_option(name);
    return d ? (int64_t)(options().*d->slot).load() : -1;
}

int32_t rg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int32_t rg_set_device(int32_t dev) {
    HIPCHK(hipSetDevice(dev));
    return RG_OK;
}

void rg_scores_match_mis(int32_t m, int32_t x, int32_t f32_variant, int32_t* s) {
    // score_matrix.rs:35-66
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            if (i == j) s[i * 6 + j] = m;
            else if (!f32_variant && (i == 5 || j == 5)) s[i * 6 + j] = 2 * x;
            else s[i * 6 + j] = x;
        }
    s[4 * 6 + 4] = x;
    s[5 * 6 + 5] = RG_SCORE_MISSING;
}

void rg_params_default(rg_params* p, int32_t mode) {
    memset(p, 0, sizeof *p);
    p->mode = mode;
    rg_scores_match_mis(2, -4, 0, p->scores);
    p->gap_open = -4;
    p->gap_ext = -2;
    p->band_b = 1.0f;
    p->band_f = 0.01f;
    p->bta_override = -1;
    p->base_rec_cost = 4;
    p->multi_rec_cost = 0.1f;
    p->rec_band_width = 1.0f;
}

int32_t rg_graph_from_gfa(const char* gfa_text, int64_t len, rg_graph** out) {
    if (!gfa_text || !out) return fail(RG_ERR_ARG, "null argument");
    auto g = std::make_unique<rg_graph>();
    int rc = build_from_gfa(gfa_text, len, g->h);
    if (rc) return rc;
    *out = g.release();
    return RG_OK;
}
int32_t rg_graph_create_lnz(const char* lnz, int64_t L, const int64_t* pred_off, const int64_t* pred_rows,
                            const uint64_t* node_id, rg_graph** out) {
    if (!out) return fail(RG_ERR_ARG, "null argument");
    auto g = std::make_unique<rg_graph>();
    int rc = build_from_lnz(lnz, L, pred_off, pred_rows, node_id, g->h);
    if (rc) return rc;
    *out = g.release();
    return RG_OK;
}
int32_t rg_graph_create_path(const char* lnz, int64_t L, int32_t P, const uint64_t* row_mask, const int64_t* edge_off,
                             const int64_t* edge_pred, const uint64_t* edge_mask, const uint64_t* node_id, rg_graph** out) {
    if (!out) return fail(RG_ERR_ARG, "null argument");
    auto g = std::make_unique<rg_graph>();
    int rc = build_from_path(lnz, L, P, row_mask, edge_off, edge_pred, edge_mask, node_id, g->h);
    if (rc) return rc;
    *out = g.release();
    return RG_OK;
}
void rg_graph_destroy(rg_graph* g) { delete g; }
const char* rg_graph_path_error(const rg_graph* g) { return g ? g->h.path_error.c_str() : ""; }
int64_t rg_graph_rows(const rg_graph* g) { return g ? g->h.L : 0; }
int32_t rg_graph_paths(const rg_graph* g) { return g && g->h.has_path ? g->h.P : 0; }
int64_t rg_graph_dump(const rg_graph* g, int32_t which, char* buf, int64_t cap) {
    std::string s = dump_graph(g->h, which);
    if (buf && (int64_t)s.size() + 1 <= cap) memcpy(buf, s.c_str(), s.size() + 1);
    return (int64_t)s.size();
}

// Largest magnitude an f32 value of -m 0 SIMD (global_abpoa::exec_simd) or AVX2 -m 1 (local_poa::exec_simd) can take on a
// graph of L rows and reads of at most `longest` bases (W = longest + 1 columns).  Every cell is the sum of the entries along
// one alignment path — at most L + W steps of at most E = max |entry| each — started from 0, and in -m 0 possibly from
// min_score = 2 * W * g(read[1], '-') (global_abpoa.rs:20) of a cell outside the band: |value| <= 2 W G + (L + W) E, with G
// the largest |(b, '-')|; -m 1 starts every cell from 0 (no min_score): (L + W) E.  Below 2^24 every such sum is an integer
// that f32 holds exactly, so the int32 kernels compute the reference's values; at or above it the reference may round (the
// order of its additions is not the prefix scans' order) and the batch is refused.
static long long f32_poa_bound(int mode, const int32_t* s, long long L, long long longest) {
    long long E = 0, G = 0;
    for (int i = 0; i < 35; ++i)
        if (s[i] != RG_SCORE_MISSING) E = std::max<long long>(E, std::llabs((long long)s[i]));
    for (int b = 0; b < 5; ++b)
        if (s[b * 6 + 5] != RG_SCORE_MISSING) G = std::max<long long>(G, std::llabs((long long)s[b * 6 + 5]));
    const long long W = longest + 1;
    return (L + W) * E + (mode == RG_MODE_GLOBAL_POA ? 2 * W * G : 0);
}

// Reads of a batch: canonicalised (sequences.rs:13-22), coded, uploaded; every per-read buffer is (re)sized.
// Work buffers of a previous run are kept when they are large enough, so a streaming caller re-uses one handle.
static int load_reads(rg_batch* b, const char* reads, const int64_t* read_off, int64_t nreads) {
    const rg_graph* g = b->g;
    const rg_params* p = &b->p;
    const int mode = p->mode;
    // validation first: a rejected read set leaves the handle exactly as it was
    for (int64_t r = 0; r < nreads; ++r)
        if (read_off[r + 1] - read_off[r] < 1) return fail(RG_ERR_ARG, "empty read");
    if (read_off[nreads] - read_off[0] >= (1ll << 40)) return fail(RG_ERR_ARG, "read set too large");
    if (mode == RG_MODE_GLOBAL_POA || mode == RG_MODE_LOCAL_POA) {
        int64_t longest = 0;
        for (int64_t r = 0; r < nreads; ++r) longest = std::max<int64_t>(longest, read_off[r + 1] - read_off[r]);
        if (f32_poa_bound(mode, p->scores, g->h.L, longest) >= (1ll << 24))
            return fail(RG_ERR_CAPACITY, "scores of this batch can reach 2^24 in magnitude: the reference computes -m 0 (SIMD) and "
                                         "-m 1 (AVX2) in f32, which is not exact there, and the int32 kernels cannot round like it");
    }
    // From here on the handle describes no read set until every buffer is sized and uploaded (`valid`): rg_batch_run and
    // rg_batch_fetch refuse it after a failed allocation instead of launching the new reads against the old buffers.
    b->valid = false;
    b->fetched = false;
    const long long base = read_off[0];
    const size_t total = (size_t)(read_off[nreads] - base);
    // staging layout (8-byte aligned pieces): offsets (int64), bta (int32), codes (u8), bad (u8)
    const size_t o_off = 0, o_bta = o_off + sizeof(long long) * (size_t)(nreads + 1);
    const size_t o_codes = (o_bta + sizeof(int) * (size_t)nreads + 7) & ~(size_t)7;
    const size_t o_bad = (o_codes + total + 7) & ~(size_t)7;
    const size_t in_bytes = o_bad + (size_t)nreads;
    int rc;
    if ((rc = b->stage.alloc(in_bytes)) || (rc = b->d_in.alloc(in_bytes + in_bytes / 4)) || (rc = b->d_rec.alloc(nreads)) ||
        (rc = b->d_cells.alloc(2)))
        return rc;
    b->nreads = nreads;
    b->off.resize(nreads + 1);
    for (int64_t i = 0; i <= nreads; ++i) b->off[i] = read_off[i] - base;
    b->bad.assign(nreads, 0);
    b->bta.resize(nreads);
    uint8_t* codes = b->stage.p + o_codes;
    b->codes = codes;
    // sequences.rs:13-22 ('-' -> 'N', upper case) + base codes, one table pass over the whole blob (rg_reads.cpp)
    b->max_n = (int)std::min<int64_t>(canonicalise_reads(reads, read_off, nreads, codes, b->bad.data()), INT32_MAX);
    for (int64_t r = 0; r < nreads; ++r) {
        const long long n = b->off[r + 1] - b->off[r];
        // main.rs:57: (b + f * seq.len() as f32) as usize, seq.len() = n + 1
        float v = p->band_b + p->band_f * (float)(n + 1);
        long long bt = p->bta_override >= 0 ? p->bta_override : (v > 0 ? (long long)v : 0);
        b->bta[r] = (int)std::min<long long>(bt, 1 << 28);
    }
    memcpy(b->stage.p + o_off, b->off.data(), sizeof(long long) * (size_t)(nreads + 1));
    memcpy(b->stage.p + o_bta, b->bta.data(), sizeof(int) * (size_t)nreads);
    memcpy(b->stage.p + o_bad, b->bad.data(), (size_t)nreads);
    const HostGraph& h = g->h;
    // traceback ops per read: POA walks at most L rows + n columns; a pathwise walk stays on the rows of one path per
    // half (forward to the source, reverse to the sink): <= 2 * (rows of the longest path + n)
    b->ops_stride = is_poa(mode) ? (long long)h.L + b->max_n + 8
                                 : std::min<long long>((long long)h.L + b->max_n + 8, 2ll * (h.max_path_rows + b->max_n) + 16);
    // (-m 64 / -m 65 score both strands in one pass and trace one: the bit is set on their handles, but there is no second pass, no
    // merge and none of the strand buffers)
    const bool both = !is_poa(mode) && (p->amb_mode & RG_AMB_BOTH_STRANDS) && !edit_strands_mode(mode).valid;
    // k_strand_merge moves op bytes in 16-byte pieces (a staged family traces the chosen strand alone: no merge, the op area of one pass)
    if (both && !gap_mode(mode).family->staged) b->ops_stride = (b->ops_stride + 15) & ~15ll;
    if ((rc = b->d_ops.alloc((size_t)nreads * b->ops_stride))) return rc;
    if (both && (rc = size_strand_buffers(b, total))) return rc;
    if (is_poa(mode)) {
        if ((rc = b->d_oprows.alloc((size_t)nreads * b->ops_stride))) return rc;
        long long maxbta = 0;
        for (int v : b->bta) maxbta = std::max<long long>(maxbta, v);
        const long long per_row = std::min<long long>(b->max_n + 1, 2 * maxbta + 40);
        b->cap_cells = std::max(b->cap_cells, (long long)h.L * per_row);   // keeps an arena regrown by an earlier run
    }
    // ONE DMA from the pinned block on the batch's stream (no blit kernel that would queue behind a running sweep of
    // another handle), ordered before the kernels of the next run
    HIPCHK(hipMemcpyAsync(b->d_in.p, b->stage.p, in_bytes, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->in.off = reinterpret_cast<const long long*>(b->d_in.p + o_off);
    b->in.bta = reinterpret_cast<const int*>(b->d_in.p + o_bta);
    b->in.reads = b->d_in.p + o_codes;
    b->in.bad = b->d_in.p + o_bad;
    b->valid = true;
    return RG_OK;
}

int32_t rg_batch_create(const rg_graph* gc, const rg_params* p, const char* reads, const int64_t* read_off, int64_t nreads,
                        rg_batch** out) {
    if (!gc || !p || !reads || !read_off || !out || nreads < 1) return fail(RG_ERR_ARG, "null/empty argument");
    const rg_graph* g = gc;
    const int mode = p->mode;
    const bool path_gap = gap_mode(mode).valid;       // (every rule in every family of rg_gap_modes.hpp)
    const bool path_edit = edit_mode(mode).valid || edit_strands_mode(mode).valid;     // (every rule in every family of rg_edit_modes.hpp, and -m 64 / -m 65: rg_edit_strands_modes.hpp)
    if (!(is_poa(mode) || mode == RG_MODE_PATHWISE || mode == RG_MODE_RECOMBINATION || mode == RG_MODE_PATHWISE_SEMI ||
          mode == RG_MODE_RECOMBINATION_SEMI || path_gap || path_edit))
        return fail(RG_ERR_ARG, "unsupported mode");
    if ((mode == RG_MODE_GAP_POA || mode == RG_MODE_GAP_LOCAL_POA || path_gap || path_edit) && (p->gap_open > 0 || p->gap_ext > 0))
        return fail(RG_ERR_ARG, "gap penalties must be <= 0");
    if (is_poa(mode) && !g->h.has_lnz) return fail(RG_ERR_ARG, "graph has no LnzGraph view");
    if (!is_poa(mode) && !g->h.has_path)
        return fail(g->h.path_error.empty() ? RG_ERR_ARG : RG_ERR_GRAPH,
                    g->h.path_error.empty() ? "graph has no paths (P lines)" : "graph has no PathGraph view: " + g->h.path_error);
    if ((mode == RG_MODE_RECOMBINATION || mode == RG_MODE_RECOMBINATION_SEMI) && (p->base_rec_cost < 0 || p->multi_rec_cost < 0))
        return fail(RG_ERR_ARG, "recombination costs must be non-negative");
    if ((mode == RG_MODE_GLOBAL_POA || mode == RG_MODE_LOCAL_POA) && g->h.L >= (1 << 20))
        return fail(RG_ERR_GRAPH, "rows >= 2^20 break the reference's f32 path-cell decoding (gaf_output.rs:664-668, 783-786)");
    if ((mode == RG_MODE_GAP_POA || mode == RG_MODE_GLOBAL_POA_SCALAR || mode == RG_MODE_LOCAL_POA_SCALAR ||
         mode == RG_MODE_GAP_LOCAL_POA) && g->h.L > 65536)
        return fail(RG_ERR_GRAPH, "rows >= 65536 are truncated by the reference's u16 path cells (bitfield_path.rs:41)");
    if (p->amb_mode & ~15) return fail(RG_ERR_ARG, "amb_mode: only bits 0 to 3 are defined");
    if ((p->amb_mode & RG_AMB_STRAND_VOTE) && (is_poa(mode) || !(p->amb_mode & RG_AMB_BOTH_STRANDS)))
        return fail(RG_ERR_ARG, "RG_AMB_STRAND_VOTE picks the first strand of RG_AMB_BOTH_STRANDS: it is valid only together with that "
                                "bit (amb_mode = 12), in the pathwise modes");
    if ((p->amb_mode & RG_AMB_BOTH_STRANDS) && is_poa(mode))
        return fail(RG_ERR_ARG, "RG_AMB_BOTH_STRANDS applies to the pathwise modes only: the POA modes align both strands through "
                                "rg_stream_opts.amb_strand (`-s true`, main.rs:82,132,188,229)");
    if ((p->amb_mode & 3) && !is_poa(mode)) return fail(RG_ERR_ARG, "amb_mode bits 0 and 1 apply to the POA modes only (main.rs:82,132,188,229)");
    if (path_gap || path_edit) {
        // what the plan of these modes refuses (amb_mode bits, reads over the family's limit, scores outside the i32 budget; the
        // edit-distance modes: anything but unit costs) is host arithmetic on the longest read: answered here, before a device is needed
        int64_t longest = 0;
        for (int64_t r = 0; r < nreads; ++r) longest = std::max<int64_t>(longest, read_off[r + 1] - read_off[r]);
        PathPlan plan;
        const HostGraph& h = g->h;
        const int prc = plan_pathwise(*p, PathPlanInput{h.P, h.L, h.fslots, h.rslots, h.max_path_rows, (int)std::min<int64_t>(longest, INT32_MAX)},
                                      options(), 0, plan);
        if (prc) return prc;
    }
    GraphTables* gt = nullptr;
    int rc = upload_graph(const_cast<rg_graph*>(g), &gt);   // per-device tables, under the graph's mutex
    if (rc) return rc;
    auto b = std::make_unique<rg_batch>();
    b->g = g;
    b->gt = gt;
    b->p = *p;
    // a both-strands family aligns both strands whatever the bit says: from here on the handle IS a both-strands handle (the
    // ops_stride, the strand buffers, the strand of a record)
    if (gap_mode(mode).family->both_strands || edit_strands_mode(mode).valid) b->p.amb_mode |= RG_AMB_BOTH_STRANDS;
    HIPCHK(hipGetDevice(&b->dev));
    {
        // the handle's stream at the highest priority: it carries the small kernels; the pathwise sweeps run on a low-priority
        // stream of their own (rg_path_driver.hip, SWEEPS ON A LOW-PRIORITY STREAM)
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&b->stream, hipStreamNonBlocking, greatest) != hipSuccess)
            HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    }
    b->timer.stream = b->stream;
    if (is_poa(mode) && (rc = poa_upload_tables(b.get()))) return rc;
    if ((rc = load_reads(b.get(), reads, read_off, nreads))) return rc;
    *out = b.release();
    return RG_OK;
}

static const char* kNoDevBuffers = "results-only handle (a tile of a stream / rg_multi): it has no device buffers";
static const char* kNoReads = "the handle holds no read set (a previous rg_batch_set_reads failed)";

int32_t rg_batch_set_reads(rg_batch* b, const char* reads, const int64_t* read_off, int64_t nreads) {
    if (!b || !reads || !read_off || nreads < 1) return fail(RG_ERR_ARG, "null/empty argument");
    if (b->dev < 0) return fail(RG_ERR_ARG, kNoDevBuffers);
    DevGuard dg(b->dev);            // the handle is bound to the device it was created on; the caller's device is restored
    HIPCHK(dg.err);
    return load_reads(b, reads, read_off, nreads);
}

int32_t rg_batch_run(rg_batch* b) {
    if (!b) return fail(RG_ERR_ARG, "null batch");
    if (b->dev < 0) return fail(RG_ERR_ARG, kNoDevBuffers);
    if (!b->valid) return fail(RG_ERR_ARG, kNoReads);
    b->fetched = false;
    DevGuard dg(b->dev);
    HIPCHK(dg.err);
    // one rule for the statistics: reset here, once; every pass of either driver adds (rg_path_args.hpp)
    reset_stats(b->stats);
    b->timer.reset();
    b->timer.spin = b->spin_wait;
    return is_poa(b->p.mode) ? run_poa(b) : rg_run_pathwise(b);
}

int32_t rg_batch_fetch(rg_batch* b) {
    if (!b) return fail(RG_ERR_ARG, "null batch");
    if (b->dev < 0) return fail(RG_ERR_ARG, kNoDevBuffers);
    if (!b->valid) return fail(RG_ERR_ARG, kNoReads);
    DevGuard dg(b->dev);
    HIPCHK(dg.err);
    b->rec.resize(b->nreads);
    HIPCHK(hipMemcpy(b->rec.data(), b->d_rec.p, sizeof(DevRecord) * b->nreads, hipMemcpyDeviceToHost));
    b->ops.resize((size_t)b->nreads * b->ops_stride);
    HIPCHK(hipMemcpy(b->ops.data(), b->d_ops.p, b->ops.size(), hipMemcpyDeviceToHost));
    if (is_poa(b->p.mode)) {
        b->oprows.resize((size_t)b->nreads * b->ops_stride);
        HIPCHK(hipMemcpy(b->oprows.data(), b->d_oprows.p, b->oprows.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    b->fetched = true;
    return RG_OK;
}

void rg_batch_destroy(rg_batch* b) { rg_batch_destroy_impl(b); }
int64_t rg_batch_size(const rg_batch* b) { return b ? b->nreads : 0; }

uint32_t rg_result_status(const rg_batch* b, int64_t i) {
    if (!b || !b->fetched || i < 0 || i >= b->nreads) return RG_READ_WOULD_PANIC;
    return public_status(b->rec[i].status);
}
int32_t rg_result_score(const rg_batch* b, int64_t i) {
    if (!b || !b->fetched || i < 0 || i >= b->nreads) return 0;
    return b->rec[i].score;
}

// GAFStruct of read i (false: the reference produces none — score-only call, or it panics on this read)
static bool build_fields(const rg_batch* b, int64_t i, const char* name, GafFields& out) {
    const DevRecord& d = b->rec[i];
    if (d.status & ST_NO_RECORD) return false;
    ReadRecord r;
    fill_record(b, i, r);
    std::string read((size_t)(b->off[i + 1] - b->off[i]), 'N');
    const bool rev = reverse_won(b, i);
    std::vector<uint8_t> rcbuf;
    const uint8_t* rcodes = rev ? revcomp_codes(b, i, rcbuf) : b->codes + (size_t)b->off[i];
    for (size_t k = 0; k < read.size(); ++k) read[k] = "ACGTN"[rcodes[k]];
    std::string nm = name ? name : "";
    switch (b->p.mode) {
        case RG_MODE_GLOBAL_POA: out = fields_m0_simd(b->g->h, read, nm, r, b->p.amb_mode); break;
        case RG_MODE_GLOBAL_POA_SCALAR:
        case RG_MODE_GAP_POA:
        case RG_MODE_LOCAL_POA:
        case RG_MODE_LOCAL_POA_SCALAR:
        case RG_MODE_GAP_LOCAL_POA: out = fields_poa_banded(b->g->h, read, nm, r, b->p.amb_mode); break;
        default: out = fields_pathwise(b->g->h, read, nm, r, b->p.mode, rev ? '-' : '+'); break;
    }
    return true;
}

int64_t rg_result_gaf(const rg_batch* b, int64_t i, const char* name, int64_t seq_index, char* buf, int64_t cap) {
    if (!b || !b->fetched || i < 0 || i >= b->nreads) return fail(RG_ERR_ARG, "result not available");
    std::string out;
    append_gaf(b, i, name, seq_index, out);
    if (buf && (int64_t)out.size() + 1 <= cap) memcpy(buf, out.c_str(), out.size() + 1);
    return (int64_t)out.size();
}

int32_t rg_result_fields(const rg_batch* b, int64_t i, rg_gaf_fields* out, uint64_t* path_ids, int64_t path_cap, char* comments,
                         int64_t comments_cap) {
    if (!b || !b->fetched || i < 0 || i >= b->nreads || !out) return fail(RG_ERR_ARG, "result not available");
    memset(out, 0, sizeof *out);
    GafFields f;
    if (!build_fields(b, i, "", f)) { out->strand = ' '; return RG_OK; }
    out->has_record = 1;
    out->empty = f.empty ? 1 : 0;
    out->query_length = f.qlen; out->query_start = f.qstart; out->query_end = f.qend;
    out->strand = f.strand;
    out->path_length = f.plen; out->path_start = f.pstart; out->path_end = f.pend;
    out->residue_matches_number = f.residues;
    out->n_path_ids = (int64_t)f.path.size();
    out->comments_len = (int64_t)f.comments.size();
    out->warning = f.pre.empty() ? 0 : (f.empty ? RG_READ_BAND_NOT_ENOUGH : RG_READ_BAND_WARNING);
    if (path_ids && path_cap >= (int64_t)f.path.size()) for (size_t k = 0; k < f.path.size(); ++k) path_ids[k] = f.path[k];
    if (comments && comments_cap >= (int64_t)f.comments.size() + 1) memcpy(comments, f.comments.c_str(), f.comments.size() + 1);
    return RG_OK;
}

int64_t rg_batch_format_all(const rg_batch* b, const char* const* names, int64_t seq_index_base, char* buf, int64_t cap,
                            int32_t nthreads) {
    if (!b || !b->fetched) return fail(RG_ERR_ARG, "result not available");
    std::string out;
    format_batch(b, names, 0, seq_index_base, nthreads, out, nullptr);
    const int64_t total = (int64_t)out.size();
    if (buf && total + 1 <= cap) memcpy(buf, out.c_str(), out.size() + 1);
    return total;
}

uint64_t rg_batch_cell_updates(const rg_batch* b) { return b ? b->cells : 0; }
uint64_t rg_batch_cell_updates_performed(const rg_batch* b) { return b ? b->cells_performed : 0; }
int32_t rg_batch_kernel_count(const rg_batch* b) { return b ? (int32_t)b->stats.size() : 0; }
const char* rg_batch_kernel_name(const rg_batch* b, int32_t k) { return b->stats[k].name.c_str(); }
double rg_batch_kernel_ms(const rg_batch* b, int32_t k) { return b->stats[k].ms; }
int64_t rg_batch_kernel_launches(const rg_batch* b, int32_t k) { return b->stats[k].launches; }

int32_t rg_align_batch(const rg_graph* g, const rg_params* p, const char* reads, const int64_t* read_off, int64_t nreads,
                       rg_batch** out) {
    rg_batch* b = nullptr;
    int rc = rg_batch_create(g, p, reads, read_off, nreads, &b);
    if (rc) return rc;
    if ((rc = rg_batch_run(b)) || (rc = rg_batch_fetch(b))) { rg_batch_destroy(b); return rc; }
    *out = b;
    return RG_OK;
}

}  // extern "C"
