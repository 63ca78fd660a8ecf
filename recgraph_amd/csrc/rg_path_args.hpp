// Argument blocks and work buffers of the pathwise (-m 4 / -m 8) kernels; device buffers, the HIP error check, kernel statistics
// and the entry of their driver (rg_path_driver.hip) as its callers (rg_strand_driver.hip, and the driver itself) see it.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "rg_device.hpp"
#include "rg_host.hpp"

namespace rg {

// flattened PathGraph (+ reverse PredHash, DP programs) in HBM
struct PathGraphDev {
    int L, P;
    const uint8_t* lnz;
    const uint64_t* row_mask;   // RG_PW words per row
    const int* knm;
    const int* dfs;
    const int* dfe;
    const int* fgoff;
    const int* rgoff;
    const GroupDesc* fgroups;
    const GroupDesc* rgroups;
    int fslots, rslots;
    const unsigned long long* node_id;
    const int* segfirst;
    const int* seglast;
    const int* eoff;
    const int* epred;
    const uint64_t* emask;      // RG_PW words per edge: path k is bit (k & 63) of word (k >> 6)
    const int* roff;
    const int* rsucc;
    const uint64_t* rmask;      // RG_PW words per edge
    const uint8_t* pnwp;
    const uint8_t* rnwp;
};

// A failed HIP call as a status code (the sticky error is cleared: the handle stays usable after a failed call); a lost or
// absent device is RG_ERR_NO_DEVICE in every driver.
inline int hip_fail(hipError_t e, const std::string& what) {
    (void)hipGetLastError();
    return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? RG_ERR_NO_DEVICE : RG_ERR_HIP, what + ": " + hipGetErrorString(e));
}
#define HIPCHK(x)                                             \
    do {                                                      \
        hipError_t e_ = (x);                                  \
        if (e_ != hipSuccess) return ::rg::hip_fail(e_, #x);  \
    } while (0)
// a status code other than RG_OK ends the calling function
#define RG_TRY(x)                 \
    do {                          \
        const int rc_ = (x);      \
        if (rc_) return rc_;      \
    } while (0)

// device buffer that only grows
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    size_t bytes() const { return p ? n * sizeof(T) : 0; }
    // oom (optional): set when hipMalloc itself reported hipErrorOutOfMemory — the one failure the pathwise driver answers with
    // smaller launches
    int alloc(size_t count, bool* oom = nullptr) {
        if (count <= n && p) return RG_OK;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        if (count == 0) count = 1;
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            if (oom && e == hipErrorOutOfMemory) *oom = true;
            return hip_fail(e, "hipMalloc of " + std::to_string(count * sizeof(T)) + " bytes");
        }
        n = count;
        return RG_OK;
    }
    template <typename U>       // (U: T, or a host struct of the same layout)
    int upload(const std::vector<U>& v) {
        static_assert(sizeof(U) == sizeof(T), "element sizes differ");
        int rc = alloc(v.size());
        if (rc) return rc;
        if (v.empty()) return RG_OK;
        const hipError_t e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e == hipSuccess ? RG_OK : hip_fail(e, "hipMemcpy of " + std::to_string(v.size() * sizeof(T)) + " bytes to the device");
    }
};

// Per-kernel device time of a batch.  rg_batch_run resets the handle's statistics once (reset_stats); every pass of every driver
// then ADDS into them (add_stat), so a name has one entry however many passes and chunks launched it.  Pseudo-entries:
//   "mem:work_bytes_per_read"            of the pathwise driver: `ms` holds bytes summed over the chunks, `launches` the chunks
//   "mem:layer_full_reads"               `ms` holds the READS the column window of the layers could not serve, summed over the chunks
//                                        (a count, not a time); `launches` the chunks
//   "mem:silent_rows" / "mem:run_rows"   of the record pipelines: `ms` holds the ROWS of the silent register runs / of all register
//                                        runs of both sweeps, summed over the chunks and passes
//   "mem:key_folds" / "mem:key_rows" / "mem:key_rows_hit" / "mem:key_folds_saved"
//                                        of the same sweeps: member folds into best-member keys on tails and general-path records /
//                                        rows closed there / those that wrote a record / folds left out for silent members; the
//                                        last is the sum of "mem:key_saved_gather" / "mem:key_saved_general" / "mem:key_saved_tail"
//   "mem:layer_window:<instantiation>"   the windowed layer kernel that ran: ms 0, launches counted, always on
//   "inst:<instantiation>"               the launch log (rg_launch_log.hpp)
struct KernelStat {
    std::string name;
    double ms = 0;
    long long launches = 0;
};
using KernelStats = std::vector<KernelStat>;
inline void add_stat(KernelStats& stats, const std::string& name, double ms, long long count) {
    for (auto& st : stats)
        if (st.name == name) { st.ms += ms; st.launches += count; return; }
    stats.push_back(KernelStat{name, ms, count});
}
// a new run (or a new attempt of a regrown one): the kernels keep their slots, the launch log's entries go (a run with the log off shows none)
inline void reset_stats(KernelStats& stats) {
    size_t n = 0;
    for (auto& s : stats)
        if (s.name.compare(0, 5, "inst:") != 0) stats[n++] = KernelStat{s.name, 0, 0};
    stats.resize(n);
}

struct PathWorkImpl;
struct PathWork {
    PathWorkImpl* impl = nullptr;
    ~PathWork();
};

// One pathwise batch (rg_path_driver.hip) is a CONTEXT, what every pass of a run shares, and a JOB, the reads of one pass and where
// their records go.  spec_level: 0 from outside (the driver calls itself with 1 and 2 for reads whose speculative bound failed,
// on work buffers and a cell counter of that pass's own).
struct KernelTimer;
struct PathCtx {
    const HostGraph& h;
    const PathGraphDev& gd;
    const rg_params& p;
    PathWork& w;
    hipStream_t stream;
    unsigned long long* d_cells;    // [2] device counters: cell updates counted | performed
    size_t mem_budget;              // bytes the work buffers of one chunk may take (0: three quarters of the free HBM)
    KernelTimer& T;
    KernelStats& stats;             // added to
    int spec_level;
};
struct PathJob {
    const uint8_t* reads;           // base codes at `off`
    const long long* off;           // [nreads + 1]
    const uint8_t* bad;             // [nreads]
    int nreads, max_n;
    DevRecord* rec;                 // out [nreads]
    uint8_t* ops;                   // out [nreads][ops_stride]
    long long ops_stride;
    // which part of the pipeline runs (PATH_STAGE_*, rg_path_plan.hpp): the whole of it, or — affine-gap pipelines, -m 76 / -m 77 /
    // -m 82 — the PICK stage (score pass + pick: `rec` gets status, score, path and end row, `ops` is not touched and may be null) or
    // the TRACE stage (`rec` holds such picks on entry, and the records and ops of the traceback on return)
    int stage = 0;
    // the same offsets on the host, or null.  -m 64 / -m 65 need them: a chunk's reads on the winning strand go into a buffer of the
    // chunk's own, at the input's offsets minus the chunk's first
    const long long* h_off = nullptr;
};
// cells [2]: the job's cell updates, counted | performed, are ADDED
int path_driver_run(const PathCtx& c, const PathJob& j, unsigned long long* cells);

// The 12-mer table of the paths that `w` holds for k_pick (built with the handle's other per-graph tables on first use):
// its keys and slot mask, for a vote that runs before the first path_driver_run (RG_AMB_STRAND_VOTE, rg_strand_vote.hip).
int path_driver_vote_table(const HostGraph& h, PathWork& w, const uint32_t** keys, unsigned* table_mask);

}  // namespace rg
