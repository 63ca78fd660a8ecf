// Argument blocks and work buffers of the pathwise (-m 4 / -m 8) kernels; device buffers, kernel statistics and the entry of
// their driver (rg_path_driver.hip) as the batch code (rg_abi.hip) sees them.
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
            (void)hipGetLastError();      // clears the sticky error: the handle stays usable after a failed call
            p = nullptr;
            if (oom && e == hipErrorOutOfMemory) *oom = true;
            return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? RG_ERR_NO_DEVICE : RG_ERR_HIP,
                        std::string("hipMalloc of ") + std::to_string(count * sizeof(T)) + " bytes: " + hipGetErrorString(e));
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
        if (e == hipSuccess) return RG_OK;
        (void)hipGetLastError();
        return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? RG_ERR_NO_DEVICE : RG_ERR_HIP,
                    std::string("hipMemcpy of ") + std::to_string(v.size() * sizeof(T)) + " bytes to the device: " + hipGetErrorString(e));
    }
};

// per-kernel device time of a batch; "mem:work_bytes_per_read" is a pseudo-entry of the pathwise driver (`ms` holds bytes)
struct KernelStat {
    std::string name;
    double ms = 0;
    long long launches = 0;
};
using KernelStats = std::vector<KernelStat>;
// adds (ms, count) to the entries called `name`, or appends one
inline void add_stat(KernelStats& stats, const std::string& name, double ms, long long count) {
    bool found = false;
    for (auto& st : stats)
        if (st.name == name) { st.ms += ms; st.launches += count; found = true; }
    if (!found) stats.push_back(KernelStat{name, ms, count});
}

struct PathWorkImpl;
struct PathWork {
    PathWorkImpl* impl = nullptr;
    bool spin_wait = false;     // the owning handle waits for the device with hipStreamSynchronize (rg_stream_opts.spin_wait)
    ~PathWork();
};

// One pathwise batch on `stream` (rg_path_driver.hip).  cells_out [2]: cell updates counted | performed; stats: cleared, then one
// entry per kernel name; spec_level: 0 from outside (the driver calls itself with 1 and 2 for reads whose speculative bound failed).
int path_driver_run(const HostGraph& h, const PathGraphDev& gd, const rg_params& p, PathWork& w, const uint8_t* d_reads,
                    const long long* d_off, const uint8_t* d_bad, int nreads, int max_n, DevRecord* d_rec, uint8_t* d_ops,
                    long long ops_stride, unsigned long long* d_cells, hipStream_t stream, size_t mem_budget,
                    unsigned long long* cells_out, KernelStats& stats, int spec_level);

// The 12-mer table of the paths that `w` holds for k_pick (built with the handle's other per-graph tables on first use):
// its keys and slot mask, for a vote that runs before the first path_driver_run (RG_AMB_STRAND_VOTE, rg_strand_vote.hip).
int path_driver_vote_table(const HostGraph& h, PathWork& w, const uint32_t** keys, unsigned* table_mask);

}  // namespace rg
