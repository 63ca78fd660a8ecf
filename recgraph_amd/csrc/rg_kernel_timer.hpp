// The one kernel timer of a batch handle: HIP-event timing per kernel name and the launch log's labels (rg_launch_log.hpp).
// rg_batch owns it; the POA driver, the strand orchestration and the pathwise driver (its nested second pass too) record into
// it by reference.  Events come from ONE cursor that only collect() rewinds, and collect() takes everything recorded so far:
// a launch that is recorded but not yet collected (the vote kernels in front of pass A) never shares events with what follows.
#pragma once
#include <utility>
#include <vector>

#include "rg_path_args.hpp"

namespace rg {

struct KernelTimer {
    hipStream_t stream = nullptr;      // the handle's stream: every timed launch goes there
    bool spin = false;                 // the handle waits with hipStreamSynchronize (rg_stream_opts.spin_wait)
    std::vector<hipEvent_t> ev;        // the pool: recorded launch k is bracketed by ev[2k], ev[2k + 1]
    hipEvent_t done_ev = nullptr;      // end-of-work marker polled by wait_stream_sleeping (no spinning host thread per handle)
    std::vector<const char*> pend;     // names of the recorded launches, in event order: its size is the cursor
    std::vector<std::pair<const char*, const char*>> insts;    // (log family, what the launcher said it launched) (the launch log is on)

    KernelTimer() = default;
    KernelTimer(const KernelTimer&) = delete;
    ~KernelTimer() {
        for (auto e : ev) (void)hipEventDestroy(e);
        if (done_ev) (void)hipEventDestroy(done_ev);
    }
    // a new run of the handle: whatever a failed run left recorded is dropped
    void reset() { pend.clear(); insts.clear(); }
    // A launcher's result: the instantiation it dispatched (null: it launched nothing — an argument block no kernel is compiled
    // for).  Called directly for a launch that is not timed.
    // family: the prefix of the pseudo-entry.  "inst:" is the launch log of the kernels of csrc/*.hip: written only when the option
    // is on, and tests/kernel_matrix.py accounts for every such entry of its cases.  `always`: a family that is reported whatever the
    // option says — the windowed layer kernels (layer_window/, a directory with a matrix of its own, launched by those same cases) say
    // which instantiation served a batch the way the driver says how many reads fell back: as a "mem:" pseudo-statistic.
    int inst(const char* label, const char* what = "an untimed launch", const char* family = "inst:", bool always = false) {
        if (!label) return fail(RG_ERR_ARG, std::string("no kernel is compiled for this launch: ") + what);
        if (always || options().launch_log) insts.push_back({family, label});
        return RG_OK;
    }
    // launch() enqueues one kernel on `stream` and returns its launcher's label; its device time goes to `name` (a literal)
    template <typename F>
    int run(const char* name, F&& launch, const char* family = "inst:", bool always = false) {
        const size_t used = 2 * pend.size();
        while (ev.size() < used + 2) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            ev.push_back(e);
        }
        HIPCHK(hipEventRecord(ev[used], stream));
        const char* label = launch();
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[used + 1], stream));
        pend.push_back(name);
        return inst(label, name, family, always);
    }
    // waits for the stream (not when nothing timed is pending: labels need no device) and adds every recorded launch to `stats`
    int collect(KernelStats& stats) {
        if (!pend.empty()) {
            if (!done_ev) HIPCHK(hipEventCreateWithFlags(&done_ev, hipEventDisableTiming));
            HIPCHK((hipError_t)wait_stream_sleeping(stream, done_ev, spin));
            for (size_t k = 0; k < pend.size(); ++k) {
                float ms = 0;
                HIPCHK(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
                add_stat(stats, pend[k], ms, 1);
            }
            pend.clear();
        }
        for (const auto& l : insts) add_stat(stats, std::string(l.first) + l.second, 0, 1);
        insts.clear();
        return RG_OK;
    }
};

}  // namespace rg
