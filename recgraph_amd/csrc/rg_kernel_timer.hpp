// The one kernel timer of a batch handle: HIP-event timing per kernel name and the launch log's labels (rg_launch_log.hpp).
// rg_batch owns it; the POA driver, the strand orchestration and the pathwise driver (its nested second pass too) record into
// it by reference.  Events come from ONE cursor that only collect() rewinds, and collect() takes everything recorded so far:
// a launch that is recorded but not yet collected (the vote kernels in front of pass A) never shares events with what follows.
#pragma once
#include <vector>

#include "rg_path_args.hpp"

namespace rg {

struct KernelTimer {
    hipStream_t stream = nullptr;      // the handle's stream: every timed launch goes there
    bool spin = false;                 // the handle waits with hipStreamSynchronize (rg_stream_opts.spin_wait)
    std::vector<hipEvent_t> ev;        // the pool: recorded launch k is bracketed by ev[2k], ev[2k + 1]
    hipEvent_t done_ev = nullptr;      // end-of-work marker polled by wait_stream_sleeping (no spinning host thread per handle)
    std::vector<const char*> pend;     // names of the recorded launches, in event order: its size is the cursor
    std::vector<const char*> insts;    // what the launchers said they launched (the launch log is on)

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
    int inst(const char* label, const char* what = "an untimed launch") {
        if (!label) return fail(RG_ERR_ARG, std::string("no kernel is compiled for this launch: ") + what);
        if (options().launch_log) insts.push_back(label);
        return RG_OK;
    }
    // launch() enqueues one kernel on `stream` and returns its launcher's label; its device time goes to `name` (a literal)
    template <typename F>
    int run(const char* name, F&& launch) {
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
        return inst(label, name);
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
        for (const char* l : insts) add_stat(stats, std::string("inst:") + l, 0, 1);
        insts.clear();
        return RG_OK;
    }
};

}  // namespace rg
