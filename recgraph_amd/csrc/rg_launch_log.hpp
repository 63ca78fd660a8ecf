// Launch log (RG_LAUNCH_LOG / rg_set_option("launch_log")): which compiled kernel a launcher dispatched.
//
// Every launcher launches through RG_LAUNCH and returns the name of the instantiation it launched, spelled as the demangled
// symbol of the code object without its parameter list (what tools/kernel_resources.py report() prints:
// "rg::k_sweep16<16, 0, true, false, false>", "rg::k_pick").  The macro takes the template arguments ONCE and uses that one
// token list for the launch and for the name, inside the `case` / `if` that dispatches: the log cannot state another rule
// than the dispatch.  The drivers hand the name to the handle's timer (KernelTimer::run, KernelTimer::inst: rg_kernel_timer.hpp), which
// turns it into an "inst:<name>" pseudo-entry of the batch's KernelStats (ms 0, launches counted) when the option is on and drops it
// otherwise; a launcher that returns null launched nothing, and the timer reports RG_ERR_ARG.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

namespace rg {

template <typename T>
inline void inst_arg(std::string& s, T v) {
    if (s.back() != '<') s += ", ";
    if constexpr (std::is_same_v<T, bool>) s += v ? "true" : "false";
    else s += std::to_string(v);
}
// K: the kernel itself (one name per instantiation: its function-local string is built on the first launch); V: its template arguments
template <auto K, auto... V>
const char* inst_label(const char* kernel) {
    static const std::string name = [&] {
        std::string s = kernel;
        if constexpr (sizeof...(V) > 0) {
            s += '<';
            (inst_arg(s, V), ...);
            s += '>';
        }
        return s;
    }();
    return name.c_str();
}

#define RG_TARGS_(...) __VA_ARGS__
// RG_LAUNCH(k_layer, (16, true), grid, block, lds bytes, stream, kernel arguments...): launches rg::k_layer<16, true> and
// RETURNS "rg::k_layer<16, true>" from the launcher (every template argument is spelled out, defaulted ones too: the symbol
// carries them all); RG_LAUNCH0: a kernel that is no template
#define RG_LAUNCH(K, TA, ...)                                                        \
    do {                                                                             \
        hipLaunchKernelGGL((K<RG_TARGS_ TA>), __VA_ARGS__);                          \
        return ::rg::inst_label<&K<RG_TARGS_ TA>, RG_TARGS_ TA>("rg::" #K);          \
    } while (0)
#define RG_LAUNCH0(K, ...)                                                           \
    do {                                                                             \
        hipLaunchKernelGGL(K, __VA_ARGS__);                                          \
        return ::rg::inst_label<&K>("rg::" #K);                                      \
    } while (0)

// RG_SWITCH_C((4, 8, 16, 32), k_layer, (, false), grid, block, lds bytes, stream, kernel arguments...): the dispatch on the columns per
// lane, inside a launcher whose parameter `C` holds them.  One RG_LAUNCH per listed value (three or four of them) with that value as
// the kernel's first template argument and TAIL — in parentheses, with its leading comma: (, true) / () — behind it; a C outside the
// list launches nothing and returns null (the timer then reports RG_ERR_ARG).  The plan only produces listed values (plan_pathwise).
#define RG_SWITCH_C_CASE_(K, TAIL, c, ...) case c: RG_LAUNCH(K, (c RG_TARGS_ TAIL), __VA_ARGS__);
#define RG_SWITCH_C_3_(K, TAIL, c0, c1, c2, ...) \
    RG_SWITCH_C_CASE_(K, TAIL, c0, __VA_ARGS__) RG_SWITCH_C_CASE_(K, TAIL, c1, __VA_ARGS__) RG_SWITCH_C_CASE_(K, TAIL, c2, __VA_ARGS__)
#define RG_SWITCH_C_4_(K, TAIL, c0, c1, c2, c3, ...) \
    RG_SWITCH_C_3_(K, TAIL, c0, c1, c2, __VA_ARGS__) RG_SWITCH_C_CASE_(K, TAIL, c3, __VA_ARGS__)
#define RG_SWITCH_C_COUNT_(a, b, c, d, N, ...) N
#define RG_SWITCH_C_PICK_(...) RG_SWITCH_C_COUNT_(__VA_ARGS__, RG_SWITCH_C_4_, RG_SWITCH_C_3_, , )
#define RG_SWITCH_C_APPLY_(M, ...) M(__VA_ARGS__)
#define RG_SWITCH_C(CS, K, TAIL, ...)                                                                  \
    do {                                                                                               \
        switch (C) {                                                                                   \
            RG_SWITCH_C_APPLY_(RG_SWITCH_C_PICK_ CS, K, TAIL, RG_TARGS_ CS, __VA_ARGS__)               \
            default: return nullptr;                                                                   \
        }                                                                                              \
    } while (0)

}  // namespace rg
