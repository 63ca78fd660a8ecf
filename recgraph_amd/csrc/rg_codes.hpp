// Codes shared by the kernels and the host formatter (no HIP here: rg_gaf.cpp is part of the host-only sanitizer build).
#pragma once
#include <stdint.h>

namespace rg {

// traceback op codes (one byte per op, walk order)
enum : uint8_t { OP_D = 1, OP_U = 2, OP_L = 3, OP_CONT = 0x80 };

// status bits mirror include/recgraph_hip.h
enum : uint32_t { ST_BAND_WARNING = 1u, ST_BAND_NOT_ENOUGH = 2u, ST_WOULD_PANIC = 4u, ST_BAD_BASE = 8u, ST_UNALIGNED = 16u, ST_OVERFLOW = 0x100u };
// a read with one of these has no record: no ops, no text, score 0 (ST_UNALIGNED: -m 12 only, where it is no error)
constexpr uint32_t ST_NO_RECORD = ST_BAD_BASE | ST_WOULD_PANIC | ST_UNALIGNED;

constexpr int WAVE = 64;

// scoring table by value in kernel arguments: t[a*6+b], alphabet "ACGTN-" -> 0..5
struct DevScores {
    int t[36];
};

}  // namespace rg

// PATH RETIREMENT of k_sweep16: the sweeps look for hopeless paths every 2^RG_SWEEP16_RETIRE_SHIFT step records;
// the kernel and the builder of the tables that go with it (rg_steps.cpp) share the constant
#ifndef RG_SWEEP16_RETIRE_SHIFT
#define RG_SWEEP16_RETIRE_SHIFT 8
#endif

// REGISTER RUNS of k_sweep16's record variants: a run keeps the rows of at most this many paths in registers.  The builder of the
// split step tables (rg_steps.cpp) moves a group behind a run as its TAIL only when the kernel handles that run as a register
// run, so both sides use this constant (the kernel ties its KRUN to it with a static_assert)
namespace rg {
constexpr int RG_SWEEP16_RUN_PATHS = 4;
}  // namespace rg
