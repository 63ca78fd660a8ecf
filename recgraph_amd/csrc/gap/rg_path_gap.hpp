// Launchers of the affine-gap pathwise kernels (-m 6 / -m 7, gap/rg_path_gap.hip) and their argument block.  The driver
// (rg_path_driver.hip: enqueue_pathwise_gap) reaches the kernels through these host functions only.
#pragma once
#include "../rg_path_kernels.hpp"

namespace rg {

// the three rules of the family (the values are the template arguments of the striped kernels: k_gap_score_long<0> is global)
enum GapKind { GAP_GLOBAL = 0, GAP_SEMI = 1, GAP_LOCAL = 2 };

struct GapArgs {
    DevScores sc;
    const uint8_t* lnz;           // base code per graph row
    const uint8_t* reads;
    const long long* read_off;
    const uint8_t* bad;
    const int* poff; const int* prow;     // rows of every path in path order (build_path_rows, forward)
    int P;
    int o, e;                     // gap_open, gap_ext (both <= 0)
    ReadState* state;
    uint32_t* dirs;               // [reads][dirs_stride]: row t of the picked path at ((t + 1) * words + w) * 64 + lane
    long long dirs_stride;
    unsigned long long* cells;    // [2]: counted | performed
    DevRecord* rec;
    uint8_t* ops;
    long long ops_stride;
};

// C: columns per lane (4, 8, 16, 32; n + 1 <= 64 C for every read of the launch); semi: -m 7
const char* launch_gap_score(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s);
const char* launch_gap_pick(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s);
const char* launch_gap_dirs(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s);
const char* launch_gap_trace(const GapArgs& a, int nreads, int C, bool semi, hipStream_t s);

}  // namespace rg
