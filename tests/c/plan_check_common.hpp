// What the host-only plan programs of tests/c/ share: the CHECK macro with its failure count and closing line, the score matrix
// the reference's CLI builds, and (namespace gap_check) the parameters, graph shape and plan_pathwise call of the affine-gap checks.
#pragma once
#include <cstdio>
#include <cstring>

#include "rg_path_plan.hpp"

using namespace rg;

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

// "<n> failures" and 1, or `ok_line` and 0: what main returns
[[maybe_unused]] static int finish(const char* ok_line) {
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    puts(ok_line);
    return 0;
}

// zeroed parameters with score_matrix.rs:35-66 as rg_scores_match_mis builds it: match m, mismatch x, any pairing with '-' twice x
static rg_params score_params(int mode, int m = 2, int x = -4) {
    rg_params p;
    memset(&p, 0, sizeof p);
    p.mode = mode;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) p.scores[i * 6 + j] = i == j ? m : (i == 5 || j == 5) ? 2 * x : x;
    p.scores[4 * 6 + 4] = x;
    p.scores[5 * 6 + 5] = RG_SCORE_MISSING;
    return p;
}

namespace gap_check {
[[maybe_unused]] static rg_params params(int mode, int o = -4, int e = -2, int amb = 0) {
    rg_params p = score_params(mode);
    p.gap_open = o;
    p.gap_ext = e;
    p.amb_mode = amb;
    return p;
}
constexpr int kRows = 1000, kPaths = 6;
[[maybe_unused]] static PathPlanInput shape(int max_n, int rows = kRows, int paths = kPaths) { return PathPlanInput{paths, rows + 2, 1400, 1400, rows, max_n}; }
[[maybe_unused]] static int run(const rg_params& p, const PathPlanInput& in, PathPlan& q) {
    Options o;
    return plan_pathwise(p, in, o, 0, q);
}
}  // namespace gap_check
