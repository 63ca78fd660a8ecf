// CPU check of the plan of the both-strands affine-gap pathwise modes (-m 26 / -m 27 / -m 32; recgraph_amd/csrc/rg_path_plan.cpp:
// plan_pathwise).  A batch of these modes runs two passes, each planned by its own longest read: whatever amb_mode the mode admits,
// the plan of a pass IS the plan of the long flavour (mode - 10) at that pass's longest read — so pass A may run the striped kernels
// and pass B the base ones, or the other way round, and the per-read byte count of each pass is the one its own kernels need.  Also
// the amb_mode values the modes admit and refuse.  Built and run by tests/test_pathwise_gap_strands_cpu.py.
#include <cstdio>
#include <cstring>

#include "rg_path_plan.hpp"

using namespace rg;

static int failures = 0;
#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { ++failures; fprintf(stderr, "gap_strands_plan_check.cpp:%d: %s\n", __LINE__, #c); } \
    } while (0)

static rg_params params(int mode, int amb = 0, int o = -4, int e = -2) {
    rg_params p;
    memset(&p, 0, sizeof p);
    p.mode = mode;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) p.scores[i * 6 + j] = i == j ? 2 : (i == 5 || j == 5) ? -8 : -4;
    p.scores[4 * 6 + 4] = -4;
    p.scores[5 * 6 + 5] = RG_SCORE_MISSING;
    p.gap_open = o;
    p.gap_ext = e;
    p.amb_mode = amb;
    return p;
}
static const int kPaths = 6;
static PathPlanInput shape(int max_n, int rows = 1000) { return PathPlanInput{kPaths, rows + 2, 1400, 1400, rows, max_n}; }
static int run(const rg_params& p, const PathPlanInput& in, PathPlan& q) {
    Options o;
    return plan_pathwise(p, in, o, 0, q);
}
static bool same_plan(const PathPlan& a, const PathPlan& b) {
    return a.gap == b.gap && a.mode == b.mode && a.semi == b.semi && a.local == b.local && a.C == b.C && a.nwv == b.nwv && a.wpad == b.wpad &&
           a.gap_words == b.gap_words && a.gdirs_stride == b.gdirs_stride && a.gbnd_stride == b.gbnd_stride && a.gdbnd_stride == b.gdbnd_stride &&
           a.per_read == b.per_read && a.maxmatch == b.maxmatch && a.per_read_all(1, 1, 1, 1) == b.per_read_all(1, 1, 1, 1);
}

int main() {
    CHECK(RG_MODE_PATHWISE_GAP_STRANDS == 26 && RG_MODE_PATHWISE_GAP_SEMI_STRANDS == 27 && RG_MODE_PATHWISE_GAP_LOCAL_STRANDS == 32);
    CHECK(RG_MODE_PATHWISE_GAP_STRANDS == RG_MODE_PATHWISE_GAP + 20 && RG_MODE_PATHWISE_GAP_SEMI_STRANDS == RG_MODE_PATHWISE_GAP_SEMI + 20 &&
          RG_MODE_PATHWISE_GAP_LOCAL_STRANDS == RG_MODE_PATHWISE_GAP_LOCAL + 20);
    for (int M : {26, 27, 32}) {
        CHECK(path_gap_strands_mode(M) && path_gap_long_mode(M) && path_gap_base_mode(M) == M - 20);
        CHECK(!path_gap_strands_mode(M - 10) && !path_gap_strands_mode(M - 20) && path_gap_base_mode(M - 10) == M - 20);
        const bool local = M == 32;
        PathPlan q, g;
        // every pass of the mode, whatever its longest read and whatever amb_mode says: the plan of the long flavour at that length
        for (int amb : {0, 4, 12}) {
            if (local && amb == 12) continue;
            for (int n : {1, 150, 255, 256, 2047, 2048, 2100, 4096, 16383}) {
                CHECK(run(params(M, amb), shape(n), q) == RG_OK);
                CHECK(run(params(M - 10), shape(n), g) == RG_OK);
                CHECK(same_plan(q, g));
                CHECK(q.gap && q.semi == (M == 27) && q.local == local && q.nwv == (n + 2048) / 2048);
            }
        }
        // two passes of one batch in different length classes, both ways round: one on the base kernels, one striped, each with the
        // bytes its own kernels take per read (the striped pass counts S stripes of direction words and both boundary buffers)
        PathPlan a, b;
        CHECK(run(params(M, 4), shape(2100), a) == RG_OK && run(params(M, 4), shape(150), b) == RG_OK);
        CHECK(a.nwv == 2 && a.C == 32 && b.nwv == 1 && b.C == 4);
        CHECK(a.per_read == (size_t)2 * 1001 * 4 * 64 * 4 + (size_t)(2 * 1001 * kPaths + 2 * 1001) * 4 + sizeof(ReadState));
        CHECK(b.per_read == (size_t)1001 * 1 * 64 * 4 + sizeof(ReadState) && b.gbnd_stride == 0 && b.gdbnd_stride == 0);
        CHECK(b.per_read < a.per_read);
        // a pass can never be longer than the batch: the longest read of pass B is one of the batch's reads, so the batch's refusals
        // (answered by rg_batch_create with the batch's longest read) cover both passes
        CHECK(run(params(M), shape(16384), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("16383") != std::string::npos);
        CHECK(run(params(M, 4, 1, -2), shape(100), q) == RG_ERR_ARG);
        CHECK(run(params(M, 4, -4, 1), shape(5000), q) == RG_ERR_ARG);
        CHECK(run(params(M, 0, -16775, -2), shape(15000), q) == RG_OK);
        CHECK(run(params(M, 0, -16776, -2), shape(15000), q) == RG_ERR_CAPACITY);
        // amb_mode: 0, 4 and (26, 27) 12; nothing else
        for (int amb : {1, 2, 3, 5, 6, 8, 9, 13, 16, 20, 28, -1}) {
            CHECK(run(params(M, amb), shape(100), q) == RG_ERR_ARG);
            CHECK(run(params(M, amb), shape(3000), q) == RG_ERR_ARG);
        }
        CHECK(run(params(M, 12), shape(100), q) == (local ? RG_ERR_ARG : RG_OK));
        if (local) CHECK(g_last_error.find("hopeless") != std::string::npos);
        // the modes without the strands keep refusing every bit
        for (int amb : {4, 12}) {
            CHECK(run(params(M - 10, amb), shape(100), q) == RG_ERR_ARG);
            CHECK(run(params(M - 20, amb), shape(100), q) == RG_ERR_ARG);
        }
    }
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    puts("gap strands plan ok");
    return 0;
}
