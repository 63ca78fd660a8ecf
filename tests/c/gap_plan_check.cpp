// CPU check of the plan of the affine-gap pathwise modes (-m 6 / -m 7; recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise): columns
// per lane on both sides of every boundary, the refusals, the bytes per read.  Built and run by tests/test_pathwise_gap_cpu.py.
#include "plan_check_common.hpp"

using namespace gap_check;

int main() {
    PathPlan q;
    const struct { int n, C, words; } routes[] = {{1, 4, 1}, {255, 4, 1}, {256, 8, 1}, {511, 8, 1}, {512, 16, 2}, {1023, 16, 2}, {1024, 32, 4}, {2047, 32, 4}};
    for (int mode : {RG_MODE_PATHWISE_GAP, RG_MODE_PATHWISE_GAP_SEMI})
        for (const auto& r : routes) {
            CHECK(run(params(mode), shape(r.n), q) == RG_OK);
            CHECK(q.gap && q.mode == RG_MODE_PATHWISE_GAP && q.semi == (mode == RG_MODE_PATHWISE_GAP_SEMI));
            CHECK(q.C == r.C && q.nwv == 1 && q.wpad == 64 * r.C && q.gap_words == r.words);
            CHECK(r.n + 1 <= 64 * q.C && (q.C == 4 || r.n + 1 > 32 * q.C));
            // 4 bits per cell of the picked path (rows + the unused layer of row 0), and the per-read state: nothing else in HBM
            CHECK(q.gdirs_stride == 1001ll * r.words * 64);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + sizeof(ReadState));
            CHECK(q.per_read_all(1, 1, 1, 1) == q.per_read);
            CHECK(!q.use16 && !q.spec && !q.spec4 && !q.two_sweep && !q.use_rec && !q.retire && !q.dsel && !q.dsel4);
        }
    // refusals
    CHECK(run(params(RG_MODE_PATHWISE_GAP), shape(2048), q) == RG_ERR_ARG);
    CHECK(g_last_error.find("2047") != std::string::npos);
    CHECK(run(params(RG_MODE_PATHWISE_GAP, 1, -2), shape(100), q) == RG_ERR_ARG);
    CHECK(run(params(RG_MODE_PATHWISE_GAP_SEMI, -4, 1), shape(100), q) == RG_ERR_ARG);
    CHECK(run(params(RG_MODE_PATHWISE_GAP, 0, 0), shape(100), q) == RG_OK);
    for (int bit : {1, 2, 4, 8, 12}) {
        rg_params p = params(RG_MODE_PATHWISE_GAP);
        p.amb_mode = bit;
        CHECK(run(p, shape(100), q) == RG_ERR_ARG);
    }
    // capacity: (rows + n) * max(|sc|, |o + e|) must stay below 2^28: 2000 * 134217 < 2^28 <= 2000 * 134218
    CHECK(run(params(RG_MODE_PATHWISE_GAP, -134215, -2), shape(1000), q) == RG_OK);
    CHECK(run(params(RG_MODE_PATHWISE_GAP, -134216, -2), shape(1000), q) == RG_ERR_CAPACITY);
    {
        rg_params p = params(RG_MODE_PATHWISE_GAP_SEMI);
        p.scores[0] = 134218;
        CHECK(run(p, shape(1000), q) == RG_ERR_CAPACITY);
        p.scores[0] = 134217;
        CHECK(run(p, shape(1000), q) == RG_OK);
        p.scores[0 * 6 + 5] = 1 << 30;      // the '-' entries are not read
        CHECK(run(p, shape(1000), q) == RG_OK);
    }
    // the other pathwise modes do not take the gap route
    CHECK(run(params(RG_MODE_PATHWISE), shape(150), q) == RG_OK && !q.gap && q.mode == RG_MODE_PATHWISE);
    return finish("gap plan ok");
}
