// CPU check of the plan of the local affine-gap pathwise mode (-m 12; recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise): the gap
// route with the `local` flag, columns per lane on both sides of every boundary, the refusals, the bytes per read — and that modes 6
// and 7 keep `local` off.  Built and run by tests/test_pathwise_gap_local_cpu.py.
#include "plan_check_common.hpp"

using namespace gap_check;

int main() {
    PathPlan q;
    const int M = RG_MODE_PATHWISE_GAP_LOCAL;
    CHECK(M == 12);
    const struct { int n, C, words; } routes[] = {{1, 4, 1}, {255, 4, 1}, {256, 8, 1}, {511, 8, 1}, {512, 16, 2}, {1023, 16, 2}, {1024, 32, 4}, {2047, 32, 4}};
    for (const auto& r : routes) {
        CHECK(run(params(M), shape(r.n), q) == RG_OK);
        CHECK(q.gap && q.local && !q.semi && q.mode == RG_MODE_PATHWISE_GAP);
        CHECK(q.C == r.C && q.nwv == 1 && q.wpad == 64 * r.C && q.gap_words == r.words);
        CHECK(r.n + 1 <= 64 * q.C && (q.C == 4 || r.n + 1 > 32 * q.C));
        // the same buffers as -m 6 / -m 7: 4 bits per cell of the picked path and the per-read state
        CHECK(q.gdirs_stride == 1001ll * r.words * 64);
        CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + sizeof(ReadState));
        CHECK(q.per_read_all(1, 1, 1, 1) == q.per_read);
        CHECK(!q.use16 && !q.spec && !q.spec4 && !q.two_sweep && !q.use_rec && !q.retire && !q.dsel && !q.dsel4);
        // ... and modes 6 / 7 plan what they planned, without the flag
        for (int mode : {RG_MODE_PATHWISE_GAP, RG_MODE_PATHWISE_GAP_SEMI}) {
            PathPlan g;
            CHECK(run(params(mode), shape(r.n), g) == RG_OK);
            CHECK(g.gap && !g.local && g.C == q.C && g.gap_words == q.gap_words && g.gdirs_stride == q.gdirs_stride && g.per_read == q.per_read);
        }
    }
    // refusals
    CHECK(run(params(M), shape(2048), q) == RG_ERR_ARG);
    CHECK(g_last_error.find("2047") != std::string::npos && g_last_error.find("-m 12") != std::string::npos);
    CHECK(run(params(RG_MODE_PATHWISE_GAP), shape(2048), q) == RG_ERR_ARG);
    CHECK(g_last_error.find("-m 6 / -m 7") != std::string::npos);
    CHECK(run(params(M, 1, -2), shape(100), q) == RG_ERR_ARG);
    CHECK(run(params(M, -4, 1), shape(100), q) == RG_ERR_ARG);
    CHECK(run(params(M, 0, 0), shape(100), q) == RG_OK);
    for (int bit : {1, 2, 4, 8, 12}) {
        rg_params p = params(M);
        p.amb_mode = bit;
        CHECK(run(p, shape(100), q) == RG_ERR_ARG);
    }
    // capacity: (rows + n) * max(|sc|, |o + e|) must stay below 2^28: 2000 * 134217 < 2^28 <= 2000 * 134218
    CHECK(run(params(M, -134215, -2), shape(1000), q) == RG_OK);
    CHECK(run(params(M, -134216, -2), shape(1000), q) == RG_ERR_CAPACITY);
    {
        rg_params p = params(M);
        p.scores[0] = 134218;
        CHECK(run(p, shape(1000), q) == RG_ERR_CAPACITY);
        p.scores[0] = 134217;
        CHECK(run(p, shape(1000), q) == RG_OK);
        p.scores[0 * 6 + 5] = 1 << 30;      // the '-' entries are not read
        CHECK(run(p, shape(1000), q) == RG_OK);
    }
    CHECK(run(params(RG_MODE_PATHWISE), shape(150), q) == RG_OK && !q.gap && !q.local);
    return finish("gap local plan ok");
}
