// CPU check of the plan of the long-read affine-gap pathwise modes (-m 16 / -m 17 / -m 22; recgraph_amd/csrc/rg_path_plan.cpp:
// plan_pathwise): up to 2047 bases the plan IS the base mode's; beyond, C = 32 and S = ceil((n + 1) / 2048) column stripes walked by
// one wave, with the direction words and the two boundary buffers counted per read; the refusals at the new lengths.  Built and run by
// tests/test_pathwise_gap_long_cpu.py.
#include "gap_mode_check.hpp"

using namespace gap_check;

int main() {
    CHECK(RG_MODE_PATHWISE_GAP_LONG == 16 && RG_MODE_PATHWISE_GAP_SEMI_LONG == 17 && RG_MODE_PATHWISE_GAP_LOCAL_LONG == 22);
    const int longs[] = {RG_MODE_PATHWISE_GAP_LONG, RG_MODE_PATHWISE_GAP_SEMI_LONG, RG_MODE_PATHWISE_GAP_LOCAL_LONG};
    for (int M : longs) {
        const int base = path_gap_base_mode(M);
        CHECK(is_family(M, GAP_FAM_LONG) && in_family(base, GAP_FAM_LONG) == M);
        PathPlan q, g;
        // up to 2047 bases: exactly the base mode's plan, and its kernels (nwv = 1)
        for (int n : {1, 255, 256, 1023, 1024, 2047}) {
            CHECK(run(params(M), shape(n), q) == RG_OK);
            CHECK(run(params(base), shape(n), g) == RG_OK);
            CHECK(q.gap && q.mode == RG_MODE_PATHWISE_GAP && q.nwv == 1);
            CHECK(q.C == g.C && q.nwv == g.nwv && q.wpad == g.wpad && q.gap_words == g.gap_words && q.gdirs_stride == g.gdirs_stride);
            CHECK(q.per_read == g.per_read && q.semi == g.semi && q.local == g.local && q.maxmatch == g.maxmatch);
            CHECK(q.gbnd_stride == 0 && q.gdbnd_stride == 0 && g.gbnd_stride == 0 && g.gdbnd_stride == 0);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + sizeof(ReadState));
        }
        CHECK(q.C == 32 && q.gdirs_stride == 1001ll * 4 * 64);
        CHECK(q.semi == (M == RG_MODE_PATHWISE_GAP_SEMI_LONG) && q.local == (M == RG_MODE_PATHWISE_GAP_LOCAL_LONG));
        // beyond: stripes of 2048 columns
        const struct { int n, S; } routes[] = {{2048, 2}, {4095, 2}, {4096, 3}, {8192, 5}, {16383, 8}};
        for (const auto& r : routes) {
            CHECK(run(params(M), shape(r.n), q) == RG_OK);
            CHECK(q.gap && q.mode == RG_MODE_PATHWISE_GAP && q.C == 32 && q.gap_words == 4);
            CHECK(q.nwv == r.S && q.wpad == r.S * 2048 && r.n + 1 <= q.wpad && r.n + 1 > q.wpad - 2048);
            CHECK(q.semi == (M == RG_MODE_PATHWISE_GAP_SEMI_LONG) && q.local == (M == RG_MODE_PATHWISE_GAP_LOCAL_LONG));
            CHECK(q.gdirs_stride == (long long)r.S * 1001 * 4 * 64);
            CHECK(q.gbnd_stride == 2ll * 1001 * kPaths && q.gdbnd_stride == 2ll * 1001);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + (size_t)(q.gbnd_stride + q.gdbnd_stride) * 4 + sizeof(ReadState));
            CHECK(q.per_read_all(1, 1, 1, 1) == q.per_read);
            CHECK(!q.use16 && !q.spec && !q.spec4 && !q.two_sweep && !q.use_rec && !q.retire && !q.dsel && !q.dsel4);
        }
        // one 16383-base read on 17000 rows: about 140 MB of direction words
        CHECK(run(params(M), shape(16383, 17000), q) == RG_OK);
        CHECK(q.gdirs_stride * 4 == 8ll * 17001 * 1024 && q.gdirs_stride * 4 > 139000000ll && q.gdirs_stride * 4 < 140000000ll);
        // refusals
        CHECK(run(params(M), shape(16384), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("16383") != std::string::npos);
        CHECK(run(params(M, 1, -2), shape(5000), q) == RG_ERR_ARG);
        CHECK(run(params(M, -4, 1), shape(5000), q) == RG_ERR_ARG);
        CHECK(run(params(M, 0, 0), shape(5000), q) == RG_OK);
        for (int bit : {1, 2, 4, 8, 12}) {
            rg_params p = params(M);
            p.amb_mode = bit;
            CHECK(run(p, shape(5000), q) == RG_ERR_ARG);
        }
        // capacity at the new lengths: (1000 + 15000) * 16777 < 2^28 <= 16000 * 16778
        CHECK(run(params(M, -16775, -2), shape(15000), q) == RG_OK);
        CHECK(run(params(M, -16776, -2), shape(15000), q) == RG_ERR_CAPACITY);
        {
            rg_params p = params(M);
            p.scores[0] = 16778;
            CHECK(run(p, shape(15000), q) == RG_ERR_CAPACITY);
            p.scores[0] = 16777;
            CHECK(run(p, shape(15000), q) == RG_OK);
            p.scores[0 * 6 + 5] = 1 << 30;      // the '-' entries are not read
            CHECK(run(p, shape(15000), q) == RG_OK);
        }
        // the base mode keeps its limit
        CHECK(run(params(base), shape(2048), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("2047") != std::string::npos);
    }
    PathPlan q;
    CHECK(run(params(RG_MODE_PATHWISE), shape(5000), q) == RG_OK && !q.gap && q.gbnd_stride == 0);
    return finish("gap long plan ok");
}
