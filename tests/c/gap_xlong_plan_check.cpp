// CPU check of the plan of the affine-gap pathwise modes for reads of up to 131071 bases (-m 56 / -m 57 / -m 62;
// recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise): up to 2047 bases the plan IS the base mode's; beyond, C = 32 and
// S = ceil((n + 1) / 2048) <= 64 column stripes with the direction words of ONE stripe, a checkpoint slot for every stripe but the
// last, the score pass's boundary buffer and the walk state counted per read — for S <= 8 too, where modes 16 / 17 / 22 would keep S
// stripes of words; the refusals at the new lengths.  Built and run by tests/test_pathwise_gap_xlong_cpu.py.
#include "gap_mode_check.hpp"

using namespace gap_check;

int main() {
    CHECK(RG_MODE_PATHWISE_GAP_XLONG == 56 && RG_MODE_PATHWISE_GAP_SEMI_XLONG == 57 && RG_MODE_PATHWISE_GAP_LOCAL_XLONG == 62);
    const int xlongs[] = {RG_MODE_PATHWISE_GAP_XLONG, RG_MODE_PATHWISE_GAP_SEMI_XLONG, RG_MODE_PATHWISE_GAP_LOCAL_XLONG};
    for (int M : xlongs) {
        const int base = kGapRuleBase[gap_mode(M).rule], lng = in_family(M, GAP_FAM_LONG), str = in_family(M, GAP_FAM_STRANDS);
        CHECK(is_family(M, GAP_FAM_XLONG) && path_gap_base_mode(M) == base && !long_limit(M) && !is_family(M, GAP_FAM_STRANDS) && in_family(base, GAP_FAM_XLONG) == M);
        CHECK(!is_family(base, GAP_FAM_XLONG) && !is_family(lng, GAP_FAM_XLONG) && !is_family(str, GAP_FAM_XLONG));
        PathPlan q, g;
        // up to 2047 bases: exactly the base mode's plan, and its kernels (nwv = 1)
        for (int n : {1, 255, 256, 1023, 1024, 2047}) {
            CHECK(run(params(M), shape(n), q) == RG_OK);
            CHECK(run(params(base), shape(n), g) == RG_OK);
            CHECK(q.gap && q.mode == RG_MODE_PATHWISE_GAP && q.nwv == 1 && !q.gap_xlong);
            CHECK(q.C == g.C && q.nwv == g.nwv && q.wpad == g.wpad && q.gap_words == g.gap_words && q.gdirs_stride == g.gdirs_stride);
            CHECK(q.per_read == g.per_read && q.semi == g.semi && q.local == g.local && q.maxmatch == g.maxmatch);
            CHECK(q.gbnd_stride == 0 && q.gdbnd_stride == 0 && q.gckpt_stride == 0 && q.gwalk_bytes == 0);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + sizeof(ReadState));
        }
        CHECK(q.semi == (M == RG_MODE_PATHWISE_GAP_SEMI_XLONG) && q.local == (M == RG_MODE_PATHWISE_GAP_LOCAL_XLONG));
        // beyond: stripes of 2048 columns, the new kernels whatever S is
        const struct { int n, S; } routes[] = {{2048, 2}, {4095, 2}, {4096, 3}, {8192, 5}, {16383, 8}, {16384, 9}, {40000, 20}, {131071, 64}};
        for (const auto& r : routes) {
            CHECK(run(params(M), shape(r.n), q) == RG_OK);
            CHECK(q.gap && q.gap_xlong && q.mode == RG_MODE_PATHWISE_GAP && q.C == 32 && q.gap_words == 4);
            CHECK(q.nwv == r.S && q.nwv >= 2 && q.nwv <= 64 && q.wpad == r.S * 2048 && r.n + 1 <= q.wpad && r.n + 1 > q.wpad - 2048);
            CHECK(q.semi == (M == RG_MODE_PATHWISE_GAP_SEMI_XLONG) && q.local == (M == RG_MODE_PATHWISE_GAP_LOCAL_XLONG));
            CHECK(q.gdirs_stride == 1001ll * 4 * 64);                              // ONE stripe
            CHECK(q.gckpt_stride == (long long)(r.S - 1) * 2 * 1001);
            CHECK(q.gbnd_stride == 2ll * 1001 * 6 && q.gdbnd_stride == 0);
            CHECK(q.gwalk_bytes > 0 && q.gwalk_bytes <= 64);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + (size_t)(q.gbnd_stride + q.gckpt_stride) * 4 + q.gwalk_bytes + sizeof(ReadState));
            CHECK(q.per_read_all(1, 1, 1, 1) == q.per_read);
            CHECK(!q.use16 && !q.spec && !q.spec4 && !q.two_sweep && !q.use_rec && !q.retire && !q.dsel && !q.dsel4);
        }
        // the long modes on the same batch keep S stripes of words and no checkpoint
        CHECK(run(params(lng), shape(8192), g) == RG_OK);
        CHECK(!g.gap_xlong && g.nwv == 5 && g.gdirs_stride == 5ll * 1001 * 4 * 64 && g.gckpt_stride == 0 && g.gdbnd_stride == 2ll * 1001);
        // one 16383-base read on 17000 rows and 16 paths: direction words and checkpoints of mode 56 against the words of mode 16
        CHECK(run(params(M), shape(16383, 17000, 16), q) == RG_OK);
        CHECK(run(params(lng), shape(16383, 17000, 16), g) == RG_OK);
        CHECK(q.gdirs_stride * 4 + q.gckpt_stride * 4 == 17001ll * 1024 + 7ll * 8 * 17001);
        CHECK(g.gdirs_stride * 4 == 8ll * 17001 * 1024);
        CHECK(q.gbnd_stride == g.gbnd_stride && q.gbnd_stride == 16ll * 2 * 17001);
        // 131071 bases on 140000 rows: the words stay one stripe's
        CHECK(run(params(M), shape(131071, 140000, 16), q) == RG_OK);
        CHECK(q.nwv == 64 && q.gdirs_stride * 4 == 140001ll * 1024 && q.gckpt_stride * 4 == 63ll * 8 * 140001);
        // refusals
        CHECK(run(params(M), shape(131072), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("131071") != std::string::npos);
        CHECK(run(params(M, 1, -2), shape(50000), q) == RG_ERR_ARG);
        CHECK(run(params(M, -4, 1), shape(50000), q) == RG_ERR_ARG);
        CHECK(run(params(M, 1, -2), shape(5), q) == RG_ERR_ARG);
        CHECK(run(params(M, 0, 0), shape(50000), q) == RG_OK);
        for (int bit : {1, 2, 4, 8, 12}) {
            rg_params p = params(M);
            p.amb_mode = bit;
            CHECK(run(p, shape(50000), q) == RG_ERR_ARG);
            CHECK(run(p, shape(5), q) == RG_ERR_ARG);
        }
        // capacity at the new lengths: (1000 + 130000) * 2049 < 2^28 <= 131000 * 2050
        CHECK(run(params(M, -2047, -2), shape(130000), q) == RG_OK);
        CHECK(run(params(M, -2048, -2), shape(130000), q) == RG_ERR_CAPACITY);
        {
            rg_params p = params(M);
            p.scores[0] = 2050;
            CHECK(run(p, shape(130000), q) == RG_ERR_CAPACITY);
            p.scores[0] = 2049;
            CHECK(run(p, shape(130000), q) == RG_OK);
            p.scores[0 * 6 + 5] = 1 << 30;      // the '-' entries are not read
            CHECK(run(p, shape(130000), q) == RG_OK);
        }
        // the earlier modes keep their limits
        CHECK(run(params(base), shape(2048), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("2047") != std::string::npos);
        CHECK(run(params(lng), shape(16384), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("16383") != std::string::npos);
        CHECK(run(params(str), shape(16384), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("16383") != std::string::npos);
    }
    return finish("gap xlong plan ok");
}
