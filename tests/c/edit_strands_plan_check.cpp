// CPU check of the plan of the both-strands edit-distance pathwise modes (-m 64 / -m 65; recgraph_amd/csrc/rg_path_plan.cpp:
// plan_pathwise_edit_strands): the two word counts on both sides of every boundary, the buffers per_read counts, every refusal with its
// message, the capacity edge, and that the two modes are rows of neither mode table.  Built and run by
// tests/test_pathwise_edit_strands_cpu.py.
#include "gap_mode_check.hpp"

using namespace gap_check;

static rg_params unit(int mode, int m = 0, int x = -1, int o = 0, int e = -1, int amb = 0) {
    rg_params p = score_params(mode, m, x);
    p.gap_open = o;
    p.gap_ext = e;
    p.amb_mode = amb;
    return p;
}
static bool says(const char* what) { return g_last_error.find(what) != std::string::npos; }

int main() {
    CHECK(RG_MODE_PATHWISE_EDIT_STRANDS == 64 && RG_MODE_PATHWISE_EDIT_SEMI_STRANDS == 65 && EDIT_STRANDS_MAX_READ == 16383 && EDIT_STRANDS_MAX_WORDS == 16);
    for (int m = -2; m < 200; ++m) {
        CHECK(edit_strands_mode(m).valid == (m == 64 || m == 65));
        CHECK(edit_strands_mode(m).semi == (m == 65));
        // the existing tables keep their rows
        CHECK(edit_mode(m).valid == (m == 44 || m == 45 || m == 94 || m == 95));
        if (m == 64 || m == 65) CHECK(!gap_mode(m).valid && !edit_mode(m).valid && path_gap_base_mode(m) == m && edit_base_mode(m) == m);
    }
    CHECK(edit_any_base_mode(64) == RG_MODE_PATHWISE_GAP && edit_any_base_mode(65) == RG_MODE_PATHWISE_GAP_SEMI);
    CHECK(edit_any_base_mode(44) == RG_MODE_PATHWISE_GAP && edit_any_base_mode(95) == RG_MODE_PATHWISE_GAP_SEMI && edit_any_base_mode(26) == 26 && edit_any_base_mode(4) == 4);
    for (int M : {RG_MODE_PATHWISE_EDIT_STRANDS, RG_MODE_PATHWISE_EDIT_SEMI_STRANDS}) {
        PathPlan q;
        // n, W of the score pass (n <= 1024 W), W of the direction pass (mode 44's: n <= 2048 W)
        const struct { int n, Wp, Wd; } routes[] = {{1, 1, 1},    {1023, 1, 1}, {1024, 1, 1}, {1025, 2, 1}, {2048, 2, 1}, {2049, 4, 2}, {4096, 4, 2},
                                                    {4097, 8, 4}, {8192, 8, 4}, {8193, 16, 8}, {16383, 16, 8}};
        for (const auto& r : routes) {
            for (int amb : {0, RG_AMB_BOTH_STRANDS}) {
                CHECK(run(unit(M, 0, -1, 0, -1, amb), shape(r.n), q) == RG_OK);
                CHECK(q.edit && q.edit_strands && !q.edit_xlong && !q.gap && !q.local && q.mode == RG_MODE_PATHWISE_EDIT && q.semi == (M == RG_MODE_PATHWISE_EDIT_SEMI_STRANDS));
                CHECK(q.edit_pair_words == r.Wp && q.edit_words == r.Wd && q.C == 32 * r.Wd && q.nwv == 1 && q.wpad == 2048 * r.Wd);
                CHECK(r.n <= 1024 * r.Wp && (r.Wp == 1 || r.n > 512 * r.Wp));
                // the direction buffer is mode 44's
                PathPlan one;
                CHECK(run(unit(M - 20), shape(r.n), one) == RG_OK && one.gdirs_stride == q.gdirs_stride && one.edit_words == q.edit_words && !one.edit_strands);
                CHECK(q.gdirs_stride == 1001ll * 2 * r.Wd * 64);
                CHECK(q.edit_orient_bytes >= (size_t)r.n && q.edit_orient_bytes % 16 == 0 && q.edit_orient_bytes < (size_t)r.n + 16);
                // ... and beside it: a second ReadState, the oriented read, the strand byte
                CHECK(q.per_read == one.per_read + sizeof(ReadState) + q.edit_orient_bytes + 1 && q.per_read_all(1, 1, 1, 1) == q.per_read);
                CHECK(q.stage == PATH_STAGE_ALL && plan_gap_stage(q, PATH_STAGE_PICK) == RG_ERR_ARG);
                CHECK(!q.use16 && !q.spec && !q.spec4 && !q.two_sweep && !q.use_rec && !q.retire && !q.layer_window);
            }
        }
        // refusals, each at 5 and at 16384 bases
        for (int n : {5, 16384}) {
            CHECK(run(unit(M, 2, -4, -4, -2), shape(n), q) == RG_ERR_ARG);          // the default scores
            CHECK(says("-M 0 -X 1 -O 0 -E 1") && says("-m 26 / -m 27") && says("-m 64 / -m 65"));
            CHECK(run(unit(M, 0, -1, -4, -1), shape(n), q) == RG_ERR_ARG && says("-M 0 -X 1 -O 0 -E 1"));      // -O 4
            CHECK(run(unit(M, 0, -1, 0, -2), shape(n), q) == RG_ERR_ARG && says("-m 26 / -m 27"));
            CHECK(run(unit(M, 0, -1, 0, 0), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, -1, 1, -1), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, -1, 0, 1), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 1, -1), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, -2), shape(n), q) == RG_ERR_ARG);
            // the plan admits amb_mode 0 and 4 alone (rg_batch_create has its own words for bits 0, 1, 3 alone and higher ones)
            for (int amb = 1; amb < 16; ++amb)
                if (amb != RG_AMB_BOTH_STRANDS) CHECK(run(unit(M, 0, -1, 0, -1, amb), shape(n), q) == RG_ERR_ARG);
        }
        CHECK(run(unit(M, 0, -1, 0, -1, RG_AMB_BOTH_STRANDS | RG_AMB_STRAND_VOTE), shape(5), q) == RG_ERR_ARG);
        CHECK(says("vote") && says("-m 64 / -m 65") && says("one pass"));
        CHECK(run(unit(M), shape(16384), q) == RG_ERR_ARG);
        CHECK(says("16383") && says("-m 64 / -m 65"));
        {
            rg_params p = unit(M);
            p.scores[0 * 6 + 5] = -2;                    // the '-' entries are not looked at
            p.scores[5 * 6 + 3] = 1 << 30;
            CHECK(run(p, shape(100), q) == RG_OK);
            p.scores[4 * 6 + 4] = 0;                     // N matches N
            CHECK(run(p, shape(100), q) == RG_OK);
            p.scores[2 * 6 + 4] = -2;                    // an N entry is inside the block
            CHECK(run(p, shape(100), q) == RG_ERR_ARG && says("-M 0 -X 1 -O 0 -E 1"));
        }
        // mode 16's budget: rows + n < 2^28
        CHECK(run(unit(M), shape(16383, (1 << 28) - 16384), q) == RG_OK);
        CHECK(run(unit(M), shape(16383, (1 << 28) - 16383), q) == RG_ERR_CAPACITY);
        CHECK(run(unit(M == RG_MODE_PATHWISE_EDIT_STRANDS ? 26 : 27), shape(16383, (1 << 28) - 16383), q) == RG_ERR_CAPACITY);
        CHECK(run(unit(M == RG_MODE_PATHWISE_EDIT_STRANDS ? 26 : 27), shape(16383, (1 << 28) - 16384), q) == RG_OK);
    }
    // the neighbours stay what they are: 44 / 45 / 94 / 95 refuse every amb_mode bit
    PathPlan q;
    for (int M : {44, 45, 94, 95})
        for (int amb : {4, 12}) CHECK(run(unit(M, 0, -1, 0, -1, amb), shape(100), q) == RG_ERR_ARG);
    CHECK(run(unit(44), shape(5000), q) == RG_OK && q.edit && !q.edit_strands && q.edit_pair_words == 0 && q.edit_orient_bytes == 0);
    CHECK(run(unit(63), shape(100), q) != RG_OK || !q.edit);
    CHECK(run(unit(66), shape(100), q) != RG_OK || !q.edit);
    return finish("edit strands plan ok");
}
