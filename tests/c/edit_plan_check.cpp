// CPU check of the plan of the edit-distance pathwise modes (-m 44 / -m 45; recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise_edit):
// W, the direction buffer's stride and per_read on both sides of 2048, 4096 and 8192 bases and at 16383; every refusal; and that the two
// modes are no rows of the affine-gap family table.  Built and run by tests/test_pathwise_edit_cpu.py.
#include "gap_mode_check.hpp"

using namespace gap_check;

static rg_params unit(int mode, int m = 0, int x = -1, int o = 0, int e = -1, int amb = 0) {
    rg_params p = score_params(mode, m, x);
    p.gap_open = o;
    p.gap_ext = e;
    p.amb_mode = amb;
    return p;
}

int main() {
    CHECK(RG_MODE_PATHWISE_EDIT == 44 && RG_MODE_PATHWISE_EDIT_SEMI == 45);
    CHECK(edit_mode(44).valid && !edit_mode(44).semi && edit_mode(45).valid && edit_mode(45).semi);
    CHECK(edit_mode(44).family == edit_mode(45).family && edit_mode(44).family->max_read == 16383 && edit_mode(44).family->gap_family == GAP_FAM_LONG);
    CHECK(edit_base_mode(44) == RG_MODE_PATHWISE_GAP && edit_base_mode(45) == RG_MODE_PATHWISE_GAP_SEMI && edit_base_mode(16) == 16 && edit_base_mode(4) == 4);
    for (int m = -2; m < 200; ++m) {
        CHECK(edit_mode(m).valid == (m == 44 || m == 45 || m == 94 || m == 95));
        if (m == 44 || m == 45) CHECK(!gap_mode(m).valid && path_gap_base_mode(m) == m);
    }
    for (int M : {RG_MODE_PATHWISE_EDIT, RG_MODE_PATHWISE_EDIT_SEMI}) {
        PathPlan q;
        const struct { int n, W; } routes[] = {{1, 1}, {2047, 1}, {2048, 1}, {2049, 2}, {4096, 2}, {4097, 4}, {8192, 4}, {8193, 8}, {16383, 8}};
        for (const auto& r : routes) {
            CHECK(run(unit(M), shape(r.n), q) == RG_OK);
            CHECK(q.edit && !q.gap && !q.local && !q.gap_xlong && q.mode == RG_MODE_PATHWISE_EDIT && q.semi == (M == RG_MODE_PATHWISE_EDIT_SEMI));
            CHECK(q.edit_words == r.W && q.C == 32 * r.W && q.nwv == 1 && q.wpad == 2048 * r.W && r.n <= q.wpad && (r.W == 1 || r.n > q.wpad / 2));
            CHECK(q.gdirs_stride == 1001ll * 2 * r.W * 64);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + sizeof(ReadState) && q.per_read_all(1, 1, 1, 1) == q.per_read);
            CHECK(q.gbnd_stride == 0 && q.gdbnd_stride == 0 && q.gckpt_stride == 0 && q.stage == PATH_STAGE_ALL);
            CHECK(!q.use16 && !q.spec && !q.spec4 && !q.two_sweep && !q.use_rec && !q.retire && !q.dsel && !q.dsel4 && !q.layer_window);
            // a stage is a thing of the affine-gap plans
            CHECK(plan_gap_stage(q, PATH_STAGE_ALL) == RG_OK && plan_gap_stage(q, PATH_STAGE_PICK) == RG_ERR_ARG);
        }
        // one 16383-base read on 17000 rows: about 70 MB of direction bits, half of mode 16's
        CHECK(run(unit(M), shape(16383, 17000), q) == RG_OK);
        CHECK(q.gdirs_stride * 4 == 17001ll * 16 * 256 && q.gdirs_stride * 4 > 69000000ll && q.gdirs_stride * 4 < 70000000ll);
        PathPlan g;
        CHECK(run(unit(M == RG_MODE_PATHWISE_EDIT ? 16 : 17), shape(16383, 17000), g) == RG_OK && g.gdirs_stride == 2 * q.gdirs_stride);
        // refusals, each at 5 and at 16384 bases
        for (int n : {5, 16384}) {
            CHECK(run(unit(M, 2, -4, -4, -2), shape(n), q) == RG_ERR_ARG);          // the default scores
            if (n == 5) CHECK(g_last_error.find("-M 0 -X 1 -O 0 -E 1") != std::string::npos);
            CHECK(run(unit(M, 0, -1, -1, -1), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, -1, 0, -2), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, -1, 0, 0), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, -1, 1, -1), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, -1, 0, 1), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 1, -1), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, -2), shape(n), q) == RG_ERR_ARG);
            CHECK(run(unit(M, 0, 1), shape(n), q) == RG_ERR_ARG);
            for (int amb : {1, 2, 4, 8, 12}) CHECK(run(unit(M, 0, -1, 0, -1, amb), shape(n), q) == RG_ERR_ARG);
        }
        CHECK(run(unit(M), shape(16384), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("16383") != std::string::npos);
        {
            rg_params p = unit(M);
            p.scores[0 * 6 + 5] = -2;                    // the '-' entries are not looked at
            p.scores[5 * 6 + 3] = 1 << 30;
            CHECK(run(p, shape(100), q) == RG_OK);
            p.scores[4 * 6 + 4] = 0;                     // N matches N
            p.scores[0 * 6 + 1] = 0;                     // any 0 / -1 matrix
            CHECK(run(p, shape(100), q) == RG_OK);
            p.scores[2 * 6 + 4] = -2;                    // an N entry is inside the block
            CHECK(run(p, shape(100), q) == RG_ERR_ARG);
            CHECK(g_last_error.find("-M 0 -X 1 -O 0 -E 1") != std::string::npos);
        }
        // mode 16's budget: rows + n < 2^28
        CHECK(run(unit(M), shape(16383, (1 << 28) - 16384), q) == RG_OK);
        CHECK(run(unit(M), shape(16383, (1 << 28) - 16383), q) == RG_ERR_CAPACITY);
        CHECK(run(unit(M == RG_MODE_PATHWISE_EDIT ? 16 : 17), shape(16383, (1 << 28) - 16383), q) == RG_ERR_CAPACITY);
    }
    // the neighbours stay what they are
    PathPlan q;
    CHECK(run(unit(16), shape(5000), q) == RG_OK && q.gap && !q.edit && q.edit_words == 0);
    CHECK(run(params(RG_MODE_PATHWISE), shape(500), q) == RG_OK && !q.gap && !q.edit);
    return finish("edit plan ok");
}
