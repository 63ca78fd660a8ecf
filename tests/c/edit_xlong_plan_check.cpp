// CPU check of the plan of the edit-distance pathwise modes for long reads (-m 94 / -m 95; recgraph_amd/csrc/rg_path_plan.cpp:
// plan_pathwise_edit): up to 16383 bases the plan IS the one of -m 44 / -m 45, field for field; beyond, S, the strides and per_read at
// 16384, 16385, 32768, 32769 and 131071 bases; every refusal; and that the modes are rows of the edit family table alone.
// Built and run by tests/test_pathwise_edit_xlong_cpu.py.
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
    CHECK(RG_MODE_PATHWISE_EDIT_XLONG == 94 && RG_MODE_PATHWISE_EDIT_SEMI_XLONG == 95);
    CHECK(EDIT_XLONG_MAX_READ == 131071 && EDIT_XLONG_STRIPE == 16384 && EDIT_XLONG_MAX_STRIPES == 8 && EDIT_MAX_READ == 16383);
    CHECK(edit_mode(94).valid && !edit_mode(94).semi && edit_mode(95).valid && edit_mode(95).semi);
    CHECK(edit_mode(94).family == edit_mode(95).family && edit_mode(94).family->max_read == 131071 && edit_mode(94).family->gap_family == GAP_FAM_XLONG);
    CHECK(edit_mode(94).family != edit_mode(44).family && edit_mode(44).family->max_read == 16383);
    CHECK(edit_base_mode(94) == RG_MODE_PATHWISE_GAP && edit_base_mode(95) == RG_MODE_PATHWISE_GAP_SEMI && edit_base_mode(93) == 93 && edit_base_mode(56) == 56);
    for (int m = -2; m < 200; ++m) {
        CHECK(edit_mode(m).valid == (m == 44 || m == 45 || m == 94 || m == 95));
        CHECK(edit_mode(m).family->offset == (m == 94 || m == 95 ? 50 : 0) && edit_mode(m).semi == (m == 45 || m == 95));
        if (m == 94 || m == 95) CHECK(!gap_mode(m).valid && path_gap_base_mode(m) == m);
    }
    for (int M : {RG_MODE_PATHWISE_EDIT_XLONG, RG_MODE_PATHWISE_EDIT_SEMI_XLONG}) {
        const bool semi = M == RG_MODE_PATHWISE_EDIT_SEMI_XLONG;
        PathPlan q, b;
        // the plan of mode 44 / 45, byte for byte of every field the driver reads
        for (int n : {1, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 16383}) {
            CHECK(run(unit(M), shape(n), q) == RG_OK && run(unit(M - 50), shape(n), b) == RG_OK);
            CHECK(q.edit && !q.edit_xlong && q.edit_slot_words == 0 && q.edit_bnd_stride == 0 && q.gwalk_bytes == 0 && q.nwv == 1);
            CHECK(q.edit == b.edit && q.edit_xlong == b.edit_xlong && q.mode == b.mode && q.semi == b.semi && q.semi == semi && q.edit_words == b.edit_words &&
                  q.C == b.C && q.nwv == b.nwv && q.wpad == b.wpad && q.gdirs_stride == b.gdirs_stride && q.per_read == b.per_read && q.gap == b.gap &&
                  q.stage == b.stage && q.gbnd_stride == b.gbnd_stride && q.gckpt_stride == b.gckpt_stride && q.edit_slot_words == b.edit_slot_words &&
                  q.edit_bnd_stride == b.edit_bnd_stride && q.gwalk_bytes == b.gwalk_bytes);
        }
        // striped (16384 bases fill ONE stripe to its last bit; the batch still gets the two of the smallest striped plan): 1000 rows -> 16 blocks of 64 rows -> 32 u64 per slot, already a multiple of 16
        const struct { int n, S; } routes[] = {{16384, 2}, {16385, 2}, {32768, 2}, {32769, 3}, {49152, 3}, {49153, 4}, {131071, 8}};
        for (const auto& r : routes) {
            CHECK(run(unit(M), shape(r.n), q) == RG_OK);
            CHECK(q.edit && q.edit_xlong && !q.gap && !q.gap_xlong && !q.local && q.mode == RG_MODE_PATHWISE_EDIT && q.semi == semi);
            CHECK(q.edit_words == 8 && q.C == 256 && q.nwv == r.S && q.wpad == 16384 * r.S && r.n <= q.wpad && (r.S == 2 || r.n > q.wpad - 16384));
            CHECK(q.gdirs_stride == 1001ll * 2 * 8 * 64);
            CHECK(q.edit_slot_words == 32 && q.edit_bnd_stride == (long long)kPaths * (r.S - 1) * 32 && q.gwalk_bytes == 32);
            CHECK(q.per_read == (size_t)1001 * 2 * 8 * 64 * 4 + (size_t)kPaths * (r.S - 1) * 32 * 8 + 32 + sizeof(ReadState));
            CHECK(q.per_read_all(1, 1, 1, 1) == q.per_read);
            CHECK(q.gbnd_stride == 0 && q.gdbnd_stride == 0 && q.gckpt_stride == 0 && q.stage == PATH_STAGE_ALL);
            CHECK(!q.use16 && !q.spec && !q.spec4 && !q.two_sweep && !q.use_rec && !q.retire && !q.dsel && !q.dsel4 && !q.layer_window);
            CHECK(plan_gap_stage(q, PATH_STAGE_ALL) == RG_OK && plan_gap_stage(q, PATH_STAGE_PICK) == RG_ERR_ARG);
        }
        // the slot: two bits per row as two masks per 64 rows, rounded up to a 128-byte line
        const struct { int rows, words; } slots[] = {{1, 16}, {64, 16}, {512, 16}, {513, 32}, {1024, 32}, {1025, 48}, {140000, 4384}};
        for (const auto& s : slots) {
            CHECK(run(unit(M), shape(20000, s.rows), q) == RG_OK);
            CHECK(q.edit_slot_words == s.words && q.edit_slot_words % 16 == 0 && q.edit_slot_words >= 2 * ((s.rows + 63) / 64) && q.edit_slot_words < 2 * ((s.rows + 63) / 64) + 16);
        }
        // one 131071-base read on 140000 rows: about 573 MB of words, four times mode 56's; the slots of 6 paths take 1.5 MB
        CHECK(run(unit(M), shape(131071, 140000), q) == RG_OK);
        CHECK(q.gdirs_stride * 4 == 140001ll * 4096 && q.gdirs_stride * 4 > 573000000ll && q.gdirs_stride * 4 < 574000000ll);
        CHECK(q.edit_bnd_stride * 8 == 6ll * 7 * 4384 * 8);
        PathPlan g;
        CHECK(run(unit(M - 38), shape(131071, 140000), g) == RG_OK && g.gap_xlong && 4 * g.gdirs_stride == q.gdirs_stride);
        // refusals, each at 5, 16384 and 131071 bases
        for (int n : {5, 16384, 131071}) {
            CHECK(run(unit(M, 2, -4, -4, -2), shape(n), q) == RG_ERR_ARG);          // the default scores
            CHECK(g_last_error.find("-M 0 -X 1 -O 0 -E 1") != std::string::npos && g_last_error.find("-m 94 / -m 95") != std::string::npos);
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
        CHECK(run(unit(M), shape(131072), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("131071") != std::string::npos);
        // modes 44 / 45 keep their limit and their message
        CHECK(run(unit(M - 50), shape(16384), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("16383") != std::string::npos && g_last_error.find("-m 44 / -m 45") != std::string::npos);
        {
            rg_params p = unit(M);
            p.scores[0 * 6 + 5] = -2;                    // the '-' entries are not looked at
            p.scores[4 * 6 + 4] = 0;                     // N matches N
            CHECK(run(p, shape(20000), q) == RG_OK && q.edit_xlong);
            p.scores[2 * 6 + 4] = -2;                    // an N entry is inside the block
            CHECK(run(p, shape(20000), q) == RG_ERR_ARG);
        }
        // mode 16's budget: rows + n < 2^28
        CHECK(run(unit(M), shape(131071, (1 << 28) - 131072), q) == RG_OK);
        CHECK(run(unit(M), shape(131071, (1 << 28) - 131071), q) == RG_ERR_CAPACITY);
        CHECK(run(unit(M - 38), shape(131071, (1 << 28) - 131071), q) == RG_ERR_CAPACITY);
    }
    return finish("edit xlong plan ok");
}
