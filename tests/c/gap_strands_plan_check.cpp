// CPU check of the plan of the both-strands affine-gap pathwise modes (-m 26 / -m 27 / -m 32; recgraph_amd/csrc/rg_path_plan.cpp:
// plan_pathwise).  A batch of these modes runs two passes, each planned by its own longest read: whatever amb_mode the mode admits,
// the plan of a pass IS the plan of the long flavour (the same rule in the long family) at that pass's longest read — so pass A may run the striped kernels
// and pass B the base ones, or the other way round, and the per-read byte count of each pass is the one its own kernels need.  Also
// the amb_mode values the modes admit and refuse.  Built and run by tests/test_pathwise_gap_strands_cpu.py.
#include "gap_mode_check.hpp"

using namespace gap_check;

static bool same_plan(const PathPlan& a, const PathPlan& b) {
    return a.gap == b.gap && a.mode == b.mode && a.semi == b.semi && a.local == b.local && a.C == b.C && a.nwv == b.nwv && a.wpad == b.wpad &&
           a.gap_words == b.gap_words && a.gdirs_stride == b.gdirs_stride && a.gbnd_stride == b.gbnd_stride && a.gdbnd_stride == b.gdbnd_stride &&
           a.per_read == b.per_read && a.maxmatch == b.maxmatch && a.per_read_all(1, 1, 1, 1) == b.per_read_all(1, 1, 1, 1);
}

int main() {
    CHECK(RG_MODE_PATHWISE_GAP_STRANDS == 26 && RG_MODE_PATHWISE_GAP_SEMI_STRANDS == 27 && RG_MODE_PATHWISE_GAP_LOCAL_STRANDS == 32);
    CHECK(RG_MODE_PATHWISE_GAP_STRANDS == in_family(RG_MODE_PATHWISE_GAP, GAP_FAM_STRANDS) && RG_MODE_PATHWISE_GAP_SEMI_STRANDS == in_family(RG_MODE_PATHWISE_GAP_SEMI, GAP_FAM_STRANDS) &&
          RG_MODE_PATHWISE_GAP_LOCAL_STRANDS == in_family(RG_MODE_PATHWISE_GAP_LOCAL, GAP_FAM_STRANDS) && kGapFamilies[GAP_FAM_STRANDS].offset == 20);
    for (int M : {RG_MODE_PATHWISE_GAP_STRANDS, RG_MODE_PATHWISE_GAP_SEMI_STRANDS, RG_MODE_PATHWISE_GAP_LOCAL_STRANDS}) {
        const int base = path_gap_base_mode(M), lng = in_family(M, GAP_FAM_LONG);
        CHECK(is_family(M, GAP_FAM_STRANDS) && long_limit(M) && base == kGapRuleBase[gap_mode(M).rule] && in_family(base, GAP_FAM_STRANDS) == M);
        CHECK(!is_family(lng, GAP_FAM_STRANDS) && !is_family(base, GAP_FAM_STRANDS) && path_gap_base_mode(lng) == base);
        const bool local = M == RG_MODE_PATHWISE_GAP_LOCAL_STRANDS;
        PathPlan q, g;
        // every pass of the mode, whatever its longest read and whatever amb_mode says: the plan of the long flavour at that length
        for (int amb : {0, 4, 12}) {
            if (local && amb == 12) continue;
            for (int n : {1, 150, 255, 256, 2047, 2048, 2100, 4096, 16383}) {
                CHECK(run(params(M, -4, -2, amb), shape(n), q) == RG_OK);
                CHECK(run(params(lng), shape(n), g) == RG_OK);
                CHECK(same_plan(q, g));
                CHECK(q.gap && q.semi == (M == RG_MODE_PATHWISE_GAP_SEMI_STRANDS) && q.local == local && q.nwv == (n + 2048) / 2048);
            }
        }
        // two passes of one batch in different length classes, both ways round: one on the base kernels, one striped, each with the
        // bytes its own kernels take per read (the striped pass counts S stripes of direction words and both boundary buffers)
        PathPlan a, b;
        CHECK(run(params(M, -4, -2, 4), shape(2100), a) == RG_OK && run(params(M, -4, -2, 4), shape(150), b) == RG_OK);
        CHECK(a.nwv == 2 && a.C == 32 && b.nwv == 1 && b.C == 4);
        CHECK(a.per_read == (size_t)2 * 1001 * 4 * 64 * 4 + (size_t)(2 * 1001 * kPaths + 2 * 1001) * 4 + sizeof(ReadState));
        CHECK(b.per_read == (size_t)1001 * 1 * 64 * 4 + sizeof(ReadState) && b.gbnd_stride == 0 && b.gdbnd_stride == 0);
        CHECK(b.per_read < a.per_read);
        // a pass can never be longer than the batch: the longest read of pass B is one of the batch's reads, so the batch's refusals
        // (answered by rg_batch_create with the batch's longest read) cover both passes
        CHECK(run(params(M), shape(16384), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("16383") != std::string::npos);
        CHECK(run(params(M, 1, -2, 4), shape(100), q) == RG_ERR_ARG);
        CHECK(run(params(M, -4, 1, 4), shape(5000), q) == RG_ERR_ARG);
        CHECK(run(params(M, -16775, -2, 0), shape(15000), q) == RG_OK);
        CHECK(run(params(M, -16776, -2, 0), shape(15000), q) == RG_ERR_CAPACITY);
        // amb_mode: 0, 4 and (26, 27) 12; nothing else
        for (int amb : {1, 2, 3, 5, 6, 8, 9, 13, 16, 20, 28, -1}) {
            CHECK(run(params(M, -4, -2, amb), shape(100), q) == RG_ERR_ARG);
            CHECK(run(params(M, -4, -2, amb), shape(3000), q) == RG_ERR_ARG);
        }
        CHECK(run(params(M, -4, -2, 12), shape(100), q) == (local ? RG_ERR_ARG : RG_OK));
        if (local) CHECK(g_last_error.find("hopeless") != std::string::npos);
        // the modes without the strands keep refusing every bit
        for (int amb : {4, 12}) {
            CHECK(run(params(lng, -4, -2, amb), shape(100), q) == RG_ERR_ARG);
            CHECK(run(params(base, -4, -2, amb), shape(100), q) == RG_ERR_ARG);
        }
    }
    return finish("gap strands plan ok");
}
