// CPU check of the plans of the both-strands affine-gap pathwise modes for reads of up to 131071 bases (-m 76 / -m 77 / -m 82;
// recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise, plan_gap_stage).  A batch of these modes runs two PICK stages and one TRACE
// stage, each planned by its own longest read: the whole-pipeline plan of a stage is mode m + 50's, a PICK plan counts ReadState
// (and, striped, the score pass's P * 2 * (rows + 1) boundary ints) per read, a TRACE plan mode m + 50's bytes minus those ints;
// plan_gap_stage leaves every plan of an existing mode as it is; the amb_mode rule and the refusals.  Built and run by
// tests/test_pathwise_gap_xstrands_cpu.py.
#include "gap_mode_check.hpp"

using namespace gap_check;

// everything of a plan but per_read and stage
static bool same_geometry(const PathPlan& a, const PathPlan& b) {
    return a.C == b.C && a.nwv == b.nwv && a.wpad == b.wpad && a.gap_words == b.gap_words && a.gdirs_stride == b.gdirs_stride &&
           a.gbnd_stride == b.gbnd_stride && a.gdbnd_stride == b.gdbnd_stride && a.gckpt_stride == b.gckpt_stride && a.gwalk_bytes == b.gwalk_bytes &&
           a.gap == b.gap && a.gap_xlong == b.gap_xlong && a.mode == b.mode && a.semi == b.semi && a.local == b.local && a.maxmatch == b.maxmatch;
}

int main() {
    CHECK(RG_MODE_PATHWISE_GAP_XSTRANDS == 76 && RG_MODE_PATHWISE_GAP_SEMI_XSTRANDS == 77 && RG_MODE_PATHWISE_GAP_LOCAL_XSTRANDS == 82);
    CHECK(PATH_STAGE_ALL == 0 && PATH_STAGE_PICK != PATH_STAGE_TRACE);
    const int modes[] = {RG_MODE_PATHWISE_GAP_XSTRANDS, RG_MODE_PATHWISE_GAP_SEMI_XSTRANDS, RG_MODE_PATHWISE_GAP_LOCAL_XSTRANDS};
    for (int M : modes) {
        const int base = kGapRuleBase[gap_mode(M).rule], xl = in_family(M, GAP_FAM_XLONG);
        const int lng = in_family(M, GAP_FAM_LONG), str = in_family(M, GAP_FAM_STRANDS);
        CHECK(is_family(M, GAP_FAM_XSTRANDS) && path_gap_base_mode(M) == base && in_family(base, GAP_FAM_XSTRANDS) == M);
        // the other families keep their members: not the new modes, and every existing mode
        CHECK(!is_family(M, GAP_FAM_XLONG) && !long_limit(M) && !is_family(M, GAP_FAM_STRANDS));
        for (int other : {base, lng, str, xl}) CHECK(!is_family(other, GAP_FAM_XSTRANDS) && path_gap_base_mode(other) == base);
        CHECK(is_family(xl, GAP_FAM_XLONG) && is_family(str, GAP_FAM_STRANDS) && long_limit(lng) && long_limit(str));
        for (int m = 0; m < 128; ++m)
            if (m != modes[0] && m != modes[1] && m != modes[2]) CHECK(!is_family(m, GAP_FAM_XSTRANDS));
        PathPlan q, g, pick, trace;
        // the whole-pipeline plan of a stage's reads IS mode m + 50's, at every length class
        for (int n : {1, 255, 1024, 2047, 2048, 4096, 16383, 16384, 40000, 131071}) {
            CHECK(run(params(M), shape(n), q) == RG_OK);
            CHECK(run(params(xl), shape(n), g) == RG_OK);
            CHECK(same_geometry(q, g) && q.per_read == g.per_read && q.stage == PATH_STAGE_ALL && g.stage == PATH_STAGE_ALL);
            CHECK(q.gap_xlong == (n > 2047));
            // PICK: ReadState, and when striped the boundary ints of the score pass
            pick = q;
            CHECK(plan_gap_stage(pick, PATH_STAGE_PICK) == RG_OK);
            CHECK(same_geometry(pick, q) && pick.stage == PATH_STAGE_PICK);
            const long long rows1 = kRows + 1;
            if (n <= 2047) CHECK(pick.per_read == sizeof(ReadState));
            else CHECK(pick.per_read == sizeof(ReadState) + (size_t)kPaths * 2 * rows1 * 4);
            // TRACE: mode m + 50's bytes minus those ints
            trace = q;
            CHECK(plan_gap_stage(trace, PATH_STAGE_TRACE) == RG_OK);
            CHECK(same_geometry(trace, q) && trace.stage == PATH_STAGE_TRACE);
            CHECK(trace.per_read == g.per_read - (n <= 2047 ? 0 : (size_t)kPaths * 2 * rows1 * 4));
            if (n > 2047) CHECK(trace.per_read == (size_t)q.gdirs_stride * 4 + (size_t)q.gckpt_stride * 4 + q.gwalk_bytes + sizeof(ReadState));
            else CHECK(trace.per_read == (size_t)q.gdirs_stride * 4 + sizeof(ReadState));
            // a PICK chunk is larger than the whole pipeline's
            CHECK(pick.per_read < q.per_read && pick.per_read + trace.per_read == q.per_read + sizeof(ReadState));
            CHECK(pick.per_read_all(1, 1, 1, 1) == pick.per_read && trace.per_read_all(1, 1, 1, 1) == trace.per_read);
            // PATH_STAGE_ALL changes nothing
            PathPlan all = q;
            CHECK(plan_gap_stage(all, PATH_STAGE_ALL) == RG_OK && all.per_read == q.per_read && all.stage == PATH_STAGE_ALL && same_geometry(all, q));
        }
        // the stages of one batch may land in different length classes: both ways round
        {
            PathPlan a, b, t;
            CHECK(run(params(M), shape(2100), a) == RG_OK && plan_gap_stage(a, PATH_STAGE_PICK) == RG_OK);      // first pick striped ...
            CHECK(run(params(M), shape(150), b) == RG_OK && plan_gap_stage(b, PATH_STAGE_PICK) == RG_OK);       // ... the other strand's on the base kernels
            CHECK(run(params(M), shape(2100), t) == RG_OK && plan_gap_stage(t, PATH_STAGE_TRACE) == RG_OK);
            CHECK(a.nwv == 2 && a.gap_xlong && b.nwv == 1 && !b.gap_xlong && b.C == 4 && t.nwv == 2 && t.gap_xlong);
            CHECK(b.per_read == sizeof(ReadState) && a.per_read == sizeof(ReadState) + (size_t)a.gbnd_stride * 4);
            CHECK(run(params(M), shape(40000), a) == RG_OK && plan_gap_stage(a, PATH_STAGE_PICK) == RG_OK);     // the qualifying reads are the long ones ...
            CHECK(run(params(M), shape(40000), t) == RG_OK && plan_gap_stage(t, PATH_STAGE_TRACE) == RG_OK);    // ... and the trace is planned by all reads
            CHECK(a.nwv == 20 && t.nwv == 20 && t.gckpt_stride == 19ll * 2 * 1001 && t.gdirs_stride == 1001ll * 4 * 64);
        }
        // amb_mode: 0, 4, and 12 in the two modes whose scores can be negative; nothing else
        for (int n : {5, 30000}) {
            for (int amb : {0, 4}) CHECK(run(params(M, -4, -2, amb), shape(n), q) == RG_OK);
            if (M == RG_MODE_PATHWISE_GAP_LOCAL_XSTRANDS) {
                CHECK(run(params(M, -4, -2, 12), shape(n), q) == RG_ERR_ARG);
                CHECK(g_last_error.find("hopeless") != std::string::npos && g_last_error.find("82") != std::string::npos);
            } else {
                CHECK(run(params(M, -4, -2, 12), shape(n), q) == RG_OK);
            }
            for (int amb : {1, 2, 3, 5, 8, 13, 16, 20, 28}) CHECK(run(params(M, -4, -2, amb), shape(n), q) == RG_ERR_ARG);
            // modes 56 / 57 / 62 keep refusing every bit
            for (int amb : {1, 2, 4, 8, 12}) CHECK(run(params(xl, -4, -2, amb), shape(n), q) == RG_ERR_ARG);
        }
        // refusals of the pipeline
        CHECK(run(params(M), shape(131072), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("131071") != std::string::npos);
        CHECK(run(params(M, 1, -2), shape(50000), q) == RG_ERR_ARG && run(params(M, -4, 1), shape(5), q) == RG_ERR_ARG);
        CHECK(run(params(M, -2047, -2), shape(130000), q) == RG_OK);
        CHECK(run(params(M, -2048, -2), shape(130000), q) == RG_ERR_CAPACITY);
        // modes 26 / 27 / 32 keep their limit
        CHECK(run(params(str), shape(16384), q) == RG_ERR_ARG);
        CHECK(g_last_error.find("16383") != std::string::npos);
    }
    // plan_gap_stage on the plans of the existing modes: no stage for a plan that is no affine-gap plan, none for the striped plan of
    // the long modes; and plan_pathwise itself returns what it returned, stage 0
    {
        PathPlan q, before;
        for (int m : {RG_MODE_PATHWISE, RG_MODE_PATHWISE_SEMI, RG_MODE_RECOMBINATION, RG_MODE_RECOMBINATION_SEMI}) {
            CHECK(run(params(m), shape(800), q) == RG_OK && !q.gap && q.stage == PATH_STAGE_ALL);
            before = q;
            CHECK(plan_gap_stage(q, PATH_STAGE_PICK) == RG_ERR_ARG && plan_gap_stage(q, PATH_STAGE_TRACE) == RG_ERR_ARG);
            CHECK(q.per_read == before.per_read && q.stage == PATH_STAGE_ALL);
            CHECK(plan_gap_stage(q, PATH_STAGE_ALL) == RG_OK && q.per_read == before.per_read);
        }
        for (int m : family_modes({GAP_FAM_LONG, GAP_FAM_STRANDS})) {
            CHECK(run(params(m), shape(5000), q) == RG_OK && q.gap && q.nwv == 3 && !q.gap_xlong && q.stage == PATH_STAGE_ALL);
            before = q;
            CHECK(plan_gap_stage(q, PATH_STAGE_TRACE) == RG_ERR_ARG && q.per_read == before.per_read && q.stage == PATH_STAGE_ALL);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + (size_t)(q.gbnd_stride + q.gdbnd_stride) * 4 + sizeof(ReadState));
        }
        for (int m : family_modes({GAP_FAM_BASE, GAP_FAM_LONG, GAP_FAM_STRANDS, GAP_FAM_XLONG})) {
            CHECK(run(params(m), shape(700), q) == RG_OK && q.stage == PATH_STAGE_ALL && q.nwv == 1);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + sizeof(ReadState));
        }
        for (int m : family_modes({GAP_FAM_XLONG})) {
            CHECK(run(params(m), shape(8192), q) == RG_OK && q.stage == PATH_STAGE_ALL);
            CHECK(q.per_read == (size_t)q.gdirs_stride * 4 + (size_t)(q.gbnd_stride + q.gckpt_stride) * 4 + q.gwalk_bytes + sizeof(ReadState));
        }
        PathPlan z;
        CHECK(run(params(RG_MODE_PATHWISE_GAP_XSTRANDS), shape(700), z) == RG_OK && plan_gap_stage(z, 3) == RG_ERR_ARG && plan_gap_stage(z, -1) == RG_ERR_ARG);
    }
    return finish("gap xstrands plan ok");
}
