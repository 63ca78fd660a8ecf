// CPU check of the pathwise driver's plan (recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise): which route a batch takes is host
// arithmetic that the GPU tests only see through byte parity — a wrong decision is usually still correct, only slower.  Every
// expected value is read off the driver as it was before the plan was split out of it; "drv:N" names the line of
// rg_path_driver.hip in that commit (0343416) the value comes from.  Built and run by tests/test_path_plan_cpu.py.
#include <map>
#include <set>
#include <string>

#include "plan_check_common.hpp"

// score_matrix.rs:35-66 as rg_scores_match_mis builds it (any pairing with '-' = 2x), and the CLI's recombination costs
static rg_params params(int mode, int m = 2, int x = -4) {
    rg_params p = score_params(mode, m, x);
    p.base_rec_cost = 4;
    p.multi_rec_cost = 0.1f;
    p.rec_band_width = 1.0f;
    return p;
}
// HOXD70-like: matches near 100, mismatches down to -125, every gap entry -200 (tests/golden/HOXD70.mtx)
static rg_params hoxd_like(int mode) {
    rg_params p = params(mode, 91, -114);
    p.scores[1 * 6 + 1] = p.scores[2 * 6 + 2] = 100;
    p.scores[0 * 6 + 1] = -125;
    for (int b = 0; b < 5; ++b) p.scores[b * 6 + 5] = p.scores[5 * 6 + b] = -200;
    return p;
}
static PathPlanInput shape(int P, int max_n) { return PathPlanInput{P, 1002, 1400, 1400, 1000, max_n}; }

static std::map<std::string, long long> fields(const PathPlan& q) {
#define F(x) {#x, (long long)q.x}
    return {F(C), F(nwv), F(wpad), F(dir_words), F(recw), F(layer_stride), F(fdirs_stride), F(rdirs_stride), F(per_read), F(mode),
            F(semi), F(maxmatch), F(gaps_nonpos), F(gaps_agree), F(score_scale), F(use16), F(two_sweep), F(use_rec), F(spec),
            F(pick_two), F(dsel), F(spec4), F(opt16), F(layer16), F(retire), F(use_split), F(gather_ok), F(retire_fwd), F(retire_rev),
            F(retire4), F(dsel4), F(order), F(spec_margin), F(spec4_margin), F(dsel_lo), F(dsel_hi), F(rec_pen), F(fcap), F(rcap),
            F(frec_cap), F(rrec_cap)};
#undef F
}
// names of the fields in which two plans differ
static std::set<std::string> changed(const PathPlan& a, const PathPlan& b) {
    std::set<std::string> out;
    const auto fa = fields(a), fb = fields(b);
    for (const auto& kv : fa) if (fb.at(kv.first) != kv.second) out.insert(kv.first);
    return out;
}
using Names = std::set<std::string>;

static PathPlan plan(const rg_params& p, const PathPlanInput& in, const Options& o, int level = 0, int expect = RG_OK) {
    PathPlan q;
    const int rc = plan_pathwise(p, in, o, level, q);
    if (rc != expect) { ++failures; fprintf(stderr, "plan_pathwise returned %d, expected %d (%s)\n", rc, expect, g_last_error.c_str()); }
    return q;
}

// -m 8, default scores, the headline shapes: packed, two sweeps, records, speculative, two-path picks, words on demand, retirement
static void headline_route() {
    const rg_params p = params(RG_MODE_RECOMBINATION);
    const Options o;
    for (int P : {5, 6, 64})
        for (int max_n : {150, 1000, 1023, 2047}) {
            const PathPlan q = plan(p, shape(P, max_n), o);
            CHECK(q.mode == RG_MODE_RECOMBINATION && !q.semi);                         // drv:168-170
            CHECK(q.nwv == 1 && q.C == (max_n == 150 ? 4 : max_n == 2047 ? 32 : 16));    // drv:172-173, 182
            CHECK(q.wpad == q.C * 64 && q.dir_words == (q.C <= 16 ? 64 : 128) && q.recw == 4 + q.C);   // drv:187-188, 368
            CHECK(q.use16);                                                            // drv:193
            CHECK(q.gaps_nonpos && q.maxmatch == 2 && q.two_sweep);                    // drv:331-338
            CHECK(q.use_rec);                                                          // drv:341
            CHECK(q.spec);                                                             // drv:352
            CHECK(q.score_scale == 1 && q.spec_margin == 112);                         // drv:356-358
            CHECK(q.pick_two);                                                         // drv:361, 473
            CHECK(q.dsel);                                                             // drv:362
            CHECK(!q.spec4 && !q.retire4 && !q.dsel4);                                 // drv:367 (mode 4 only)
            CHECK(q.opt16);                                                            // drv:487
            CHECK(q.gaps_agree && q.layer16);                                          // drv:583-585
            CHECK(q.gather_ok);                                                        // drv:431
            CHECK(q.use_split == (q.C <= 16));                                         // drv:434: the split tables stop at 16 columns per lane (1023 bases)
            CHECK(q.retire && q.retire_fwd && q.retire_rev && q.order);                // drv:437, 516, 540, 479
            CHECK(q.dsel_lo == 1002 / 8 && q.dsel_hi == 1002 - 1 - 1002 / 8);          // drv:443
            CHECK(q.rec_pen == 4 + 1);                                                 // drv:477: 4 + ceil(0.1 * 8)
            CHECK(q.fcap == 1u << 15 && q.rcap == 1u << 16 && q.frec_cap == 1u << 14 && q.rrec_cap == 1u << 13);   // drv:369
            CHECK(q.layer_stride == 1002ll * q.dir_words && q.fdirs_stride == 1400ll * q.dir_words && q.rdirs_stride == q.fdirs_stride);   // drv:315-317
            CHECK(q.per_read == (size_t)(2 * q.fdirs_stride) * 4 + (size_t)q.layer_stride * 8 + (size_t)(P + 2) * q.wpad * 4 +
                                    (size_t)q.wpad * 20 + sizeof(ReadState));          // drv:319-321
            CHECK(q.per_read_all(q.fcap, q.rcap, q.frec_cap, q.rrec_cap) ==
                  q.per_read + ((size_t)1 << 15) * 16 + ((size_t)1 << 16) * 20 + (((size_t)1 << 14) + (1 << 13)) * q.recw * 4);   // drv:378-379
        }
}

// each switch of the GPU switch families flips exactly these fields of the headline plan
static void single_options() {
    const rg_params p = params(RG_MODE_RECOMBINATION);
    const PathPlanInput in = shape(6, 1000);
    const PathPlan base = plan(p, in, Options());
    struct Case { const char* name; int value; Names flips; };
    const Case cases[] = {
        // drv:193 use16 off; with it drv:341, 362, 487, 585, 431, 434; the Cand lists of drv:369; spec (P <= 64) and retire (one wave) stay
        {"sweep_i32", 1, {"use16", "use_rec", "dsel", "opt16", "layer16", "gather_ok", "use_split", "fcap", "rcap"}},
        // drv:338; with it drv:341, 352, 361, 362 and the sizes of drv:369 without records / speculation; retire (drv:437) stays
        {"three_sweeps", 1, {"two_sweep", "use_rec", "spec", "pick_two", "dsel", "rcap", "frec_cap", "rrec_cap"}},
        {"no_frec", 1, {"use_rec", "dsel", "fcap", "rcap"}},                            // drv:341, 362, 369
        {"no_spec", 1, {"spec", "pick_two", "dsel", "frec_cap", "rrec_cap"}},           // drv:352, 361, 362, 369
        {"no_pick2", 1, {"pick_two"}},                                                  // drv:361, 473
        {"no_dsel", 1, {"dsel"}},                                                       // drv:362
        {"no_retire", 1, {"retire", "retire_fwd", "retire_rev"}},                       // drv:437
        {"no_retire", 2, {"retire_rev"}},                                               // drv:540
        {"no_retire", 3, {"retire_fwd"}},                                               // drv:516
        {"no_split", 1, {"use_split"}},                                                 // drv:434
        {"no_gather", 1, {"gather_ok", "use_split"}},                                   // drv:431, 434
        {"layer_i32", 1, {"layer16"}},                                                  // drv:585
        {"no_order", 1, {"order"}},                                                     // drv:479
        {"spec_margin", 0, {"spec_margin", "spec4_margin"}},                            // drv:357-358, 457
        {"dsel_edge", 16, {"dsel_lo", "dsel_hi"}},                                      // drv:443
        {"debug", 1, {}}, {"chunk_reads", 64, {}}, {"stripe_c", 16, {}},                // not the plan's (stripe_c: long reads only, drv:178-181)
    };
    for (const Case& c : cases) {
        Options o;
        const OptionDesc* d = find_option(c.name);
        CHECK(d != nullptr);
        if (!d) continue;
        store_option(o, *d, c.value);
        const Names got = changed(base, plan(p, in, o));
        if (got != c.flips) {
            ++failures;
            fprintf(stderr, "%s = %d flips:", c.name, c.value);
            for (const auto& n : got) fprintf(stderr, " %s", n.c_str());
            fprintf(stderr, "\n");
        }
    }
    // every field that flipped is a switch that went OFF (or a list that went back to its size without records / speculation)
    Options o;
    o.sweep_i32 = 1;
    const PathPlan q = plan(p, in, o);
    CHECK(!q.use16 && !q.use_rec && q.spec && q.retire && q.fcap == 1u << 20 && q.rcap == 1u << 19);      // drv:369
    Options o2;
    o2.no_spec = 1;
    const PathPlan q2 = plan(p, in, o2);
    CHECK(!q2.spec && q2.frec_cap == 1u << 16 && q2.rrec_cap == 1u << 15 && q2.fcap == 1u << 15 && q2.rcap == 1u << 16);   // drv:369
}

static void modes() {
    const Options o;
    const PathPlanInput in = shape(6, 1000);
    // -m 9 / -m 5: the kernels of -m 8 / -m 4 with `semi`; no speculation, no retirement, no split tables (drv:168-170, 352, 367, 434, 437)
    const PathPlan m9 = plan(params(RG_MODE_RECOMBINATION_SEMI), in, o);
    CHECK(m9.mode == RG_MODE_RECOMBINATION && m9.semi && m9.use16 && m9.two_sweep && m9.use_rec);
    CHECK(!m9.spec && !m9.pick_two && !m9.dsel && !m9.use_split && !m9.retire && !m9.retire_fwd && !m9.retire_rev && !m9.spec4);
    CHECK(m9.frec_cap == 1u << 16 && m9.rrec_cap == 1u << 15);
    const PathPlan m5 = plan(params(RG_MODE_PATHWISE_SEMI), in, o);
    CHECK(m5.mode == RG_MODE_PATHWISE && m5.semi && m5.use16 && !m5.spec && !m5.spec4 && !m5.retire4 && !m5.dsel4 && !m5.use_split && !m5.two_sweep);
    // -m 4: the speculative bound under its five conditions (drv:367): global, packed (one wave), gap entries <= 0, first pass, not switched off
    const rg_params p4 = params(RG_MODE_PATHWISE);
    const PathPlan m4 = plan(p4, in, o);
    CHECK(m4.mode == RG_MODE_PATHWISE && m4.spec4 && m4.retire4 && m4.dsel4 && m4.order && !m4.spec && !m4.two_sweep && !m4.retire);
    CHECK(m4.spec4_margin == 280);                                                       // drv:456-457: 112 * 25 / 10
    CHECK(m4.per_read == (size_t)m4.fdirs_stride * 4 + (size_t)m4.layer_stride * 4 + (size_t)8 * m4.wpad * 4 + (size_t)m4.wpad * 20 + sizeof(ReadState));
    CHECK(m4.per_read_all(1, 2, 3, 4) == m4.per_read);                                   // drv:378: lists in -m 8 only
    { Options x; x.sweep_i32 = 1; CHECK(!plan(p4, in, x).spec4); }
    { Options x; x.no_spec = 1; CHECK(!plan(p4, in, x).spec4); }
    CHECK(!plan(p4, in, o, 1).spec4);
    CHECK(!plan(p4, shape(6, 3000), o).spec4);                                           // striped: not packed
    { rg_params g = p4; g.scores[0 * 6 + 5] = g.scores[1 * 6 + 5] = g.scores[2 * 6 + 5] = g.scores[3 * 6 + 5] = g.scores[4 * 6 + 5] = 1;
      const PathPlan q = plan(g, in, o); CHECK(!q.gaps_nonpos && !q.use16 && !q.spec4); }
    { Options x; x.no_retire = 1; const PathPlan q = plan(p4, in, x); CHECK(q.spec4 && !q.retire4 && q.dsel4); }    // drv:459
    { Options x; x.no_dsel = 1; const PathPlan q = plan(p4, in, x); CHECK(q.spec4 && q.retire4 && !q.dsel4); }      // drv:463
    { Options x; x.spec4_margin_x10 = 10; CHECK(plan(p4, in, x).spec4_margin == 112); }
}

static void score_matrices() {
    const Options o;
    // a positive gap entry: three sweeps, no packed rows, no retirement (drv:334, 338, 437; rg_sweep16.hip:1687)
    rg_params g = params(RG_MODE_RECOMBINATION);
    g.scores[5 * 6 + 2] = 1;
    const PathPlan q = plan(g, shape(6, 1000), o);
    CHECK(!q.gaps_nonpos && !q.two_sweep && !q.use16 && !q.use_rec && !q.spec && !q.retire && !q.gaps_agree && !q.layer16);
    CHECK(q.fcap == 1u << 15 && q.rcap == 1u << 19);
    // -200 gaps: outside the 16-bit budget (rg_sweep16.hip:1699-1701) -> i32 rows; speculation up to 64 paths only (drv:352),
    // margin in units of the best match (drv:356-358)
    const rg_params hx = hoxd_like(RG_MODE_RECOMBINATION);
    const PathPlan h6 = plan(hx, shape(6, 150), o), h64 = plan(hx, shape(64, 150), o), h65 = plan(hx, shape(65, 150), o);
    CHECK(!h6.use16 && h6.two_sweep && !h6.use_rec && h6.spec && h6.pick_two && !h6.dsel && h6.retire && !h6.opt16 && !h6.layer16);
    CHECK(h6.maxmatch == 100 && h6.score_scale == 50 && h6.spec_margin == 112 * 50);
    CHECK(h6.fcap == 1u << 20 && h6.rcap == 1u << 19);
    CHECK(h64.spec && h64.retire && !h65.spec && !h65.retire && !h65.pick_two);         // drv:352, 437
    // more than 64 paths on packed rows keep both (drv:352, 437: round 6)
    const PathPlan w = plan(params(RG_MODE_RECOMBINATION), shape(128, 1000), o);
    CHECK(w.use16 && w.spec && w.pick_two && w.dsel && w.retire && w.use_split);
    { Options x; x.sweep_i32 = 1; const PathPlan wi = plan(params(RG_MODE_RECOMBINATION), shape(128, 1000), x); CHECK(!wi.spec && !wi.retire); }
    // scores that can reach 2^23 in the i32 keys are refused (drv:194-200): (1000 + 1000 + 2) * 5000 >= 2^23
    plan(params(RG_MODE_RECOMBINATION, 5000, -4), shape(6, 1000), o, 0, RG_ERR_CAPACITY);
    CHECK(g_last_error == "scores of this batch can reach 2^23 in magnitude: outside the 32-bit (value, path) keys of the pathwise kernels");
    plan(params(RG_MODE_RECOMBINATION, 4000, -4), shape(6, 1000), o);                    // 2002 * 4000 < 2^23
}

static void long_reads() {
    const rg_params p = params(RG_MODE_RECOMBINATION);
    const Options o;
    // drv:172-183: stripes of 1024 columns up to 8191 bases, 2048 beyond, at most 8 waves
    const int ns[] = {2048, 8191, 8192, 16383}, cs[] = {16, 16, 32, 32}, ws[] = {3, 8, 5, 8};
    for (int i = 0; i < 4; ++i) {
        const PathPlan q = plan(p, shape(6, ns[i]), o);
        CHECK(q.C == cs[i] && q.nwv == ws[i] && q.wpad == ws[i] * cs[i] * 64 && q.dir_words == ws[i] * 64 * (cs[i] <= 16 ? 1 : 2));
        // striped: i32 rows and Cand lists, still two sweeps on a speculative bound with the margin scaled by the length
        // (drv:193, 338, 352, 357); retirement at <= 16 columns per lane (drv:437)
        CHECK(!q.use16 && q.two_sweep && !q.use_rec && q.spec && !q.dsel && !q.opt16 && !q.layer16 && !q.use_split && !q.gather_ok);
        CHECK(q.retire == (cs[i] <= 16));
        CHECK(q.spec_margin == 112 * ((ns[i] + 999) / 1000));
    }
    plan(p, shape(6, 16384), o, 0, RG_ERR_ARG);
    CHECK(g_last_error == "reads longer than 16383 bases are not supported by the pathwise kernels");
    // stripe_c applies only where the read fits 8 stripes of that width (drv:180), and never to reads of one wave
    { Options x; x.stripe_c = 8; CHECK(plan(p, shape(6, 4000), x).C == 8 && plan(p, shape(6, 4000), x).nwv == 8); CHECK(plan(p, shape(6, 5000), x).C == 16); CHECK(plan(p, shape(6, 1000), x).C == 16); }
    { Options x; x.stripe_c = 32; CHECK(plan(p, shape(6, 3000), x).C == 32 && plan(p, shape(6, 3000), x).nwv == 2); }
    { Options x; x.stripe_c = 16; CHECK(plan(p, shape(6, 9000), x).C == 32); }
    { Options x; x.stripe_c = 12; CHECK(plan(p, shape(6, 3000), x).C == 16); }
    // long reads need a uniform read-gap cost (drv:184-186); reads of one wave do not
    rg_params g = p;
    g.scores[2 * 6 + 5] = -6;
    plan(g, shape(6, 2048), o, 0, RG_ERR_ARG);
    CHECK(g_last_error == "reads longer than 2047 bases need a uniform read-gap cost");
    CHECK(!plan(g, shape(6, 2047), o).use16);                                            // (and no packed rows: rg_sweep16.hip:1686)
}

static void second_pass_levels() {
    const rg_params p = params(RG_MODE_RECOMBINATION);
    const Options o;
    const PathPlan l0 = plan(p, shape(6, 1500), o), l1 = plan(p, shape(6, 1500), o, 1), l2 = plan(p, shape(6, 1500), o, 2);
    CHECK(l0.spec_margin == 112 && l1.spec_margin == 112 + 320 * 2);                     // drv:357-358
    CHECK(l1.spec && l1.pick_two && !l1.dsel && l1.retire);                              // drv:352, 362: every word the second time
    CHECK(!l2.spec && !l2.pick_two && !l2.dsel && l2.retire && l2.use_rec);              // drv:348
    CHECK(l2.frec_cap == 1u << 16 && l2.rrec_cap == 1u << 15);                           // drv:369
    CHECK(changed(l0, l1) == (Names{"dsel", "spec_margin", "spec4_margin"}));
    // a margin of 0 (the tests' way to force the second pass) is not scaled (drv:358)
    Options z;
    z.spec_margin = 0;
    CHECK(plan(hoxd_like(RG_MODE_RECOMBINATION), shape(6, 150), z).spec_margin == 0);
    CHECK(plan(hoxd_like(RG_MODE_RECOMBINATION), shape(6, 150), z, 1).spec_margin == 320);
}

// even_chunks (rg_host.hpp): the reads per launch of both batch drivers — as few launches as `maxchunk` allows, no short tail
static void even_launches() {
    for (long long n = 1; n <= 300; ++n)
        for (long long maxchunk = 1; maxchunk <= 300; ++maxchunk) {
            const long long chunk = even_chunks(n, maxchunk);
            const long long launches = (n + chunk - 1) / chunk, last = n - (launches - 1) * chunk;
            if (!(1 <= chunk && chunk <= maxchunk) || launches != (n + maxchunk - 1) / maxchunk || !(1 <= last && last <= chunk)) {
                ++failures;
                fprintf(stderr, "even_chunks(%lld, %lld) = %lld: %lld launches, the last of %lld\n", n, maxchunk, chunk, launches, last);
            }
        }
    CHECK(even_chunks(5, 2) == 2);
    CHECK(even_chunks(10000, 8192) == 5000);
    CHECK(even_chunks(7, 100) == 7);
}

int main() {
    even_launches();
    headline_route();
    single_options();
    modes();
    score_matrices();
    long_reads();
    second_pass_levels();
    return finish("plan ok");
}
