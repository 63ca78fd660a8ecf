// The plan of a one-path -m 8 batch as tests/test_gpu_forward_bound.py runs it (recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise, host
// arithmetic only):   forward_bound_plan <rows of the graph> <longest read> [option=value ...]
// prints "C nwv use16 opt16 spec dsel spec_margin" — the fields that decide which bound kernel the batch launches and whether k_verify
// looks at the bound alone.
#include <cstdlib>
#include <string>

#include "plan_check_common.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int L = atoi(argv[1]), max_n = atoi(argv[2]);
    Options o;
    for (int k = 3; k < argc; ++k) {
        const char* eq = strchr(argv[k], '=');
        if (!eq) return 2;
        const OptionDesc* d = find_option(std::string(argv[k], (size_t)(eq - argv[k])).c_str());
        if (!d) { fprintf(stderr, "no option %s\n", argv[k]); return 2; }
        store_option(o, *d, atoi(eq + 1));
    }
    // the default scores (score_matrix.rs:35-66: match 2, mismatch -4, any pairing with '-' twice the mismatch)
    rg_params p = score_params(RG_MODE_RECOMBINATION);
    p.base_rec_cost = 4;
    p.multi_rec_cost = 0.1f;
    p.rec_band_width = 1.0f;
    PathPlan q;
    // one path through every row: one direction-word slot per row
    const int rc = plan_pathwise(p, PathPlanInput{1, L, L, L, L, max_n}, o, 0, q);
    if (rc != RG_OK) { fprintf(stderr, "plan_pathwise: %d (%s)\n", rc, g_last_error.c_str()); return 1; }
    printf("%d %d %d %d %d %d %d\n", q.C, q.nwv, (int)q.use16, (int)q.opt16, (int)q.spec, (int)q.dsel, q.spec_margin);
    return 0;
}
