// What plan_pathwise answers to every edit-distance pathwise mode at every amb_mode, length class and scoring: one line per combination,
//   mode amb n scoring -> rc | g_last_error             (a refusal)
//   mode amb n scoring -> 0 |  | edit_xlong edit_words C nwv wpad gdirs_stride edit_slot_words edit_bnd_stride gwalk_bytes per_read semi
// tests/test_edit_mode_table_cpu.py compares the output with tests/golden/edit_plan_refusals.txt byte for byte.
#include "plan_check_common.hpp"

using namespace gap_check;

// match 0, mismatch -1, o = 0, e = -1, and what each scoring changes of it
static rg_params scoring(int mode, int amb, int which) {
    rg_params p = which == 1 ? params(mode, -4, -2, amb) : score_params(mode, 0, -1);
    if (which == 1) return p;                    // the default scores
    p.amb_mode = amb;
    p.gap_open = which == 2 ? -1 : which == 4 ? 1 : 0;
    p.gap_ext = which == 3 ? 0 : -1;
    if (which == 5) p.scores[4 * 6 + 4] = 0;     // N matches N
    if (which == 6) p.scores[2 * 6 + 4] = -2;    // an N entry is inside the ACGTN block
    return p;
}

int main() {
    const char* const names[] = {"unit", "default", "o=-1", "e=0", "o=1", "N=N", "GN=-2"};
    for (int mode : {RG_MODE_PATHWISE_EDIT, RG_MODE_PATHWISE_EDIT_SEMI, RG_MODE_PATHWISE_EDIT_XLONG, RG_MODE_PATHWISE_EDIT_SEMI_XLONG})
        for (int amb : {0, 1, 2, 3, 4, 8, 12})
            for (int n : {1, 2048, 16383, 16384, 131071, 131072})
                for (int s = 0; s < 7; ++s) {
                    PathPlan q;
                    const int rc = run(scoring(mode, amb, s), shape(n), q);
                    printf("%d %d %d %s -> %d | %s", mode, amb, n, names[s], rc, rc == RG_OK ? "" : g_last_error.c_str());
                    if (rc == RG_OK)
                        printf(" | %d %d %d %d %d %lld %d %lld %zu %zu %d", (int)q.edit_xlong, q.edit_words, q.C, q.nwv, q.wpad, q.gdirs_stride,
                               q.edit_slot_words, q.edit_bnd_stride, q.gwalk_bytes, q.per_read, (int)q.semi);
                    putchar('\n');
                }
    return 0;
}
