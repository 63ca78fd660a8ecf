// What plan_pathwise answers to every affine-gap pathwise mode at every amb_mode, length class and gap sign: one line per combination,
//   mode amb n o e -> rc | g_last_error             (a refusal)
//   mode amb n o e -> 0 |  | C nwv gap_xlong gdirs_stride gbnd_stride gdbnd_stride gckpt_stride gwalk_bytes per_read semi local
// tests/test_gap_mode_table_cpu.py compares the output with tests/golden/gap_plan_refusals.txt byte for byte.
#include "plan_check_common.hpp"

using namespace gap_check;

int main() {
    const int modes[] = {RG_MODE_PATHWISE_GAP, RG_MODE_PATHWISE_GAP_SEMI, RG_MODE_PATHWISE_GAP_LOCAL,
                         RG_MODE_PATHWISE_GAP_LONG, RG_MODE_PATHWISE_GAP_SEMI_LONG, RG_MODE_PATHWISE_GAP_LOCAL_LONG,
                         RG_MODE_PATHWISE_GAP_STRANDS, RG_MODE_PATHWISE_GAP_SEMI_STRANDS, RG_MODE_PATHWISE_GAP_LOCAL_STRANDS,
                         RG_MODE_PATHWISE_GAP_XLONG, RG_MODE_PATHWISE_GAP_SEMI_XLONG, RG_MODE_PATHWISE_GAP_LOCAL_XLONG,
                         RG_MODE_PATHWISE_GAP_XSTRANDS, RG_MODE_PATHWISE_GAP_SEMI_XSTRANDS, RG_MODE_PATHWISE_GAP_LOCAL_XSTRANDS};
    const int gaps[][2] = {{-4, -2}, {1, -2}};
    for (int mode : modes)
        for (int amb : {0, 1, 2, 3, 4, 8, 12})
            for (int n : {1, 2047, 2048, 16383, 16384, 131071, 131072})
                for (const auto& oe : gaps) {
                    PathPlan q;
                    const int rc = run(params(mode, oe[0], oe[1], amb), shape(n), q);
                    printf("%d %d %d %d %d -> %d | %s", mode, amb, n, oe[0], oe[1], rc, rc == RG_OK ? "" : g_last_error.c_str());
                    if (rc == RG_OK)
                        printf(" | %d %d %d %lld %lld %lld %lld %zu %zu %d %d", q.C, q.nwv, (int)q.gap_xlong, q.gdirs_stride, q.gbnd_stride,
                               q.gdbnd_stride, q.gckpt_stride, q.gwalk_bytes, q.per_read, (int)q.semi, (int)q.local);
                    putchar('\n');
                }
    return 0;
}
