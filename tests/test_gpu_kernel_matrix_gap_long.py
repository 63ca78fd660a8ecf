"""GPU: every instantiation of the long-read gap kernels (tests/kernel_matrix_gap_long.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on, every read is checked against the rule (check_long of
tests/test_gpu_pathwise_gap_long.py: whole line, re-scored CIGAR, status), and EVERY batch of the case — one per boundary length —
must have launched the entry's instantiation.  Cases that several entries share run once."""
import pytest

import kernel_matrix_gap_long as KG
import pathwise_gap_rule as R
from test_gpu_pathwise_gap_long import check_long

pytestmark = pytest.mark.gpu
_RESULTS = {}


def _run_case(cid):
    if cid in _RESULTS:
        return _RESULTS[cid]
    from recgraph_amd import api
    case = KG.CASES[cid]
    g, batches = KG.build(case)
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    graph = (g, gg, lnz, rows, R.graph_node_ids(gg))
    per_batch, coarse = [], set()
    try:
        api.set_option("launch_log", 1)
        for reads in batches:
            b = api.Batch(gg, reads, api.make_params(case.mode, **case.kw))
            b.run()
            b.fetch()
            status = [b.status(i) for i in range(len(reads))]
            assert status == [0] * len(reads), cid
            texts = [b.gaf_text(i, "r%d" % i, i + 1) for i in range(len(reads))]
            stats = b.kernel_stats()
            per_batch.append({k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")})
            coarse |= {k for k in stats if not k.startswith("inst:")}
            api.set_option("launch_log", 0)
            check_long(graph, reads, case.mode, texts=texts, status=status, **case.kw)
            api.set_option("launch_log", 1)
    finally:
        api.set_option("launch_log", 0)
    _RESULTS[cid] = (per_batch, coarse)
    return _RESULTS[cid]


@pytest.mark.parametrize("name", sorted(KG.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KG.MATRIX[name]
    mode = KG.CASES[cid].mode
    kind = (16, 17, 22).index(mode)
    per_batch, coarse = _run_case(cid)
    assert len(per_batch) == len(KG.CASES[cid].batches)
    for b in per_batch:
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        # nothing but the striped kernels of this kind and the base mode's pick
        assert set(b) == {"rg::k_gap_score_long<%d>" % kind, KG.PICK[mode], "rg::k_gap_dirs_long<%d>" % kind, KG.TRACE[mode]}, sorted(b)
    assert {"k_gap_score_long", "k_gap_dirs_long"} <= coarse
