"""GPU: every instantiation of recgraph_amd/csrc/gap_strands/rg_gap_strands.hip (tests/kernel_matrix_gap_strands.py) ran and was
right.

One test per entry: the entry's case is aligned with the launch log on, every read is checked against the composed rule
(check_strands of tests/pathwise_support.py: whole line, status, strand and score accessors, re-scored CIGAR on the
chosen strand), and EVERY batch of the case must have launched the entry's instantiation — and not the gate of the other modes."""
import pytest

import kernel_matrix_gap_strands as KS
from pathwise_support import check_strands, graph_tuple, run_batch_strands

pytestmark = pytest.mark.gpu
_RESULTS = {}


def _run_case(cid):
    if cid in _RESULTS:
        return _RESULTS[cid]
    case = KS.CASES[cid]
    g, batches = KS.build(case)
    graph = graph_tuple(g)
    per_batch = []
    for reads in batches:
        res = run_batch_strands(graph[1], reads, case.mode, log=True, **case.kw)
        check_strands(graph, reads, case.mode, res)
        per_batch.append(res)
    _RESULTS[cid] = per_batch
    return per_batch


@pytest.mark.parametrize("name", sorted(KS.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KS.MATRIX[name]
    per_batch = _run_case(cid)
    assert len(per_batch) == len(KS.CASES[cid].batches)
    for res in per_batch:
        assert res["inst"].get(name, 0) == 1, (name, cid, sorted(res["inst"].items()))
        assert "rg::k_strand_gate" not in res["inst"] and res["inst"].get("rg::k_revcomp") == 1 and res["inst"].get("rg::k_strand_merge") == 1
        assert res["stats"]["k_gap_strands_gate"] == 1
    # the small batch's second pass is striped, the big one's is not
    assert per_batch[1]["inst"].get("rg::k_gap_score_long<2>") == 2 and not any(k.startswith("rg::k_gap_score_long") for k in per_batch[0]["inst"])
