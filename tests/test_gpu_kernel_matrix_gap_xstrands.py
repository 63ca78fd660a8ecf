"""GPU: every instantiation of recgraph_amd/csrc/gap_xstrands/rg_gap_xstrands.hip (tests/kernel_matrix_gap_xstrands.py) ran and was
right.

One test per entry: the entry's case is aligned with the launch log on, every read is checked against the composed rule (check_x of
tests/pathwise_support.py: whole line, status, strand and score accessors, re-scored CIGAR on the chosen strand, both
counters), and EVERY batch of the case must have launched the entry's instantiation — the pick twice out and once in, the duel and
the marks once — and no merge."""
import pytest

import kernel_matrix_gap_xstrands as KX
from pathwise_support import check_x, graph_tuple, run_batch_strands

pytestmark = pytest.mark.gpu
_RESULTS = {}
LAUNCHES = {"rg::k_gap_pick_out": 2, "rg::k_gap_seed_pick": 1, "rg::k_gap_xstrands_duel": 1, "rg::k_gap_xstrands_mark": 1}


def _run_case(cid):
    if cid in _RESULTS:
        return _RESULTS[cid]
    case = KX.CASES[cid]
    g, batches = KX.build(case)
    graph = graph_tuple(g)
    per_batch = []
    for reads in batches:
        res = run_batch_strands(graph[1], reads, case.mode, log=True, **case.kw)
        check_x(graph, reads, case.mode, res)
        per_batch.append(res)
    _RESULTS[cid] = per_batch
    return per_batch


@pytest.mark.parametrize("name", sorted(KX.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KX.MATRIX[name]
    per_batch = _run_case(cid)
    assert len(per_batch) == len(KX.CASES[cid].batches)
    for res in per_batch:
        assert res["inst"].get(name, 0) == LAUNCHES[name], (name, cid, sorted(res["inst"].items()))
        assert "rg::k_strand_merge" not in res["inst"] and res["inst"].get("rg::k_revcomp") == 1 and res["inst"].get("rg::k_strand_orient") == 1
        assert res["stats"][name[4:]] == LAUNCHES[name]
    local = KX.CASES[cid].mode == 82
    assert all(("rg::k_gap_strands_gate" in res["inst"]) == local and ("rg::k_strand_gate" in res["inst"]) != local for res in per_batch)
    # the small batch's stages are striped (both picks: the 2100-base read goes both ways), the big one's are not
    kind = 2 if local else 1
    assert per_batch[1]["inst"].get("rg::k_gap_score_long<%d>" % kind) == 2 and per_batch[1]["inst"].get("rg::k_gap_ckpt_long<%d>" % kind) == 1
    assert not any(k.startswith("rg::k_gap_score_long") or k.startswith("rg::k_gap_ckpt_long") for k in per_batch[0]["inst"])
