"""GPU: every instantiation of the both-strands edit-distance kernels (tests/kernel_matrix_edit_strands.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on (run_case of tests/kernel_matrix_checks.py), every read is
checked against the exact rule of mode 26 / 27 at unit costs (whole line — the strand column included —, status, score, both cell
counters), and EVERY batch of the case — one per side of the width's boundary — must have launched the entry's instantiation, and
nothing but the seven kernels of its (mode, W).  Cases that several entries share run once."""
import pytest

import kernel_matrix_edit_strands as KS
import pathwise_edit_strands_rule as ES
import pathwise_gap_strands_rule as S
from edit_strands_support import KERNELS, expect, instantiations
from kernel_matrix_checks import run_case
from pathwise_support import run_batch_unit

pytestmark = pytest.mark.gpu
_RESULTS = {}


def _check(graph, reads, case, run):
    from recgraph_amd import api
    exp = expect(graph, reads, case.mode)
    assert run.texts == [x[0] for x in exp], (case.mode, [i for i in range(len(reads)) if run.texts[i] != exp[i][0]])
    assert run.status == [x[1] for x in exp] and run.scores == [S.score_of(x[0]) for x in exp], (run.status, run.scores)
    want = ES.counters(case.mode, reads, exp, graph[2], graph[3], api._table_from_dict(api.create_score_matrix_i32(0, -1)))
    assert (run.counted, run.performed) == want, (run.counted, run.performed, want)
    if len(reads) > 1:
        assert {x[2] for x in exp} == {"+", "-"}, [x[2] for x in exp]


@pytest.mark.parametrize("name", sorted(KS.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KS.MATRIX[name]
    case = KS.CASES[cid]
    per_batch, coarse = run_case(KS, cid, _RESULTS, lambda gg, reads, case: run_batch_unit(gg, reads, case.mode), _check)
    assert len(per_batch) == len(case.batches) == 2
    for b, longest in zip(per_batch, case.batches):
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        assert set(b) == instantiations(case.mode, longest), sorted(b)
    assert coarse == KERNELS
