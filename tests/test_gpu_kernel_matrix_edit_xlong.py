"""GPU: every instantiation of the striped edit-distance kernels (tests/kernel_matrix_edit_xlong.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on (run_case of tests/kernel_matrix_checks.py), every read is
checked against the rule of modes 6 / 7 at unit costs (check_reads of tests/pathwise_support.py: whole line, re-scored CIGAR, status),
and EVERY batch of the case — 16384 bases and 32769 — must have launched the entry's instantiation, and nothing but the four kernels of
its mode.  Cases that several entries share run once."""
import pytest

import kernel_matrix_edit_xlong as KX
from kernel_matrix_checks import run_case
from pathwise_support import check_reads, run_batch_unit, unit_costs

pytestmark = pytest.mark.gpu
_RESULTS = {}
XLONG_KERNELS = {"k_edit_score_xlong", "k_gap_pick", "k_edit_redo_xlong", "k_edit_walk_xlong"}


def _check(graph, reads, case, run):
    from recgraph_amd import api
    check_reads(graph, reads, api._lib.GAP_SEMI if KX.MODES[case.mode] else api._lib.GAP_GLOBAL, unit_costs(), 0, -1, texts=run.texts, status=run.status)


@pytest.mark.parametrize("name", sorted(KX.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KX.MATRIX[name]
    case = KX.CASES[cid]
    per_batch, coarse = run_case(KX, cid, _RESULTS, lambda gg, reads, case: run_batch_unit(gg, reads, case.mode), _check)
    assert len(per_batch) == len(case.batches) == 2
    for b in per_batch:
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        assert set(b) == KX.instantiations(case), sorted(b)
    assert coarse == XLONG_KERNELS
