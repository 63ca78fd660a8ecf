"""GPU: every instantiation of the gap kernels (tests/kernel_matrix_gap.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on (run_case of tests/kernel_matrix_checks.py), every read is
checked against the rule (check_base of tests/pathwise_support.py: whole line, comments column, re-scored CIGAR, status), and EVERY
batch of the case — one per boundary length — must have launched the entry's instantiation.  Cases that several entries share run once."""
import pytest

import kernel_matrix_gap as KG
from kernel_matrix_checks import run_case
from pathwise_support import check_base

pytestmark = pytest.mark.gpu
_RESULTS = {}


def _check(graph, reads, case, run):
    check_base(graph, reads, case.mode == 7, texts=run.texts, status=run.status, **case.kw)


@pytest.mark.parametrize("name", sorted(KG.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KG.MATRIX[name]
    per_batch, coarse = run_case(KG, cid, _RESULTS, check=_check)
    assert len(per_batch) == len(KG.CASES[cid].batches)
    for b in per_batch:
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        # nothing but the gap kernels of this C and end rule
        assert len(b) == 4 and all("k_gap_" in k for k in b), sorted(b)
    assert {"k_gap_score", "k_gap_pick", "k_gap_dirs", "k_gap_trace"} <= coarse
