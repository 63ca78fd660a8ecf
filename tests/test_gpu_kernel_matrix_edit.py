"""GPU: every instantiation of the edit-distance kernels (tests/kernel_matrix_edit.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on (run_case of tests/kernel_matrix_checks.py), every read is
checked against the rule (check_edit of tests/pathwise_support.py: whole line, re-scored CIGAR, status), and EVERY batch of the case —
one per side of the width's boundary — must have launched the entry's instantiation, and nothing but the four kernels of its (mode, W).
Cases that several entries share run once."""
import pytest

import kernel_matrix_edit as KE
from kernel_matrix_checks import run_case
from pathwise_support import EDIT_KERNELS, check_edit, run_batch_unit

pytestmark = pytest.mark.gpu
_RESULTS = {}


@pytest.mark.parametrize("name", sorted(KE.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KE.MATRIX[name]
    case = KE.CASES[cid]
    per_batch, coarse = run_case(KE, cid, _RESULTS, lambda gg, reads, case: run_batch_unit(gg, reads, case.mode),
                                 lambda graph, reads, case, run: check_edit(graph, reads, case.mode, out=run))
    assert len(per_batch) == len(case.batches) == 2
    for b in per_batch:
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        assert set(b) == KE.instantiations(case), sorted(b)
    assert coarse == EDIT_KERNELS
