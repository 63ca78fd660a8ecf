"""GPU: every instantiation of the edit-distance kernels (tests/kernel_matrix_edit.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on, every read is checked against the rule (check_edit of
tests/test_gpu_pathwise_edit.py: whole line, re-scored CIGAR, status), and EVERY batch of the case — one per side of the width's
boundary — must have launched the entry's instantiation, and nothing but the four kernels of its (mode, W).  Cases that several entries
share run once."""
import pytest

import kernel_matrix_edit as KE
from test_gpu_pathwise_edit import EDIT_KERNELS, run_matrix_case

pytestmark = pytest.mark.gpu
_RESULTS = {}


@pytest.mark.parametrize("name", sorted(KE.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KE.MATRIX[name]
    case = KE.CASES[cid]
    per_batch, coarse = run_matrix_case(cid, _RESULTS)
    assert len(per_batch) == len(case.batches) == 2
    for b in per_batch:
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        assert set(b) == KE.instantiations(case), sorted(b)
    assert coarse == EDIT_KERNELS
