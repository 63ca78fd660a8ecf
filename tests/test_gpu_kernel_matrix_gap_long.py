"""GPU: every instantiation of the long-read gap kernels (tests/kernel_matrix_gap_long.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on (run_case of tests/kernel_matrix_checks.py), every read is
checked against the rule (check_reads of tests/pathwise_support.py: whole line, re-scored CIGAR, status), and EVERY batch of the case —
one per boundary length — must have launched the entry's instantiation.  Cases that several entries share run once."""
import pytest

import kernel_matrix_gap_long as KG
from kernel_matrix_checks import run_case

pytestmark = pytest.mark.gpu
_RESULTS = {}


@pytest.mark.parametrize("name", sorted(KG.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KG.MATRIX[name]
    mode = KG.CASES[cid].mode
    kind = (16, 17, 22).index(mode)
    per_batch, coarse = run_case(KG, cid, _RESULTS)
    assert len(per_batch) == len(KG.CASES[cid].batches)
    for b in per_batch:
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        # nothing but the striped kernels of this kind and the base mode's pick
        assert set(b) == {"rg::k_gap_score_long<%d>" % kind, KG.PICK[mode], "rg::k_gap_dirs_long<%d>" % kind, KG.TRACE[mode]}, sorted(b)
    assert {"k_gap_score_long", "k_gap_dirs_long"} <= coarse
