"""GPU: every instantiation of the local gap kernels (tests/kernel_matrix_gap_local.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on (run_case of tests/kernel_matrix_checks.py), every read is
checked against the rule (check_local of tests/pathwise_support.py: whole line, re-scored CIGAR, status), and EVERY batch of the case
— one per boundary length — must have launched the entry's instantiation.  Cases that several entries share run once."""
import pytest

import kernel_matrix_gap_local as KL
from kernel_matrix_checks import run_case
from pathwise_support import check_local

pytestmark = pytest.mark.gpu
_RESULTS = {}


def _check(graph, reads, case, run):
    check_local(graph, reads, texts=run.texts, status=run.status, **case.kw)
    # the flanked read is clipped on both sides; a whole path ends on its last column
    f = run.texts[0].split("\t")
    assert int(f[2]) > 0 and int(f[3]) < len(reads[0]) - 1, f[:4]


@pytest.mark.parametrize("name", sorted(KL.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KL.MATRIX[name]
    per_batch, coarse = run_case(KL, cid, _RESULTS, check=_check)
    assert len(per_batch) == len(KL.CASES[cid].batches)
    for b in per_batch:
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        # nothing but the local gap kernels of this C
        assert len(b) == 4 and all("k_gap_" in k and "_local" in k for k in b), sorted(b)
    assert {"k_gap_score_local", "k_gap_pick_local", "k_gap_dirs_local", "k_gap_trace_local"} <= coarse
