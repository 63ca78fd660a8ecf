"""GPU: every instantiation of the one-stripe traceback kernels (tests/kernel_matrix_gap_xlong.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on (run_case of tests/kernel_matrix_checks.py), every read is
checked against the rule (check_reads of tests/pathwise_support.py: whole line, re-scored CIGAR, status), and EVERY batch of the case —
one per length — must have launched the entry's instantiation.  Cases that several entries share run once."""
import pytest

import kernel_matrix_gap_xlong as KX
from kernel_matrix_checks import run_case

pytestmark = pytest.mark.gpu
_RESULTS = {}


@pytest.mark.parametrize("name", sorted(KX.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KX.MATRIX[name]
    mode = KX.CASES[cid].mode
    kind = (56, 57, 62).index(mode)
    per_batch, coarse = run_case(KX, cid, _RESULTS)
    assert len(per_batch) == len(KX.CASES[cid].batches)
    for b, longest in zip(per_batch, KX.CASES[cid].batches):
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        # nothing but the score pass of this kind, the base mode's pick and the new kernels of this kind
        assert set(b) == {KX.SCORE[mode], KX.PICK[mode], "rg::k_gap_ckpt_long<%d>" % kind, "rg::k_gap_redo_long<%d>" % kind, KX.WALK[mode]}, sorted(b)
        # one rebuild and one walk launch per stripe of the batch's longest read, one checkpoint pass
        stripes = (longest + 2048) // 2048
        assert (b["rg::k_gap_ckpt_long<%d>" % kind], b["rg::k_gap_redo_long<%d>" % kind], b[KX.WALK[mode]]) == (1, stripes, stripes), sorted(b.items())
    assert {"k_gap_score_long", "k_gap_ckpt_long", "k_gap_redo_long"} <= coarse and not {"k_gap_dirs_long", "k_gap_trace_long", "k_gap_trace_local_long"} & coarse
