"""CPU: the rule of -m 12 (tests/pathwise_gap_local_rule.py) against hand-checked lines and a plain scalar Smith-Waterman-Gotoh, the
admission and the refusals of rg_batch_create (answered before a device is needed), the plan's routes
(tests/c/gap_local_plan_check.cpp), the CLI's parser and the registers of the new kernels."""
import numpy as np
import pytest

import plan_check_build

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
from pathwise_support import DIAMOND, TWO_BUBBLES, assert_rows_in_registers, create_rc, no_device

COSTS = [(-4, -2), (0, -2), (-6, 0), (-40, -1), (0, 0)]


def _graph(gfa):
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(gfa)
    lnz, rows = R.graph_paths(g)
    return lnz, rows, R.graph_node_ids(g)


def test_the_row_step_is_smith_waterman_gotoh():
    """H of every cell: X through one maximum.accumulate over the CLAMPED H' equals the cell-by-cell recurrence (exact because o <= 0),
    o = 0 and e = 0 included."""
    rng = np.random.default_rng(12)
    for t in range(300):
        b = "".join("ACGTN"[int(x)] for x in rng.integers(0, 5, size=int(rng.integers(1, 14))))
        r = "".join("ACGTN"[int(x)] for x in rng.integers(0, 5, size=int(rng.integers(1, 14))))
        o, e = COSTS[t % 5]
        full = L.path_rows(b, r, R.default_scores(), o, e)
        assert [[int(v) for v in f[0]] for f in full] == L.naive_local(b, r, R.default_scores(), o, e), (b, r, o, e)


def test_hand_checked_lines():
    lnz, rows, ids = _graph(DIAMOND)
    # clipped flanks: the ATG of path 0 sits at read columns 3 .. 5
    assert L.line_local(lnz, rows, ids, "n", "CCATGCC") == "n\t7\t2\t4\t+\t>1>2>4\t3\t0\t2\t0\t*\t*\t3M, best path: 0, score: 6\tATG\n"
    # nothing clipped: the -m 7 line
    assert L.line_local(lnz, rows, ids, "n", "ATG") == R.line(lnz, rows, ids, "n", "ATG", semi=True)
    # all N: no cell above 0
    assert L.align_local(lnz, rows, "NNN") is None and L.line_local(lnz, rows, ids, "n", "NNN") == ""
    # the G of row 4 is the same cell on both paths: the lowest path index wins
    assert L.align_local(lnz, rows, "G") == (2, 0, 4, 1, 0, "D", "G")
    assert L.line_local(lnz, rows, ids, "n", "TTCGTT") == "n\t6\t2\t3\t+\t>3>4\t2\t0\t1\t0\t*\t*\t2M, best path: 1, score: 4\tCG\n"
    lnz, rows, ids = _graph(TWO_BUBBLES)
    assert L.line_local(lnz, rows, ids, "n", "GGATGATCC") == "n\t9\t2\t6\t+\t>1>2>4>5>7\t5\t0\t4\t0\t*\t*\t5M, best path: 0, score: 10\tATGAT\n"
    # A scores 2 on rows 1 (both paths) and 5 (path 0): the smallest row, then the lowest path
    assert L.align_local(lnz, rows, "A") == (2, 0, 1, 1, 0, "D", "A")
    # both columns of AA reach 2 on row 1: the smallest column
    assert L.align_local(lnz, rows, "AA")[3:5] == (1, 0)
    assert L.align_local(lnz, rows, "NNNN") is None
    # a gap inside a local alignment is kept when the flanks pay for it: ATG + 1 inserted base + AT, 5 matches + o + e = 10 - 6
    score, k, end_row, end_col, stop_col, ops, pseq = L.align_local(lnz, rows, "CCATGGATCC")
    assert (score, k, end_col, stop_col, ops[::-1], pseq) == (6, 0, 5, 2, "DDD", "ATG")
    score, k, end_row, end_col, stop_col, ops, pseq = L.align_local(lnz, rows, "CCATGGATCC", R.default_scores(5, -4))
    assert (score, k, end_col, stop_col, ops[::-1], pseq) == (19, 0, 8, 2, "DDLDDD", "ATGAT")        # walking back, D wins: the read's FIRST G is the inserted base
    assert L.rescore("2M1D3M", "ATGAT", "CCATGGATCC", 2, 7, R.default_scores(5, -4)) == (19, 6, 5)


def test_mode_12_is_admitted_and_refuses_before_a_device_is_needed():
    from recgraph_amd import api
    mode = api.MODE_PATHWISE_GAP_LOCAL
    assert mode == 12 == api._lib.MODE_PATHWISE_GAP_LOCAL and api.READ_UNALIGNED == 16 == api._lib.READ_UNALIGNED
    rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode)
    # (on the parent commit: RG_ERR_ARG "unsupported mode")
    assert rc == (-3 if no_device() else 0), (rc, msg)
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=1)[0] == -1
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, e=1)[0] == -1
    for amb in (1, 2, 4, 8, 12):
        assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, amb=amb)[0] == -1, amb
    rc, msg = create_rc(TWO_BUBBLES, ["A" * 2048], mode)
    assert rc == -1 and "2047" in msg, (rc, msg)
    assert create_rc(TWO_BUBBLES, ["A" * 2047], mode)[0] == (-3 if no_device() else 0)
    # (5 rows + 5 bases) * 2^25 >= 2^28
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25)[0] == -5
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=-(1 << 25))[0] == -5
    # no mode between the families was admitted by accident
    for other in (13, 14, -1):
        rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], other)
        assert rc == -1 and "unsupported mode" in msg


def test_modes_6_and_7_refuse_what_they_refused():
    from recgraph_amd import api
    for mode in (api.MODE_PATHWISE_GAP, api.MODE_PATHWISE_GAP_SEMI):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * 2048], mode)
        assert rc == -1 and "(-m 6 / -m 7)" in msg, (rc, msg)
        rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode, amb=4)
        assert rc == -1 and "(-m 6 / -m 7)" in msg, (rc, msg)
        assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=1)[0] == -1
        assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25)[0] == -5


def test_no_new_entry_point():
    from recgraph_amd import _lib
    assert len(_lib.SYMBOLS) == 63


def test_the_api_refuses_both_strands():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
        with pytest.raises(api._lib.RecGraphError):
            fn(g, ["ATG"], mode=api.MODE_PATHWISE_GAP_LOCAL, both_strands=True)
        with pytest.raises(api._lib.RecGraphError):
            fn(g, ["ATG"], mode=api.MODE_PATHWISE_GAP_LOCAL, strand_vote=True)
    assert callable(api.pathwise_alignment_gap_local_exec)


def test_the_cli_takes_the_mode():
    from recgraph_amd import cli
    a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", "12", "-O", "6", "-E", "1"])
    assert a.alignment_mode == 12 and (a.gap_open, a.gap_extension) == (6, 1)
    for flag in ("--both-strands", "--strand-vote"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", "12", flag])
        assert "mode 12" in str(ex.value) and "6 and 7" not in str(ex.value)
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", "7", flag])
        assert "6 and 7" in str(ex.value)
    for m in ("10", "11", "13"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", m])
        assert str(ex.value) == "Alignment mode must be in [0..9], or 12"


def test_gap_local_plan_routes(tmp_path):
    plan_check_build.run_ok("gap_local_plan_check", tmp_path, "gap local plan ok")


def test_the_kernels_keep_their_rows_in_registers():
    """The bar of -m 6 / -m 7: no scratch, no spilled VGPR, no AGPR, at most 200 VGPRs and the score table's 160 B of LDS in every
    instantiation of gap_local/rg_path_gap_local.hip."""
    assert_rows_in_registers("gap_local/rg_path_gap_local.hip", 10, vgprs=200, lds=160)
