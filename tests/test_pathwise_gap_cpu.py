"""CPU: the rule of -m 6 / -m 7 (tests/pathwise_gap_rule.py) against the hand-checked results and a plain scalar Gotoh, the refusals
of rg_batch_create (answered before a device is needed), the plan's routes (tests/c/gap_plan_check.cpp), the CLI's parser and the
registers of the new kernels."""
import numpy as np
import pytest

import plan_check_build

import pathwise_gap_rule as R
from pathwise_support import DIAMOND, TWO_BUBBLES, assert_rows_in_registers, create_rc, no_device


def _graph(gfa):
    from recgraph_amd import api
    return api.Graph.from_gfa_text(gfa)


def _paths(gfa):
    return R.graph_paths(_graph(gfa))


def test_the_rule_reproduces_the_hand_checked_results():
    lnz, rows = _paths(DIAMOND)
    assert R.comments(lnz, rows, "ATG") == "3M, best path: 0, score: 6\tATG"
    lnz, rows = _paths(TWO_BUBBLES)
    # both paths score 4 (one mismatch each): the lowest index wins, where -m 4 picks path 1
    assert R.comments(lnz, rows, "ATGCT") == "3M1X1M, best path: 0, score: 4\tATGAT"
    assert [R.path_rows([lnz[r] for r in pr], "ATGCT", R.default_scores(), -4, -2, False, False)[-1] for pr in rows] == [4, 4]
    # the GG run is paid as ONE gap: 5 matches + o + 2 e = 10 - 8
    score, k, end_row, ops, pseq = R.align(lnz, rows, "ATGGGAT")
    assert (score, k, end_row, ops[::-1], pseq) == (2, 0, rows[0][-1], "DDLLDDD", "ATGAT")
    assert R.cigar_of(ops, pseq, "ATGGGAT") == "2M2D3M"
    # -m 7, read T: every path reaches 2; the smallest row wins: row 2 (the T of path 0)
    score, k, end_row, ops, pseq = R.align(lnz, rows, "T", semi=True)
    assert (score, k, end_row, ops, pseq) == (2, 0, 2, "D", "T") and lnz[2] == "T"
    # the whole lines: -m 6 as the issue states it; -m 7 starts inside the graph (segment 2, the T of path 0)
    ids = R.graph_node_ids(_graph(TWO_BUBBLES))
    assert R.line(lnz, rows, ids, "name", "ATGCT") == "name\t5\t0\t4\t+\t>1>2>4>5>7\t5\t0\t4\t0\t*\t*\t3M1X1M, best path: 0, score: 4\tATGAT\n"
    assert R.line(lnz, rows, ids, "name", "T", semi=True) == "name\t1\t0\t0\t+\t>2\t1\t0\t0\t0\t*\t*\t1M, best path: 0, score: 2\tT\n"


def test_the_row_step_is_gotoh():
    """X through one maximum.accumulate equals the cell-by-cell recurrence (exact because o <= 0), o = 0 and e = 0 included."""
    rng = np.random.default_rng(1)
    for t in range(200):
        b = "".join("ACGTN"[int(x)] for x in rng.integers(0, 5, size=int(rng.integers(1, 14))))
        r = "".join("ACGTN"[int(x)] for x in rng.integers(0, 5, size=int(rng.integers(1, 14))))
        o, e = [(-4, -2), (0, -2), (-6, 0), (-40, -1), (0, 0)][t % 5]
        for semi in (False, True):
            assert R.path_rows(b, r, R.default_scores(), o, e, semi, False) == R.naive_scores(b, r, R.default_scores(), o, e, semi)


def test_linear_gaps_on_one_path_equal_the_oracle_m4(oracle):
    """o = 0 and P = 1: affine gaps of cost e per base are the linear gaps of -m 4 / -m 5 when the matrix's gap entries equal e — and
    the tie rules coincide there, so the rule's WHOLE line (path string, length, start, end: line()) must be the oracle's."""
    from recgraph_amd import api, synth
    g = synth.random_dag_graph(30, 1, seed=5)
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    ids = R.graph_node_ids(gg)
    og = oracle.Graph.from_gfa_text(g.gfa())
    sc = R.default_scores(2, -4)            # gap entries: -8
    rng = np.random.default_rng(2)
    w = g.path_sequence(0)
    reads = (w, w[:20] + w[31:], w[:40] + "ACGTAC" + w[40:], "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=60)), "A",
             w[30:70], w[50:90] + "TT")
    for rd in reads:
        for semi, om in ((False, oracle.M4_ABS), (True, oracle.M5_ABS)):
            text = og.align(om, rd, name="r", idx=1)[0]
            assert R.line(lnz, rows, ids, "r", rd, sc, 0, -8, semi) == text, (semi, rd, text[-120:])


def test_modes_6_and_7_are_supported_and_refuse_before_a_device_is_needed():
    from recgraph_amd import api
    for mode in (api.MODE_PATHWISE_GAP, api.MODE_PATHWISE_GAP_SEMI):
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
        rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25)
        assert rc == -5, (rc, msg)
        rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=-(1 << 25))
        assert rc == -5, (rc, msg)


def test_the_api_refuses_both_strands():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
        with pytest.raises(api._lib.RecGraphError):
            fn(g, ["ATG"], mode=api.MODE_PATHWISE_GAP, both_strands=True)
        with pytest.raises(api._lib.RecGraphError):
            fn(g, ["ATG"], mode=api.MODE_PATHWISE_GAP_SEMI, strand_vote=True)


def test_the_cli_takes_the_modes():
    from recgraph_amd import cli
    for m in ("6", "7"):
        a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", m, "-O", "6", "-E", "1"])
        assert a.alignment_mode == int(m) and (a.gap_open, a.gap_extension) == (6, 1)
    for flag in ("--both-strands", "--strand-vote"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", "6", flag])
        assert "6 and 7" in str(ex.value)


def test_gap_plan_routes(tmp_path):
    plan_check_build.run_ok("gap_plan_check", tmp_path, "gap plan ok")


def test_the_kernels_keep_their_rows_in_registers():
    """No scratch, no spilled VGPRs and no AGPRs (a kernel without MFMA that holds AGPRs has had VGPRs moved there: a spill in all but
    name) in any instantiation: H and Y of a row live in registers (DESIGN 4.8 lists the counts)."""
    # 200 VGPRs: two waves per SIMD at the least, C = 32 included; 160 B of LDS: the score table only, no row was moved to LDS
    assert_rows_in_registers("gap/rg_path_gap.hip", 18, vgprs=200, lds=160)
