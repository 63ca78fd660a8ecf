"""CPU: the rule of -m 6 / -m 7 (tests/pathwise_gap_rule.py) against the hand-checked results and a plain scalar Gotoh, the refusals
of rg_batch_create (answered before a device is needed), the plan's routes (tests/c/gap_plan_check.cpp), the CLI's parser and the
registers of the new kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import plan_check_build

import pathwise_gap_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAMOND = ("H\tVN:Z:1.0\nS\t1\tA\nS\t2\tT\nS\t3\tC\nS\t4\tG\nL\t1\t+\t2\t+\t0M\nL\t1\t+\t3\t+\t0M\nL\t2\t+\t4\t+\t0M\n"
           "L\t3\t+\t4\t+\t0M\nP\tp0\t1+,2+,4+\t*\nP\tp1\t1+,3+,4+\t*\n")
TWO_BUBBLES = ("S\t1\tA\nS\t2\tT\nS\t3\tC\nS\t4\tG\nS\t5\tA\nS\t6\tC\nS\t7\tT\n" +
               "".join(f"L\t{a}\t+\t{b}\t+\t0M\n" for a, b in [(1, 2), (1, 3), (2, 4), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)]) +
               "P\tp0\t1+,2+,4+,5+,7+\t*\nP\tp1\t1+,3+,4+,6+,7+\t*\n")


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


def _create(gfa, reads, mode, o=-4, e=-2, amb=0, match=2):
    from recgraph_amd import api
    lib = api._lib.load()
    g = api.Graph.from_gfa_text(gfa)
    p = api.make_params(mode, o=o, e=e, amb=amb)
    p.scores[0] = match
    blob = "".join(reads).encode()
    off = (C.c_int64 * (len(reads) + 1))(*np.concatenate([[0], np.cumsum([len(r) for r in reads])]).tolist())
    out = C.c_void_p()
    rc = lib.rg_batch_create(g._h, C.byref(p), blob, off, len(reads), C.byref(out))
    if rc == 0:
        lib.rg_batch_destroy(out)
    return rc, lib.rg_last_error().decode()


def _no_device():
    from recgraph_amd import api
    return api._lib.load().rg_device_count() == 0


def test_modes_6_and_7_are_supported_and_refuse_before_a_device_is_needed():
    from recgraph_amd import api
    for mode in (api.MODE_PATHWISE_GAP, api.MODE_PATHWISE_GAP_SEMI):
        rc, msg = _create(TWO_BUBBLES, ["ATGCT"], mode)
        # (on the parent commit: RG_ERR_ARG "unsupported mode")
        assert rc == (-3 if _no_device() else 0), (rc, msg)
        assert _create(TWO_BUBBLES, ["ATGCT"], mode, o=1)[0] == -1
        assert _create(TWO_BUBBLES, ["ATGCT"], mode, e=1)[0] == -1
        for amb in (1, 2, 4, 8, 12):
            assert _create(TWO_BUBBLES, ["ATGCT"], mode, amb=amb)[0] == -1, amb
        rc, msg = _create(TWO_BUBBLES, ["A" * 2048], mode)
        assert rc == -1 and "2047" in msg, (rc, msg)
        assert _create(TWO_BUBBLES, ["A" * 2047], mode)[0] == (-3 if _no_device() else 0)
        # (5 rows + 5 bases) * 2^25 >= 2^28
        rc, msg = _create(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25)
        assert rc == -5, (rc, msg)
        rc, msg = _create(TWO_BUBBLES, ["ATGCT"], mode, o=-(1 << 25))
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
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.report("gap/rg_path_gap.hip")
    assert len(ks) == 18
    for k in ks:
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0 and k["AGPRs"] == 0, (k["name"], k)
        assert k["VGPRs"] <= 200, (k["name"], k)         # (two waves per SIMD at the least, C = 32 included)
        assert k["LDS Size [bytes/block]"] <= 160, (k["name"], k)      # the score table only: no row was moved to LDS
