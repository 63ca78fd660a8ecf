"""CPU: the both-strands flavours of the affine-gap pathwise modes (-m 26 / -m 27 / -m 32 = modes 6 / 7 / 12 + 20): the defines,
admission and refusals of rg_batch_create (answered before a device is needed), the plan of the two passes
(tests/c/gap_strands_plan_check.cpp), the API and CLI surface, the registers of the new gate kernel, and the composed rule of
tests/pathwise_gap_strands_rule.py on hand cases and in the score regimes the GPU tests use."""
import functools
import inspect
import os

import pytest

import plan_check_build

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
import pathwise_gap_strands_rule as S
import strand_vote_rule as V
from pathwise_support import TWO_BUBBLES, assert_rows_in_registers, create_rc, kernel_resources, no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRANDS = {26: 6, 27: 7, 32: 12}


@pytest.mark.parametrize("mode", sorted(STRANDS))
def test_the_modes_are_admitted_and_refuse_before_a_device_is_needed(mode):
    ok = -3 if no_device() else 0
    rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode)
    # (on the parent commit: RG_ERR_ARG "unsupported mode")
    assert rc == ok, (rc, msg)
    for n in (2047, 2048, 16383):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * n], mode)
        assert rc == ok, (n, rc, msg)
    rc, msg = create_rc(TWO_BUBBLES, ["ATG", "A" * 16384], mode)
    assert rc == -1 and "16383" in msg, (rc, msg)
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=1)[0] == -1
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, e=1)[0] == -1
    assert create_rc(TWO_BUBBLES, ["A" * 5000], mode, o=1, amb=4)[0] == -1
    # the two capacity cases of the long modes: (5 rows + 5 bases) * 2^25 >= 2^28, and (5 rows + 16379 bases) * 2^14 = 2^28
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25)[0] == -5
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=-(1 << 25))[0] == -5
    assert create_rc(TWO_BUBBLES, ["A" * 16379], mode, match=1 << 14)[0] == -5
    assert create_rc(TWO_BUBBLES, ["A" * 16378], mode, match=1 << 14)[0] == ok


@pytest.mark.parametrize("mode", sorted(STRANDS))
def test_amb_mode_admission(mode):
    ok = -3 if no_device() else 0
    for amb in (0, 4):
        for rd in ("ATGCT", "A" * 3000):
            rc, msg = create_rc(TWO_BUBBLES, [rd], mode, amb=amb)
            assert rc == ok, (amb, rc, msg)
    rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode, amb=12)
    if mode == 32:
        # the message says why: a vote needs a score that says "hopeless"
        assert rc == -1 and "hopeless" in msg and "32" in msg, (rc, msg)
    else:
        assert rc == ok, (rc, msg)
    for amb in (1, 2, 8, 16, 3, 5, 13, 20, 28):
        assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, amb=amb)[0] == -1, amb
        assert create_rc(TWO_BUBBLES, ["A" * 3000], mode, amb=amb)[0] == -1, amb


def test_the_gaps_between_the_modes_stay_closed_and_the_other_modes_keep_refusing():
    for other in (24, 25, 28, 29, 30, 31, 33, 34, 36, 42, 46):
        rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], other)
        assert rc == -1 and "unsupported mode" in msg, (other, rc, msg)
    for mode in (6, 7, 12, 16, 17, 22):
        for amb in (4, 12):
            rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode, amb=amb)
            assert rc == -1 and "as given" in msg, (mode, amb, rc, msg)


def test_no_new_entry_point():
    from recgraph_amd import _lib
    assert len(_lib.SYMBOLS) == 63
    exports = open(os.path.join(ROOT, "recgraph_amd", "csrc", "exports.map")).read()
    assert "strand" not in exports and "long" not in exports and "gate" not in exports


def test_the_api_surface():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for fn in (api.pathwise_alignment_gap_exec, api.pathwise_alignment_gap_semi_exec, api.pathwise_alignment_gap_local_exec):
        assert inspect.signature(fn).parameters["both_strands"].default is False
        assert inspect.signature(fn).parameters["long_reads"].default is False
    assert [api._gap_exec_mode(m, False, True) for m in (6, 7, 12)] == [26, 27, 32]
    assert [api._gap_exec_mode(m, True, True) for m in (6, 7, 12)] == [26, 27, 32]
    assert [api._gap_exec_mode(m, True, False) for m in (6, 7, 12)] == [16, 17, 22]
    assert [api._gap_exec_mode(m, False, False) for m in (6, 7, 12)] == [6, 7, 12]
    # in the new modes both_strands is redundant, and the vote is bit 3 in modes 26 and 27 only
    for mode in (26, 27, 32):
        assert api._both_strands_kw(mode, False, {}) == {}
        assert api._both_strands_kw(mode, True, {}) == {"amb": 4}
    for mode in (26, 27):
        assert api._both_strands_kw(mode, False, {"o": -3}, True) == {"o": -3, "amb": 12}
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
        with pytest.raises(api._lib.RecGraphError) as ex:
            fn(g, ["ATG"], mode=32, strand_vote=True)
        assert "hopeless" in str(ex.value)
        # mode = 6, both_strands = True and its kin keep raising
        for mode in (6, 7, 12, 16, 17, 22):
            with pytest.raises(api._lib.RecGraphError):
                fn(g, ["ATG"], mode=mode, both_strands=True)
            with pytest.raises(api._lib.RecGraphError):
                fn(g, ["ATG"], mode=mode, strand_vote=True)


def test_the_cli_takes_the_modes():
    from recgraph_amd import cli
    for m in sorted(STRANDS):
        for flags in [[], ["--both-strands"]] + ([["--strand-vote"]] if m != 32 else []):
            a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", str(m), "-O", "6", "-E", "1"] + flags)
            assert a.alignment_mode == m and (a.gap_open, a.gap_extension) == (6, 1)
            # accepted: main gets as far as the graph file, which is not there
            with pytest.raises(Exception) as ex:
                cli.main(["no-such-reads.fa", "no-such-graph.gfa", "-m", str(m)] + flags)
            assert not isinstance(ex.value, SystemExit), (m, flags, ex.value)
    with pytest.raises(SystemExit) as ex:
        cli.main(["reads.fa", "graph.gfa", "-m", "32", "--strand-vote"])
    assert "mode 32" in str(ex.value) and "hopeless" in str(ex.value)
    for m in ("24", "25", "28", "29", "30", "31", "33", "34"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", m])
        assert str(ex.value).startswith("Alignment mode must be in")
    for m in ("6", "7", "12", "16", "17", "22"):
        with pytest.raises(SystemExit):
            cli.main(["reads.fa", "graph.gfa", "-m", m, "--both-strands"])


def test_gap_strands_plan_routes(tmp_path):
    plan_check_build.run_ok("gap_strands_plan_check", tmp_path, "gap strands plan ok")


def test_the_gate_kernel_is_small():
    """Like the three kernels of rg_strand.hip it runs beside other handles' Gotoh waves: at most 64 VGPRs, no scratch, no spill, no
    AGPR, and no store whose source register is overwritten too early.  It is the only kernel of its directory."""
    d = os.path.join(ROOT, "recgraph_amd", "csrc", "gap_strands")
    assert sorted(os.listdir(d)) == ["rg_gap_strands.hip", "rg_gap_strands.hpp"]
    ks = assert_rows_in_registers("gap_strands/rg_gap_strands.hip", 1, vgprs=64)
    assert {k["name"].split("(")[0] for k in ks} == {"rg::k_gap_strands_gate"}, ks
    hits, stores = kernel_resources().store_hazards("gap_strands/rg_gap_strands.hip")
    assert not hits, hits[:4]


# ---- the composed rule, without a device ----

def _fake(table):
    """A pass as a lookup: read text -> line (the line's other columns do not matter to the composition)."""
    def line_of(rd):
        sc = table[rd]
        return "" if sc is None else "q\t%d\t0\t%d\t+\t>1\t9\t0\t8\t0\t*\t*\t1M, best path: 0, score: %d\t%s\n" % (len(rd), len(rd) - 1, sc, rd)
    return line_of


def test_the_composition_on_hand_cases():
    rd, rv = "AACCG", "CGGTT"
    assert V.rc(rd) == rv
    # exact rule, modes 26 / 27: the reverse pass runs only below 0, and wins only when strictly greater
    for mode in (26, 27):
        t, st, strand, passes = S.expected(mode, rd, _fake({rd: 0, rv: 50}))
        assert (st, strand, passes) == (0, "+", ["+"]) and "score: 0" in t
        t, st, strand, passes = S.expected(mode, rd, _fake({rd: -2, rv: 50}))
        assert (st, strand, passes) == (0, "-", ["+", "-"]) and t.split("\t")[4] == "-" and "score: 50" in t and t.endswith(rv + "\n")
        for other in (-2, -7):
            t, st, strand, passes = S.expected(mode, rd, _fake({rd: -2, rv: other}))
            assert (st, strand, passes) == (0, "+", ["+", "-"]) and "score: -2" in t
        assert S.expected(mode, "AAC?G", _fake({})) == ("", S.READ_BAD_BASE, " ", [])
        assert S.expected(mode, "aac-g", _fake({"AACNG": 3}))[2:] == ("+", ["+"])           # canonicalised like every read
    # mode 32: every read with a record goes both ways; score 0 is "unaligned"
    t, st, strand, passes = S.expected(32, rd, _fake({rd: None, rv: 12}))
    assert (st, strand, passes) == (0, "-", ["+", "-"]) and "score: 12" in t
    assert S.expected(32, rd, _fake({rd: None, rv: None})) == ("", S.READ_UNALIGNED, " ", ["+", "-"])
    t, st, strand, passes = S.expected(32, rd, _fake({rd: 12, rv: 12}))
    assert (st, strand, passes) == (0, "+", ["+", "-"])
    t, st, strand, passes = S.expected(32, rd, _fake({rd: 12, rv: None}))
    assert (st, strand) == (0, "+")
    pal = "ACGTACGT"
    assert V.rc(pal) == pal and S.expected(32, pal, _fake({pal: 8}))[1:3] == (0, "+")
    assert S.expected(32, "AAC?G", _fake({})) == ("", S.READ_BAD_BASE, " ", [])
    # vote rule: a read that goes reverse first and scores >= 0 there never has its forward strand looked at
    path = "ACGGTCATTGCAGGCTTAACCGATCGGATTACCA"
    kmers = V.kmer_set([path])
    fwd_read, rev_read = path[2:30], V.rc(path[2:30])
    assert V.votes(kmers, fwd_read)[0] > 0 and V.first_reverse(kmers, rev_read) and not V.first_reverse(kmers, fwd_read)
    t, st, strand, passes = S.expected(26, rev_read, _fake({rev_read: 40, V.rc(rev_read): 3}), kmers)
    assert (strand, passes) == ("-", ["-"]) and "score: 3" in t                   # (the exact rule would have kept forward, 40)
    assert S.expected(26, rev_read, _fake({rev_read: 40, V.rc(rev_read): 3}))[2:] == ("+", ["+"])
    t, st, strand, passes = S.expected(27, rev_read, _fake({rev_read: -1, V.rc(rev_read): -1}), kmers)
    assert (strand, passes) == ("+", ["-", "+"])                                     # a tie keeps forward, whichever went first
    t, st, strand, passes = S.expected(27, rev_read, _fake({rev_read: -9, V.rc(rev_read): -1}), kmers)
    assert (strand, passes) == ("-", ["-", "+"])
    assert S.expected(26, "ACGTACG", _fake({"ACGTACG": -5, "CGTACGT": -3}), kmers)[2:] == ("-", ["+", "-"])     # under 12 bases: votes 0 / 0, forward first
    with pytest.raises(AssertionError):
        S.expected(32, rd, _fake({}), kmers)


@functools.lru_cache(maxsize=None)
def _graph400():
    from recgraph_amd import api, synth
    g = synth.haplotype_graph(400 * 13 // 10, 2, path_len=400, seed=71)
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    return g, lnz, rows, R.graph_node_ids(gg)


def test_the_score_regimes_the_gpu_tests_rely_on():
    """On a two-path graph of about 400 rows with the default scores: whole-path and 40- to 300-base reads given on the wrong strand
    score well below 0 forward in modes 6 and 7 (so the exact rule's gate fires) and above 0 on their own strand; 12- to 20-base
    semiglobal reads can score ABOVE 0 on the wrong strand (so the gate does not fire although the other strand is better); local
    wrong-strand scores are small against the right strand's."""
    g, lnz, rows, node_ids = _graph400()
    w = g.path_sequence(0)
    for semi in (False, True):
        for piece in (w, w[100:140], w[50:350]):
            wrong = R.align(lnz, rows, V.rc(piece), semi=semi)[0]
            right = R.align(lnz, rows, piece, semi=semi)[0]
            assert wrong < -10 and (right > 0 or not semi), (semi, len(piece), wrong, right)
            line_of = S.line_fn(27 if semi else 26, lnz, rows, node_ids, "q")
            t, st, strand, passes = S.expected(27 if semi else 26, V.rc(piece), line_of)
            if semi or piece is w:
                assert (st, strand, passes) == (0, "-", ["+", "-"]) and t == V.minus(line_of(piece))
    seen = 0
    for q in range(0, 300, 7):
        for n in (12, 16, 20):
            rd = V.rc(w[q:q + n])
            f, r = R.align(lnz, rows, rd, semi=True)[0], R.align(lnz, rows, w[q:q + n], semi=True)[0]
            assert r == 2 * n
            if f >= 0:
                seen += 1
                assert 0 <= f < r
                assert S.expected(27, rd, S.line_fn(27, lnz, rows, node_ids, "q"))[2:] == ("+", ["+"])
    assert seen >= 1
    for piece in (w[100:140], w[50:185]):
        wrong, right = L.align_local(lnz, rows, V.rc(piece))[0], L.align_local(lnz, rows, piece)[0]
        assert 0 < wrong <= 30 and right == 2 * len(piece), (wrong, right)
        assert S.expected(32, V.rc(piece), S.line_fn(32, lnz, rows, node_ids, "q"))[1:] == (0, "-", ["+", "-"])
