"""CPU: the both-strands affine-gap pathwise modes for reads of up to 131071 bases (-m 76 / -m 77 / -m 82 = modes 6 / 7 / 12,
`mode + 70`): the defines, admission and refusals of rg_batch_create (answered before a device is needed), the plans of the stages
(tests/c/gap_xstrands_plan_check.cpp), the API and CLI surface, the registers of the new kernels, and the composed rule of
tests/pathwise_gap_xstrands_rule.py on hand cases."""
import inspect
import os

import pytest

import plan_check_build

import pathwise_gap_rule as R
import pathwise_gap_xstrands_rule as X
import strand_vote_rule as V
from pathwise_support import TWO_BUBBLES, assert_rows_in_registers, create_rc, kernel_resources, no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XSTRANDS = {76: 6, 77: 7, 82: 12}
KERNELS = ["rg::k_gap_pick_out", "rg::k_gap_seed_pick", "rg::k_gap_xstrands_duel", "rg::k_gap_xstrands_mark"]
LENGTHS = (5, 30000, 131072)


@pytest.mark.parametrize("mode", sorted(XSTRANDS))
def test_the_modes_are_admitted_before_a_device_is_needed(mode):
    """The test that fails without the feature: on the parent commit rg_batch_create answers RG_ERR_ARG "unsupported mode"."""
    ok = -3 if no_device() else 0
    rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode)
    assert rc == ok, (rc, msg)
    for n in (2047, 2048, 16383, 16384, 30000, 131071):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * n], mode)
        assert rc == ok, (n, rc, msg)
    for amb in (0, 4) + ((12,) if mode != 82 else ()):
        for n in (5, 30000):
            rc, msg = create_rc(TWO_BUBBLES, ["A" * n], mode, amb=amb)
            assert rc == ok, (amb, n, rc, msg)


@pytest.mark.parametrize("mode", sorted(XSTRANDS))
def test_every_refusal_at_every_length(mode):
    """amb_mode bits 0 and 1, bit 3 alone, any higher bit, positive gap costs, a read over 131071 bases: RG_ERR_ARG at 5, 30000 and
    131072 bases alike (the last is refused for its length whatever else is asked)."""
    for n in LENGTHS:
        reads = ["ATG", "A" * n]
        for amb in (1, 2, 3, 5, 6, 8, 9, 13, 16, 20, 28, 32, 36, 44):
            assert create_rc(TWO_BUBBLES, reads, mode, amb=amb)[0] == -1, (n, amb)
        assert create_rc(TWO_BUBBLES, reads, mode, o=1)[0] == -1, n
        assert create_rc(TWO_BUBBLES, reads, mode, e=1)[0] == -1, n
        assert create_rc(TWO_BUBBLES, reads, mode, o=1, amb=4)[0] == -1, n
        rc, msg = create_rc(TWO_BUBBLES, reads, mode, amb=12)
        if mode == 82:
            # mode 32's message and reason
            assert rc == -1 and (n == 131072 or ("hopeless" in msg and "82" in msg)), (n, rc, msg)
        elif n == 131072:
            assert rc == -1
    for amb in (0, 4):
        rc, msg = create_rc(TWO_BUBBLES, ["ATG", "A" * 131072], mode, amb=amb)
        assert rc == -1 and "131071" in msg, (rc, msg)


@pytest.mark.parametrize("mode", sorted(XSTRANDS))
def test_both_capacity_edges(mode):
    """(5 rows + 5 bases) * 2^25 >= 2^28, and (5 rows + 131067 bases) * 2^11 = 2^28: RG_ERR_CAPACITY; one base fewer is admitted."""
    ok = -3 if no_device() else 0
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25)[0] == -5
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=-(1 << 25))[0] == -5
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25, amb=4)[0] == -5
    assert create_rc(TWO_BUBBLES, ["A" * 131067], mode, match=1 << 11)[0] == -5
    assert create_rc(TWO_BUBBLES, ["A" * 131066], mode, match=1 << 11)[0] == ok


def test_the_neighbours_stay_unsupported_and_the_siblings_keep_their_rules():
    for other in (78, 79, 80, 81, 83, 86, 92, 70, 71, 73, 74, 75, 84, 85, 87, 96, 97, 102):
        for amb in (0, 4):
            rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], other, amb=amb)
            assert rc == -1 and "unsupported mode" in msg, (other, rc, msg)
    for other in (36, 37, 42, 46, 47, 52, 66, 67, 72):
        rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], other)
        assert rc == -1 and "unsupported mode" in msg, (other, rc, msg)
    # modes 56 / 57 / 62 keep refusing every amb_mode bit, modes 26 / 27 / 32 keep their 16383 limit
    for mode in (56, 57, 62):
        for amb in (1, 2, 4, 8, 12):
            for rd in ("ATGCT", "A" * 30000):
                rc, msg = create_rc(TWO_BUBBLES, [rd], mode, amb=amb)
                assert rc == -1 and (amb & 3 or amb == 8 or "as given" in msg), (mode, amb, rc, msg)
    for mode in (26, 27, 32):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * 16384], mode)
        assert rc == -1 and "16383" in msg, (mode, rc, msg)


def test_no_new_entry_point():
    from recgraph_amd import _lib
    assert len(_lib.SYMBOLS) == 63
    exports = open(os.path.join(ROOT, "recgraph_amd", "csrc", "exports.map")).read()
    for word in ("xstrands", "strand", "duel", "pick", "stage"):
        assert word not in exports, word
    assert not [s for s in _lib.SYMBOLS if "xstrands" in s or "stage" in s]


def test_the_api_surface():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for fn in (api.pathwise_alignment_gap_exec, api.pathwise_alignment_gap_semi_exec, api.pathwise_alignment_gap_local_exec):
        par = inspect.signature(fn).parameters
        assert par["very_long_both_strands"].default is False
        assert par["very_long_reads"].default is False and par["long_reads"].default is False and par["both_strands"].default is False
        # the existing refusal stays, and names very_long_reads
        with pytest.raises(api._lib.RecGraphError) as ex:
            fn(list("$ATG"), g, very_long_reads=True, both_strands=True)
        assert "very_long_reads" in str(ex.value)
    assert inspect.signature(api._gap_exec_mode).parameters["very_long_both_strands"].default is False
    assert [api._gap_exec_mode(m, False, False, False, True) for m in (6, 7, 12)] == [76, 77, 82]
    assert [api._gap_exec_mode(m, False, False, very_long_both_strands=True) for m in (6, 7, 12)] == [76, 77, 82]
    assert [api._gap_exec_mode(m, False, False, True) for m in (6, 7, 12)] == [56, 57, 62]
    assert [api._gap_exec_mode(m, False, True) for m in (6, 7, 12)] == [26, 27, 32]
    assert [api._gap_exec_mode(m, True, False) for m in (6, 7, 12)] == [16, 17, 22]
    assert [api._gap_exec_mode(m, False, False) for m in (6, 7, 12)] == [6, 7, 12]
    with pytest.raises(api._lib.RecGraphError):
        api._gap_exec_mode(6, True, True, True)
    # both_strands is redundant in the new modes, and the vote is bit 3 in modes 76 and 77 only
    for mode in (76, 77, 82):
        assert api._both_strands_kw(mode, False, {}) == {}
        assert api._both_strands_kw(mode, True, {}) == {"amb": 4}
    for mode in (76, 77):
        assert api._both_strands_kw(mode, False, {"o": -3}, True) == {"o": -3, "amb": 12}
    with pytest.raises(api._lib.RecGraphError) as ex:
        api._both_strands_kw(82, False, {}, True)
    assert "hopeless" in str(ex.value) and "82" in str(ex.value)
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
        with pytest.raises(api._lib.RecGraphError) as ex:
            fn(g, ["ATG"], mode=82, strand_vote=True)
        assert "hopeless" in str(ex.value)
        # modes 56 / 57 / 62 keep raising
        for mode in (56, 57, 62):
            with pytest.raises(api._lib.RecGraphError) as ex:
                fn(g, ["ATG"], mode=mode, both_strands=True)
            assert "56, 57, 62" in str(ex.value)


def test_the_cli_takes_the_modes():
    from recgraph_amd import api, cli
    for m in sorted(XSTRANDS):
        for flags in [[], ["--both-strands"]] + ([["--strand-vote"]] if m != 82 else []):
            a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", str(m), "-O", "6", "-E", "1"] + flags)
            assert a.alignment_mode == m and (a.gap_open, a.gap_extension) == (6, 1)
            # accepted: main gets as far as the graph file, which is not there
            with pytest.raises((OSError, api._lib.RecGraphError)):
                cli.main(["no-such-reads.fa", "no-such-graph.gfa", "-m", str(m)] + flags)
    with pytest.raises(SystemExit) as ex:
        cli.main(["reads.fa", "graph.gfa", "-m", "82", "--strand-vote"])
    assert "mode 82" in str(ex.value) and "hopeless" in str(ex.value)
    for m in ("78", "79", "80", "81", "83", "86", "92", "66", "72"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", m])
        assert str(ex.value) == "Alignment mode must be in [0..9], or 12"
    for m in ("56", "57", "62"):
        with pytest.raises(SystemExit):
            cli.main(["reads.fa", "graph.gfa", "-m", m, "--both-strands"])


def test_gap_xstrands_plan_routes(tmp_path):
    plan_check_build.run_ok("gap_xstrands_plan_check", tmp_path, "gap xstrands plan ok")


def test_the_new_kernels_are_small():
    """They run beside other handles' Gotoh waves: no scratch, no spill, no AGPR, no LDS, at most 48 VGPRs, and no store whose source
    register is overwritten too early.  The directory holds the two files and nothing else; no inline assembly, no atomics."""
    d = os.path.join(ROOT, "recgraph_amd", "csrc", "gap_xstrands")
    assert sorted(os.listdir(d)) == ["rg_gap_xstrands.hip", "rg_gap_xstrands.hpp"]
    ks = assert_rows_in_registers("gap_xstrands/rg_gap_xstrands.hip", len(KERNELS), vgprs=48, lds=0)
    assert sorted(k["name"].split("(")[0] for k in ks) == KERNELS, ks
    assert all(k["SGPRs Spill"] == 0 for k in ks), [(k["name"], k["SGPRs Spill"]) for k in ks]
    hits, stores = kernel_resources().store_hazards("gap_xstrands/rg_gap_xstrands.hip")
    assert not hits and stores >= 4, hits[:4]
    src = open(os.path.join(d, "rg_gap_xstrands.hip")).read()
    assert "asm" not in src and "atomic" not in src.replace("no atomics", "")


def test_the_kernel_directories_of_the_family_kept_their_kernels():
    """The stages are driver code and four new kernels of their own: no `__global__` was added to the directories whose kernel sets
    the matrices pin."""
    csrc = os.path.join(ROOT, "recgraph_amd", "csrc")
    for d, n in (("gap", 1), ("gap_local", 1), ("gap_long", 1), ("gap_strands", 1), ("gap_xlong", 1), ("gap_xstrands", 1)):
        assert len([f for f in os.listdir(os.path.join(csrc, d)) if f.endswith(".hip")]) == n, d
    for f in ("rg_path_driver.hip", "rg_strand_driver.hip", "rg_abi.hip", "rg_stream.hip"):
        assert "__global__" not in open(os.path.join(csrc, f)).read(), f


# ---- the composed rule, without a device ----

def _fake(table):
    """A pick as a lookup: sequence -> score (None: an unaligned local pick)."""
    return lambda seq: table[seq]


def test_the_composition_on_hand_cases():
    rd, rv = "AACCG", "CGGTT"
    assert V.rc(rd) == rv
    # exact rule, modes 76 / 77: the reverse pick runs only below 0, and wins only when strictly greater
    for mode in (76, 77):
        assert X.decide(mode, rd, _fake({rd: 0, rv: 50})) == ("+", ["+"], 0)
        assert X.decide(mode, rd, _fake({rd: -2, rv: 50})) == ("-", ["+", "-"], 50)
        for other in (-2, -7):
            assert X.decide(mode, rd, _fake({rd: -2, rv: other})) == ("+", ["+", "-"], -2)
    # mode 82: every read goes both ways; an unaligned pick scores 0
    assert X.decide(82, rd, _fake({rd: None, rv: 12})) == ("-", ["+", "-"], 12)
    assert X.decide(82, rd, _fake({rd: None, rv: None})) == ("+", ["+", "-"], None)
    assert X.decide(82, rd, _fake({rd: 12, rv: 12})) == ("+", ["+", "-"], 12)
    assert X.decide(82, rd, _fake({rd: 12, rv: None})) == ("+", ["+", "-"], 12)
    assert X.decide(82, rd, _fake({rd: 12, rv: 13})) == ("-", ["+", "-"], 13)
    pal = "ACGTACGT"
    assert V.rc(pal) == pal and X.decide(82, pal, _fake({pal: 8})) == ("+", ["+", "-"], 8)
    # vote rule: a read that goes reverse first and scores >= 0 there never has its forward strand looked at
    path = "ACGGTCATTGCAGGCTTAACCGATCGGATTACCA"
    kmers = V.kmer_set([path])
    fwd_read, rev_read = path[2:30], V.rc(path[2:30])
    assert V.first_reverse(kmers, rev_read) and not V.first_reverse(kmers, fwd_read)
    assert X.decide(76, rev_read, _fake({rev_read: 40, fwd_read: 3}), kmers) == ("-", ["-"], 3)       # (the exact rule keeps forward, 40)
    assert X.decide(76, rev_read, _fake({rev_read: 40, fwd_read: 3})) == ("+", ["+"], 40)
    assert X.decide(77, rev_read, _fake({rev_read: -1, fwd_read: -1}), kmers) == ("+", ["-", "+"], -1)   # a tie keeps forward, whichever went first
    assert X.decide(77, rev_read, _fake({rev_read: -9, fwd_read: -1}), kmers) == ("-", ["-", "+"], -1)
    assert X.decide(77, rev_read, _fake({rev_read: -1, fwd_read: -9}), kmers) == ("+", ["-", "+"], -1)
    assert X.decide(76, "ACGTACG", _fake({"ACGTACG": -5, "CGTACGT": -3}), kmers) == ("-", ["+", "-"], -3)     # under 12 bases: votes 0 / 0
    with pytest.raises(AssertionError):
        X.decide(82, rd, _fake({}), kmers)


def test_the_rule_on_the_hand_graph():
    """TWO_BUBBLES: whole reads, counters included.  A read given on the wrong strand is reported as its reverse complement's line
    of mode m + 50 with column 5 set to '-'; the counted cells are rows x n per path and picked strand; the performed cells add the
    traceback of the winning strand alone."""
    from recgraph_amd import api
    gg = api.Graph.from_gfa_text(TWO_BUBBLES)
    lnz, rows = R.graph_paths(gg)
    node_ids = R.graph_node_ids(gg)
    total = sum(len(r) for r in rows)
    w = "".join(lnz[r] for r in rows[0])
    for mode in (76, 77):
        semi = mode == 77
        fwd = X.expected(mode, w, lnz, rows, node_ids, "q")
        assert (fwd["strand"], fwd["picked"], fwd["status"]) == ("+", ["+"], 0) and fwd["score"] == 2 * len(w)
        assert fwd["text"] == R.line(lnz, rows, node_ids, "q", w, None, -4, -2, semi)
        assert fwd["cells"] == total * len(w) and fwd["performed"] == fwd["cells"] + len(rows[0]) * len(w)
        rev = X.expected(mode, V.rc(w), lnz, rows, node_ids, "q")
        if R.align(lnz, rows, V.rc(w), semi=semi)[0] < 0:
            assert (rev["strand"], rev["picked"]) == ("-", ["+", "-"]) and rev["text"] == V.minus(fwd["text"]) and rev["score"] == fwd["score"]
            assert rev["cells"] == 2 * fwd["cells"] and rev["performed"] == rev["cells"] + len(rows[0]) * len(w)
        else:
            assert (rev["strand"], rev["picked"]) == ("+", ["+"])
    loc = X.expected(82, V.rc(w), lnz, rows, node_ids, "q")
    assert (loc["strand"], loc["picked"], loc["score"]) == ("-", ["+", "-"], 2 * len(w)) and loc["text"].split("\t")[4] == "-"
    none = X.expected(82, "NNNN", lnz, rows, node_ids, "q")
    assert (none["text"], none["status"], none["strand"], none["picked"]) == ("", X.READ_UNALIGNED, " ", ["+", "-"])
    assert none["cells"] == none["performed"] == 2 * total * 4
    bad = X.expected(82, "AC?T", lnz, rows, node_ids, "q")
    assert (bad["status"], bad["picked"], bad["cells"]) == (X.READ_BAD_BASE, [], 0)
    # striped: the same read in a batch whose longest read is over 2047 bases is traced by the checkpointed kernels: the checkpoint
    # pass and one rebuilt stripe
    st = X.expected(76, w, lnz, rows, node_ids, "q", striped=True)
    assert st["performed"] == st["cells"] + 2 * len(rows[0]) * len(w) and st["text"] == X.expected(76, w, lnz, rows, node_ids, "q")["text"]
