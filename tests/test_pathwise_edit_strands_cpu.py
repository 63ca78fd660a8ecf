"""CPU: the both-strands edit-distance pathwise modes (-m 64 / -m 65 = modes 26 / 27 at unit costs, both strands scored in one wave):
the cross-lane bit arithmetic of the half-wave row step on the host (tests/c/edit_pair_bits_check.cpp, plain and under AddressSanitizer +
UBSan), "both strands of every read, strictly greater" against the `< 0` gate of modes 26 / 27, the constants on every side, admission
and refusals of rg_batch_create (answered before a device is needed), the plan (tests/c/edit_strands_plan_check.cpp), the API's and the
CLI's flag rules and the registers of the new kernels."""
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest

import pathwise_edit_strands_rule as ES
import pathwise_gap_rule as R
import pathwise_gap_strands_rule as S
import plan_check_build
import strand_vote_rule as V
from edit_strands_support import MODES, run_host_program
from pathwise_support import PALINDROME, TWO_BUBBLES, assert_rows_in_registers, create_rc, graph_tuple, no_device, rand_bases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = "-M 0 -X 1 -O 0 -E 1"

# (return code, message) of rg_batch_create on TWO_BUBBLES at unit costs, each of them a keyword
_create = functools.partial(create_rc, TWO_BUBBLES, match=0, mismatch=-1, o=0, e=-1)


# ---- 1. bits ----

@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_the_half_wave_row_step_on_the_host(tmp_path, sanitize):
    run_host_program("edit_pair_bits_check", tmp_path, "edit pair bits ok", sanitize=sanitize)


# ---- 2. rule ----

_N_MATCHES_N = R.default_scores(0, -1)
_N_MATCHES_N[4 * 6 + 4] = 0


def _small_graph(seed, alphabet):
    """A few shared segments with two-allele bubbles over `alphabet`, 3 paths, at most 60 rows."""
    from recgraph_amd import synth
    rng = np.random.default_rng(seed)
    segments, links, paths = [], set(), [[], [], []]

    def add(k):
        segments.append((len(segments) + 1, rand_bases(rng, k, alphabet)))
        return len(segments)
    for b in range(4):
        s = add(int(rng.integers(2, 9)))
        for p in paths:
            if p:
                links.add((p[-1], s))
            p.append(s)
        if b == 3:
            break
        alleles = [add(int(rng.integers(1, 6))) for _ in range(2)]
        for k, p in enumerate(paths):
            a = alleles[(k + b) % 2]
            links.add((s, a))
            p.append(a)
    return graph_tuple(synth.SynthGraph(segments, sorted(links), paths))


@pytest.mark.parametrize("mode", MODES)
def test_every_read_on_both_strands_is_the_gate_of_modes_26_and_27_at_unit_costs(mode):
    """Text, status and strand of "both strands of every read, reverse only if strictly greater" equal the exact rule's of mode 26 / 27
    at unit costs and at a table in which N matches N, on random small graphs: path pieces on either strand (forward score 0: the gate
    of mode 26 / 27 stays shut), noisy ones, random reads, reverse palindromes, reads with N and reads with a bad base."""
    seen = {"+": 0, "-": 0, "zero": 0, "bad": 0, "gate shut": 0, "tie": 0}
    for seed, alphabet in ((1, "ACGT"), (2, "ACGTN"), (3, "AC"), (4, "ACGT")):
        g, gg, lnz, rows, node_ids = _small_graph(10 * mode + seed, alphabet)
        rng = np.random.default_rng(seed + mode)
        w = [g.path_sequence(k) for k in range(3)]
        reads = [w[0], V.rc(w[1]), w[2][3:15], V.rc(w[2][2:12]), PALINDROME[:8], "ACGT", "AT", "N" * 5, "NAN", "AC?GT", w[1][:6] + "x"]
        for _ in range(14):
            k, n = int(rng.integers(0, 3)), int(rng.integers(1, 20))
            q = int(rng.integers(0, max(1, len(w[k]) - n)))
            piece = list(w[k][q:q + n])
            for t in range(len(piece)):
                if rng.random() < 0.15:
                    piece[t] = alphabet[int(rng.integers(0, len(alphabet)))]
            piece = "".join(piece)
            reads += [piece, V.rc(piece), rand_bases(rng, n, alphabet)]
        for table in (R.default_scores(0, -1), _N_MATCHES_N):
            for i, rd in enumerate(reads):
                line_of = S.line_fn(ES.EDIT_STRANDS[mode], lnz, rows, node_ids, "r%d" % i, table, 0, -1)
                gate = S.expected(ES.EDIT_STRANDS[mode], rd, line_of)
                both = ES.expected(mode, rd, line_of)
                assert both[:3] == gate[:3], (mode, seed, rd, both[:3], gate[:3])
                if gate[1] == S.READ_BAD_BASE:
                    seen["bad"] += 1
                    continue
                assert S.score_of(gate[0]) <= 0, (mode, rd, gate[0])
                seen[gate[2]] += 1
                seen["zero"] += S.score_of(line_of(S.canonical(rd))) == 0
                seen["gate shut"] += gate[3] == ["+"]
                seen["tie"] += gate[3] == ["+", "-"] and S.score_of(line_of(V.rc(S.canonical(rd)))) == S.score_of(line_of(S.canonical(rd)))
    assert min(seen.values()) >= 4, seen


def test_the_rule_on_hand_cases():
    """Without a graph: scores by a table.  A forward score of 0 stays '+' whatever the reverse strand is given; ties stay '+'; a
    strictly greater reverse score wins; a bad base has no record."""
    def lines(scores):
        return lambda s: "r\t%d\t0\t%d\t+\t>1\t9\t0\t9\t0\t*\t*\t1M, best path: 0, score: %d\tA\n" % (len(s), len(s) - 1, scores[s])
    for mode in MODES:
        assert ES.expected(mode, "AAC", lines({"AAC": 0, "GTT": 0}))[1:] == (0, "+", ["+", "-"])
        assert ES.expected(mode, "AAC", lines({"AAC": -2, "GTT": -2}))[1:] == (0, "+", ["+", "-"])
        assert ES.expected(mode, "AAC", lines({"AAC": -2, "GTT": -1}))[1:] == (0, "-", ["+", "-"])
        assert ES.expected(mode, "AAC", lines({"AAC": -1, "GTT": -2}))[1:] == (0, "+", ["+", "-"])
        assert ES.expected(mode, "AAC", lines({"AAC": -3, "GTT": 0}))[0].split("\t")[4] == "-"
        assert ES.expected(mode, "ACGT", lines({"ACGT": -3}))[1:] == (0, "+", ["+", "-"])       # a reverse palindrome
        assert ES.expected(mode, "A?C", lines({})) == ("", 8, " ", [])
        for f, r in ((0, 0), (-2, -2), (-2, -1), (-1, -2), (-3, 0)):
            sc = lines({"AAC": f, "GTT": r})
            assert ES.expected(mode, "AAC", sc)[:3] == S.expected(ES.EDIT_STRANDS[mode], "AAC", sc)[:3]


# ---- 3. table and refusals ----

def test_the_constants_agree_on_every_side():
    from recgraph_amd import _lib, api
    header = open(os.path.join(ROOT, "include", "recgraph_hip.h")).read()
    rust = open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    modes_hpp = open(os.path.join(ROOT, "recgraph_amd", "csrc", "rg_edit_strands_modes.hpp")).read()
    for name, value in (("PATHWISE_EDIT_STRANDS", 64), ("PATHWISE_EDIT_SEMI_STRANDS", 65)):
        assert re.search(r"^#define RG_MODE_%s %d$" % (name, value), header, re.M)
        assert re.search(r"^pub const RG_MODE_%s: i32 = %d;$" % (name, value), rust, re.M)
        assert getattr(_lib, "MODE_" + name) == getattr(api, "MODE_" + name) == value
        assert "RG_MODE_%s" % name in modes_hpp
    assert api.PATHWISE_EDIT_STRANDS_MODES == _lib.EDIT_STRANDS_MODES == (64, 65) and _lib.EDIT_STRANDS_MAX_READ == 16383
    assert _lib.edit_strands_mode(64) is False and _lib.edit_strands_mode(65) is True
    assert [m for m in range(-2, 200) if _lib.edit_strands_mode(m) is not None] == [64, 65]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi
    assert gen_rust_ffi.generate() == rust


def test_the_modes_are_rows_of_neither_table_and_nothing_is_exported():
    from recgraph_amd import _lib
    for mode in MODES:
        assert _lib.edit_mode(mode) is None and _lib.gap_mode(mode) is None
        assert mode not in _lib.EDIT_MODE_NAMES.values() and mode not in _lib.GAP_MODE_NAMES.values()
    assert sorted(_lib.EDIT_MODE_NAMES.values()) == [44, 45, 94, 95]
    assert len(_lib.SYMBOLS) == 63
    exports = open(os.path.join(ROOT, "recgraph_amd", "csrc", "exports.map")).read()
    assert "edit" not in exports and "strand" not in exports
    host = open(os.path.join(ROOT, "recgraph_amd", "csrc", "rg_host.hpp")).read()
    assert len(re.findall(r"^\s*X\(", host[host.index("#define RG_OPTIONS"):host.index("#define RG_TUNING_OPTIONS")], re.M)) == 21
    for other in (63, 66, 67, 68, 69):
        rc, msg = _create(["ATGCT"], other)
        assert rc == -1 and "unsupported mode" in msg, (other, rc, msg)


@pytest.mark.parametrize("mode", MODES)
def test_the_modes_are_admitted_before_a_device_is_needed(mode):
    ok = -3 if no_device() else 0
    for n in (1, 1024, 1025, 16383):
        rc, msg = _create(["A" * n], mode)
        # (on the parent commit: RG_ERR_ARG "unsupported mode")
        assert rc == ok, (n, rc, msg)
    assert _create(["ATGCT", "A" * 3000, "C"], mode)[0] == ok
    assert _create(["ATGCT"], mode, entries=((4, 4, 0), (0, 1, 0)))[0] == ok
    assert _create(["ATGCT"], mode, entries=((0, 5, -2), (5, 2, -2), (5, 4, 7)))[0] == ok


@pytest.mark.parametrize("mode", MODES)
def test_every_amb_mode_is_admitted_or_refused_as_the_header_says(mode):
    ok = -3 if no_device() else 0
    for amb in range(16):
        rc, msg = _create(["ATGCT", "AC"], mode, amb=amb)
        if amb in (0, 4):
            assert rc == ok, (amb, rc, msg)
        else:
            assert rc == -1, (amb, rc, msg)
    # the vote: refused in the modes' own words, which say why
    rc, msg = _create(["ATGCT"], mode, amb=12)
    assert rc == -1 and "-m 64 / -m 65" in msg and "vote" in msg and "one pass" in msg, msg
    for amb in (16, 20, 32, 1 << 20):
        assert _create(["ATGCT"], mode, amb=amb)[0] == -1, amb
    # the one-strand modes keep refusing every bit
    for other in (44, 45, 94, 95):
        for amb in (4, 12):
            assert _create(["ATGCT"], other, amb=amb)[0] == -1, (other, amb)


@pytest.mark.parametrize("n", [5, 16384])
@pytest.mark.parametrize("mode", MODES)
def test_every_refusal_comes_before_a_device_is_needed(mode, n):
    reads = ["ATG", "A" * n]
    # the default scores (M = 2, X = 4, O = 4, E = 2), -O 4 and every other scoring: the message names the flags and modes 26 / 27
    for kw in (dict(match=2, mismatch=-4, o=-4, e=-2), dict(o=-4), dict(o=-1), dict(e=-2), dict(e=0), dict(match=1), dict(mismatch=-2),
               dict(entries=((4, 4, 1),)), dict(entries=((2, 4, -2),)), dict(entries=((3, 0, 2),))):
        rc, msg = _create(reads, mode, **kw)
        assert rc == -1 and FLAGS in msg and "-m 26 / -m 27" in msg and "-m 64 / -m 65" in msg, (kw, rc, msg)
    assert _create(reads, mode, o=1)[0] == -1
    assert _create(reads, mode, e=1)[0] == -1
    if n > 16383:
        rc, msg = _create(reads, mode)
        assert rc == -1 and "16383" in msg and "-m 64 / -m 65" in msg, (rc, msg)
        assert _create(["ATG", "A" * 16383], mode)[0] == (-3 if no_device() else 0)


def test_plan_routes_refusals_and_the_capacity_edge(tmp_path):
    plan_check_build.run_ok("edit_strands_plan_check", tmp_path, "edit strands plan ok")


def test_the_api_takes_the_modes_and_its_flag_rule():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for mode in MODES:
        # both_strands=True is redundant: the keyword becomes amb_mode 4, which the mode accepts
        assert api._both_strands_kw(mode, True, {}) == {"amb": api.AMB_BOTH_STRANDS}
        assert api._both_strands_kw(mode, False, {"o": 0}) == {"o": 0}
        for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
            with pytest.raises(api._lib.RecGraphError) as ex:
                fn(g, ["ATG"], mode=mode, strand_vote=True)
            assert "64, 65" in str(ex.value) and "one pass" in str(ex.value)
    for mode in (44, 45, 94, 95):
        with pytest.raises(api._lib.RecGraphError):
            api._both_strands_kw(mode, True, {})
    sig = inspect.signature(api.pathwise_alignment_edit_strands_exec).parameters
    assert list(sig) == ["sequence", "graph", "semi", "score_matrix"] and sig["semi"].default is False and sig["score_matrix"].default is None
    # the reference's default scoring is what the modes refuse, in the wrapper too
    with pytest.raises(api._lib.RecGraphError) as ex:
        api.pathwise_alignment_edit_strands_exec(["$"] + list("ATG"), g, score_matrix=api.create_score_matrix_i32(2, -4))
    assert ex.value.code == -1 and FLAGS in str(ex.value)


def test_the_cli_flag_rules_come_before_the_graph_is_opened(tmp_path):
    """The graph file named here does not exist: a refusal must come first, and an admitted command line fails to open it."""
    from recgraph_amd import cli
    unit = ["-M", "0", "-X", "1", "-O", "0", "-E", "1"]
    missing = str(tmp_path / "missing.gfa")
    for m in ("64", "65"):
        a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", m] + unit)
        assert a.alignment_mode == int(m)
        for args in ([], ["-M", "0", "-X", "1"], ["-O", "0", "-E", "1"], unit[:4] + ["-O", "4", "-E", "1"], unit[:6] + ["-E", "2"], ["-M", "1"] + unit[2:]):
            with pytest.raises(SystemExit) as ex:
                cli.main(["reads.fa", missing, "-m", m] + args)
            assert FLAGS in str(ex.value) and "-m 26 / -m 27" in str(ex.value), (m, args, str(ex.value))
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", missing, "-m", m, "--strand-vote"] + unit)
        assert "64, 65" in str(ex.value) and "one pass" in str(ex.value)
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", missing, "-m", m, "-s", "true"] + unit)
        assert "64 and 65" in str(ex.value)
        # --both-strands is redundant, and a 0 / -1 matrix file with -O 0 -E 1 passes: both then fail to open the graph
        with pytest.raises(OSError):
            cli.main(["reads.fa", missing, "-m", m, "--both-strands"] + unit)
        mtx = tmp_path / "unit.mtx"
        mtx.write_text("  A C G T N\n" + "".join("%s %s\n" % (r, " ".join("0" if r == c else "-1" for c in "ACGTN")) for r in "ACGTN"))
        with pytest.raises(OSError):
            cli.main(["reads.fa", missing, "-m", m, "-t", str(mtx), "-O", "0", "-E", "1"])
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", missing, "-m", m, "-t", str(mtx)])
        assert FLAGS in str(ex.value)
    assert "64, 65" in cli.build_parser().format_help()
    for m in ("63", "66"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", m])
        assert str(ex.value).startswith("Alignment mode must be in")


# ---- 5. resources ----

# VGPRs of k_edit_score_pair<W, kSemi> as built (global | semiglobal): the state of a lane is 7 W words (Peq of five bases, Pv, Mv) and
# a row step holds about 7 W more; the ceiling leaves 4 registers for a compiler's mood
_BUILT = {1: (22, 22), 2: (33, 36), 4: (57, 59), 8: (116, 116), 16: (229, 232)}


def test_the_kernels_keep_their_rows_in_registers():
    """No scratch, no spilled VGPR and no AGPR in the 11 instantiations of edit_strands/rg_edit_strands.hip, W = 16 included; LDS: the 32
    bytes of the match table (the duel: none)."""
    def cap(name):
        mm = re.search(r"k_edit_score_pair<(\d+), (true|false)>", name)
        return _BUILT[int(mm.group(1))][mm.group(2) == "true"] + 4 if mm else 16
    ks = assert_rows_in_registers("edit_strands/rg_edit_strands.hip", 11, vgprs=cap, lds=32)
    want = ["rg::k_edit_score_pair<%d, %s>" % (w, s) for w in (1, 2, 4, 8, 16) for s in ("false", "true")] + ["rg::k_edit_strands_duel"]
    assert sorted(k["name"] for k in ks) == sorted(want)
    assert all(k["SGPRs Spill"] == 0 for k in ks), [(k["name"], k["SGPRs Spill"]) for k in ks]
    assert all(k["LDS Size [bytes/block]"] == (0 if "duel" in k["name"] else 32) for k in ks)
    # the kernels of -m 44 / -m 45 keep their 17 instantiations
    assert len(assert_rows_in_registers("edit/rg_path_edit.hip", 17, vgprs=256, lds=32)) == 17
