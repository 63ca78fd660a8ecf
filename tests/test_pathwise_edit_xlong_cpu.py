"""CPU: the bit-vector edit-distance pathwise modes for reads of up to 131071 bases (-m 94 / -m 95 = modes 56 / 57 restricted to unit
costs): admission and refusals of rg_batch_create (answered before a device is needed), the constants on every side, the striped row step
of tests/pathwise_edit_xlong_rule.py against the whole-vector rule of tests/pathwise_edit_rule.py, the striped bit arithmetic of the
kernels on the host (tests/c/edit_xlong_bits_check.cpp), the plan (tests/c/edit_xlong_plan_check.cpp), the API and CLI surface and the
registers of the new kernels."""
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest

import pathwise_edit_rule as E
import pathwise_edit_xlong_rule as X
import pathwise_gap_rule as R
import plan_check_build

from pathwise_support import TWO_BUBBLES, assert_rows_in_registers, create_rc, no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XLONG = (94, 95)
FLAGS = "-M 0 -X 1 -O 0 -E 1"


# (return code, message) of rg_batch_create on TWO_BUBBLES at unit costs, each of them a keyword
_create = functools.partial(create_rc, TWO_BUBBLES, match=0, mismatch=-1, o=0, e=-1)


@pytest.mark.parametrize("mode", XLONG)
def test_the_modes_are_admitted_before_a_device_is_needed(mode):
    ok = -3 if no_device() else 0
    for n in (1, 16383, 16384, 131071):
        rc, msg = _create(["A" * n], mode)
        # (without the feature: RG_ERR_ARG "unsupported mode")
        assert rc == ok, (n, rc, msg)
    assert _create(["ATGCT", "A" * 20000, "C"], mode)[0] == ok
    # any 0 / -1 matrix: N matches N, A matches C; a '-' entry is not looked at
    assert _create(["ATGCT", "A" * 16385], mode, entries=((4, 4, 0), (0, 1, 0)))[0] == ok
    assert _create(["ATGCT"], mode, entries=((0, 5, -2), (5, 2, -2), (5, 4, 7)))[0] == ok


@pytest.mark.parametrize("n", [5, 16384, 131072])
@pytest.mark.parametrize("mode", XLONG)
def test_every_refusal_comes_before_a_device_is_needed(mode, n):
    reads = ["ATG", "A" * n]
    # the default scores (M = 2, X = 4, O = 4, E = 2) and every other scoring of tests/test_pathwise_edit_cpu.py: the message names the flags
    for kw in (dict(match=2, mismatch=-4, o=-4, e=-2), dict(o=-1), dict(e=-2), dict(e=0), dict(match=1), dict(mismatch=-2),
               dict(entries=((4, 4, 1),)), dict(entries=((2, 4, -2),)), dict(entries=((3, 0, 2),))):
        rc, msg = _create(reads, mode, **kw)
        assert rc == -1 and FLAGS in msg and "-m 94 / -m 95" in msg, (kw, rc, msg)
    # what mode 56 refuses
    assert _create(reads, mode, o=1)[0] == -1
    assert _create(reads, mode, e=1)[0] == -1
    for amb in (1, 2, 4, 8, 12, 16):
        rc, msg = _create(reads, mode, amb=amb)
        assert rc == -1, (amb, rc, msg)
    if n > 131071:
        rc, msg = _create(reads, mode)
        assert rc == -1 and "131071" in msg, (rc, msg)
        assert _create(["ATG", "A" * 131071], mode)[0] == (-3 if no_device() else 0)


def test_the_neighbours_stay_unsupported_and_modes_44_and_45_keep_their_limit():
    from recgraph_amd import _lib
    for other in (90, 91, 93, 98):
        rc, msg = _create(["ATGCT"], other)
        assert rc == -1 and "unsupported mode" in msg, (other, rc, msg)
    for mode in (44, 45):
        rc, msg = _create(["ATG", "A" * 16384], mode)
        assert rc == -1 and "16383" in msg and "-m 44 / -m 45" in msg, (mode, rc, msg)
    assert all(_lib.gap_mode(m) is None for m in XLONG)
    # one lookup: the same four modes, each with its rule, and modes 94 / 95 in a family of their own with its own reach
    assert [(m, _lib.edit_mode(m).semi, _lib.edit_mode(m).family.max_read) for m in range(-2, 200) if _lib.edit_mode(m)] == \
        [(44, False, 16383), (45, True, 16383), (94, False, 131071), (95, True, 131071)]
    assert _lib.edit_mode(94).family is _lib.edit_mode(95).family is not _lib.edit_mode(44).family and _lib.edit_mode(44).family is _lib.edit_mode(45).family


def test_no_new_entry_point():
    from recgraph_amd import _lib
    assert len(_lib.SYMBOLS) == 63
    exports = open(os.path.join(ROOT, "recgraph_amd", "csrc", "exports.map")).read()
    assert "edit" not in exports and "xlong" not in exports


def test_the_constants_agree_on_every_side():
    from recgraph_amd import _lib, api
    header = open(os.path.join(ROOT, "include", "recgraph_hip.h")).read()
    rust = open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    modes_hpp = open(os.path.join(ROOT, "recgraph_amd", "csrc", "rg_edit_modes.hpp")).read()
    for name, value in (("PATHWISE_EDIT_XLONG", 94), ("PATHWISE_EDIT_SEMI_XLONG", 95)):
        assert re.search(r"^#define RG_MODE_%s %d$" % (name, value), header, re.M)
        assert re.search(r"^pub const RG_MODE_%s: i32 = %d;$" % (name, value), rust, re.M)
        assert getattr(_lib, "MODE_" + name) == getattr(api, "MODE_" + name) == value
        assert "RG_MODE_%s" % name in modes_hpp
    assert api.PATHWISE_EDIT_XLONG_MODES == (94, 95) and api.PATHWISE_EDIT_MODES == (44, 45)
    assert _lib.edit_mode(94).family.max_read == 131071 and "EDIT_XLONG_MAX_READ == 131071" in modes_hpp and _lib.edit_mode(44).family.max_read == 16383
    assert modes_hpp.count("constexpr EditMode edit_") == 1 and "constexpr EditMode edit_mode(int mode)" in modes_hpp
    assert X.STRIPE == 16384 and "EDIT_XLONG_STRIPE = 32 * EDIT_MAX_WORDS * WAVE" in modes_hpp
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi
    assert gen_rust_ffi.generate() == rust


_N_MATCHES_N = R.default_scores(0, -1)
_N_MATCHES_N[4 * 6 + 4] = 0


@pytest.mark.parametrize("alphabet", ["ACGT", "ACGTN", "AC"])
def test_the_striped_row_step_is_the_row_step_on_the_whole_vector(alphabet):
    """Stripes of 3, 5 and 8 bits against pathwise_edit_rule.path_bits: Ph and D0 of every row and the last column of every row, a few
    hundred random small cases per alphabet, both kinds, the 0 / -1 table and the one in which N matches N; every value of hin occurs."""
    rng = np.random.default_rng(90 + len(alphabet))
    hins, cases = set(), 0
    for it in range(150):
        m, n = int(rng.integers(1, 14)), int(rng.integers(1, 25))
        bases = "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=m))
        read = "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n))
        if it % 7 == 0:
            read = (bases * 3)[:n]                   # long diagonals across the seams
        for scores in (R.default_scores(0, -1), _N_MATCHES_N):
            for semi in (False, True):
                want = E.path_bits(bases, read, scores, semi)
                for width in (3, 5, 8):
                    assert X.striped_bits(bases, read, scores, semi, width, hins) == want, (bases, read, semi, width)
                    cases += 1
    assert hins == {-1, 0, 1} and cases >= 1500


def test_the_rebuilt_cells_of_a_walk():
    # two stripes of 4: the walk starts in stripe 1 with 3 rows, enters stripe 0 with 2
    assert X.rebuilt("DLLDD", 3, 6, stripe=4) == (3 * 2 + 2 * 4, [1, 0])
    # row 0 reached in stripe 1: stripe 0 is never rebuilt; the semiglobal end in column 0 neither
    assert X.rebuilt("DD" + "L" * 5, 2, 7, stripe=4) == (2 * 3, [1])
    assert X.rebuilt("DDDD", 6, 4, stripe=4) == (6 * 4, [0])
    # a walk that leaves a stripe through its first column with a D and is then on the border
    assert X.rebuilt("D" + "L" * 4, 1, 5, stripe=4) == (1 * 1, [1])


def test_the_striped_bit_arithmetic_of_the_kernels_on_the_host(tmp_path):
    plan_check_build.run_ok("edit_xlong_bits_check", tmp_path, "edit xlong bits ok")


def test_edit_xlong_plan_routes(tmp_path):
    plan_check_build.run_ok("edit_xlong_plan_check", tmp_path, "edit xlong plan ok")


def test_the_api_takes_the_modes_and_refuses_both_strands():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for mode in XLONG:
        for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
            for flag in ("both_strands", "strand_vote"):
                with pytest.raises(api._lib.RecGraphError) as ex:
                    fn(g, ["ATG"], mode=mode, **{flag: True})
                assert "94, 95" in str(ex.value)
    sig = inspect.signature(api.pathwise_alignment_edit_xlong_exec).parameters
    assert list(sig) == ["sequence", "graph", "semi", "score_matrix"] and sig["semi"].default is False and sig["score_matrix"].default is None
    # the wrapper of modes 44 / 45 keeps its signature
    assert list(inspect.signature(api.pathwise_alignment_edit_exec).parameters) == ["sequence", "graph", "semi", "score_matrix"]


def test_the_cli_wants_the_unit_costs_spelled_out(tmp_path):
    """-m 94 / -m 95 without -M 0 -X 1 -O 0 -E 1 (or with a matrix that is not 0 / -1) are refused before the graph is opened: the
    graph file named here does not exist."""
    from recgraph_amd import cli
    unit = ["-M", "0", "-X", "1", "-O", "0", "-E", "1"]
    for m in ("94", "95"):
        a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", m] + unit)
        assert a.alignment_mode == int(m)
        for args in ([], ["-M", "0", "-X", "1"], ["-O", "0", "-E", "1"], unit[:6] + ["-E", "2"], ["-M", "1"] + unit[2:], unit[:2] + ["-X", "2"] + unit[4:]):
            with pytest.raises(SystemExit) as ex:
                cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m] + args)
            assert FLAGS in str(ex.value) and "-m 94 / -m 95" in str(ex.value), (m, args, str(ex.value))
        for flag in ("--both-strands", "--strand-vote"):
            with pytest.raises(SystemExit) as ex:
                cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m, flag] + unit)
            assert "94 and 95" in str(ex.value)
        # a 0 / -1 matrix file with -O 0 -E 1 passes the check (and then fails to open the graph); without the gap flags it does not
        mtx = tmp_path / "unit.mtx"
        mtx.write_text("  A C G T N\n" + "".join("%s %s\n" % (r, " ".join("0" if r == c else "-1" for c in "ACGTN")) for r in "ACGTN"))
        with pytest.raises(OSError):
            cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m, "-t", str(mtx), "-O", "0", "-E", "1"])
        with pytest.raises(OSError):
            cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m] + unit)
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m, "-t", str(mtx)])
        assert FLAGS in str(ex.value)
    for m in ("90", "91", "93", "96", "98"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", m])
        assert str(ex.value).startswith("Alignment mode must be in")


def test_the_kernels_keep_their_rows_in_registers():
    """No scratch, no spilled VGPR or SGPR and no AGPR in the 4 instantiations of edit_xlong/rg_path_edit_xlong.hip; LDS: the 32 bytes of
    the match table.  The kernels that hold EditLane<8> stay under the cap of edit/rg_path_edit.hip at W = 8, 16 W + 24; the walk holds a
    handful of scalars."""
    cap = lambda name: 32 if "walk" in name else 16 * 8 + 24
    ks = assert_rows_in_registers("edit_xlong/rg_path_edit_xlong.hip", 4, vgprs=cap, lds=32)
    want = ["rg::k_edit_score_xlong<false>", "rg::k_edit_score_xlong<true>", "rg::k_edit_redo_xlong", "rg::k_edit_walk_xlong"]
    assert sorted(k["name"] for k in ks) == sorted(want)
    assert all(k["SGPRs Spill"] == 0 for k in ks), [(k["name"], k["SGPRs Spill"]) for k in ks]
