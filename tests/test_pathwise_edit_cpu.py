"""CPU: the bit-vector edit-distance pathwise modes (-m 44 / -m 45 = modes 16 / 17 restricted to unit costs): admission and refusals of
rg_batch_create (answered before a device is needed), the two constants on every side, the bit-vector rule of tests/pathwise_edit_rule.py
against the numpy rule of modes 6 / 7, the bit arithmetic of the kernels on the host (tests/c/edit_bits_check.cpp), the plan
(tests/c/edit_plan_check.cpp), the API and CLI surface and the registers of the new kernels."""
import functools
import os
import re
import sys

import numpy as np
import pytest

import pathwise_edit_rule as E
import pathwise_gap_rule as R
import plan_check_build

from pathwise_support import TWO_BUBBLES, assert_rows_in_registers, create_rc, no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDIT = (44, 45)
FLAGS = "-M 0 -X 1 -O 0 -E 1"


# (return code, message) of rg_batch_create on TWO_BUBBLES at unit costs, each of them a keyword
_create = functools.partial(create_rc, TWO_BUBBLES, match=0, mismatch=-1, o=0, e=-1)


@pytest.mark.parametrize("mode", EDIT)
def test_the_edit_modes_are_admitted_before_a_device_is_needed(mode):
    ok = -3 if no_device() else 0
    for n in (1, 2048, 2049, 16383):
        rc, msg = _create(["A" * n], mode)
        # (on the parent commit: RG_ERR_ARG "unsupported mode")
        assert rc == ok, (n, rc, msg)
    assert _create(["ATGCT", "A" * 3000, "C"], mode)[0] == ok
    # any 0 / -1 matrix: N matches N, A matches C; a '-' entry is not looked at
    assert _create(["ATGCT"], mode, entries=((4, 4, 0), (0, 1, 0)))[0] == ok
    assert _create(["ATGCT"], mode, entries=((0, 5, -2), (5, 2, -2), (5, 4, 7)))[0] == ok


@pytest.mark.parametrize("n", [5, 16384])
@pytest.mark.parametrize("mode", EDIT)
def test_every_refusal_comes_before_a_device_is_needed(mode, n):
    reads = ["ATG", "A" * n]
    # the default scores (M = 2, X = 4, O = 4, E = 2) and every other scoring: the message names the flags
    for kw in (dict(match=2, mismatch=-4, o=-4, e=-2), dict(o=-1), dict(e=-2), dict(e=0), dict(match=1), dict(mismatch=-2),
               dict(entries=((4, 4, 1),)), dict(entries=((2, 4, -2),)), dict(entries=((3, 0, 2),))):
        rc, msg = _create(reads, mode, **kw)
        assert rc == -1 and FLAGS in msg, (kw, rc, msg)
    # what mode 16 refuses
    assert _create(reads, mode, o=1)[0] == -1
    assert _create(reads, mode, e=1)[0] == -1
    for amb in (1, 2, 4, 8, 12, 16):
        rc, msg = _create(reads, mode, amb=amb)
        assert rc == -1, (amb, rc, msg)
    if n > 16383:
        rc, msg = _create(reads, mode)
        assert rc == -1 and "16383" in msg, (rc, msg)
        assert _create(["ATG", "A" * 16383], mode)[0] == (-3 if no_device() else 0)


def test_the_neighbours_stay_unsupported_and_the_modes_are_no_rows_of_the_gap_table():
    from recgraph_amd import _lib
    for other in (38, 39, 40, 41, 43, 48, 49):
        rc, msg = _create(["ATGCT"], other)
        assert rc == -1 and "unsupported mode" in msg, (other, rc, msg)
    assert _lib.gap_mode(44) is None and _lib.gap_mode(45) is None
    assert 44 not in _lib.GAP_MODE_NAMES.values() and 45 not in _lib.GAP_MODE_NAMES.values()
    assert [(m, _lib.edit_mode(m).semi, _lib.edit_mode(m).family.max_read) for m in range(-2, 200) if _lib.edit_mode(m)] == \
        [(44, False, 16383), (45, True, 16383), (94, False, 131071), (95, True, 131071)]


def test_no_new_entry_point():
    from recgraph_amd import _lib
    assert len(_lib.SYMBOLS) == 63
    exports = open(os.path.join(ROOT, "recgraph_amd", "csrc", "exports.map")).read()
    assert "edit" not in exports


def test_the_constants_agree_on_every_side():
    from recgraph_amd import _lib, api
    header = open(os.path.join(ROOT, "include", "recgraph_hip.h")).read()
    rust = open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    modes_hpp = open(os.path.join(ROOT, "recgraph_amd", "csrc", "rg_edit_modes.hpp")).read()
    for name, value in (("PATHWISE_EDIT", 44), ("PATHWISE_EDIT_SEMI", 45)):
        assert re.search(r"^#define RG_MODE_%s %d$" % (name, value), header, re.M)
        assert re.search(r"^pub const RG_MODE_%s: i32 = %d;$" % (name, value), rust, re.M)
        assert getattr(_lib, "MODE_" + name) == getattr(api, "MODE_" + name) == value
        assert "RG_MODE_%s" % name in modes_hpp
    assert api.PATHWISE_EDIT_MODES == (44, 45) and _lib.edit_mode(44).family.max_read == 16383 and "EDIT_MAX_READ == 16383" in modes_hpp
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi
    assert gen_rust_ffi.generate() == rust


_N_MATCHES_N = R.default_scores(0, -1)
_N_MATCHES_N[4 * 6 + 4] = 0


@pytest.mark.parametrize("alphabet", ["ACGT", "ACGTN", "AC"])
def test_the_bit_vector_rule_is_the_rule_of_modes_6_and_7_at_unit_costs(alphabet):
    """The row step and the walk on big integers against naive_scores (the last column of every row) and traceback (from EVERY end row),
    ties included: a few hundred random small cases per alphabet, both kinds, the 0 / -1 table and the one in which N matches N."""
    rng = np.random.default_rng(len(alphabet))
    walks = 0
    for it in range(120):
        m, n = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        bases = "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=m))
        read = "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n))
        if it % 10 == 0:
            read = bases[:n]                        # long diagonals, and equal rows in the semiglobal kind
        for scores in (R.default_scores(0, -1), _N_MATCHES_N):
            for semi in (False, True):
                last, bits = E.path_bits(bases, read, scores, semi)
                assert last == R.naive_scores(bases, read, scores, 0, -1, semi), (bases, read, semi)
                full = R.path_rows(bases, read, scores, 0, -1, semi, keep=True)
                assert last == [int(f[0][len(read)]) for f in full]
                for m_end in range(1, m + 1):
                    assert E.walk(bits, bases, read, scores, m_end, semi) == R.traceback(full, m_end, len(read), 0, -1, semi), (bases, read, semi, m_end)
                    walks += 1
    assert walks >= 1000


def test_the_bit_arithmetic_of_the_kernels_on_the_host(tmp_path):
    plan_check_build.run_ok("edit_bits_check", tmp_path, "edit bits ok")


def test_edit_plan_routes(tmp_path):
    plan_check_build.run_ok("edit_plan_check", tmp_path, "edit plan ok")


def test_the_api_takes_the_modes_and_refuses_both_strands():
    import inspect
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for mode in EDIT:
        for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
            for flag in ("both_strands", "strand_vote"):
                with pytest.raises(api._lib.RecGraphError) as ex:
                    fn(g, ["ATG"], mode=mode, **{flag: True})
                assert "44, 45" in str(ex.value)
    sig = inspect.signature(api.pathwise_alignment_edit_exec).parameters
    assert list(sig) == ["sequence", "graph", "semi", "score_matrix"] and sig["semi"].default is False and sig["score_matrix"].default is None
    # the default matrix of the wrapper is the 0 / -1 one; the reference's default is what the modes refuse
    t = api._table_from_dict(api.create_score_matrix_i32(0, -1))
    assert api._lib.unit_costs(t, 0, -1) and not api._lib.unit_costs(t, -4, -2) and not api._lib.unit_costs(t, 0, 0)
    assert not api._lib.unit_costs(api._table_from_dict(api.create_score_matrix_i32(2, -4)), 0, -1)


def test_the_cli_wants_the_unit_costs_spelled_out(tmp_path):
    """-m 44 / -m 45 without -M 0 -X 1 -O 0 -E 1 (or with a matrix that is not 0 / -1) are refused before the graph is opened: the
    graph file named here does not exist."""
    from recgraph_amd import cli
    unit = ["-M", "0", "-X", "1", "-O", "0", "-E", "1"]
    for m in ("44", "45"):
        a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", m] + unit)
        assert a.alignment_mode == int(m)
        for args in ([], ["-M", "0", "-X", "1"], ["-O", "0", "-E", "1"], unit[:6] + ["-E", "2"], ["-M", "1"] + unit[2:], unit[:2] + ["-X", "2"] + unit[4:]):
            with pytest.raises(SystemExit) as ex:
                cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m] + args)
            assert FLAGS in str(ex.value), (m, args, str(ex.value))
        for flag in ("--both-strands", "--strand-vote"):
            with pytest.raises(SystemExit) as ex:
                cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m, flag] + unit)
            assert "44 and 45" in str(ex.value)
        # a 0 / -1 matrix file with -O 0 -E 1 passes the check (and then fails to open the graph); HOXD70 does not
        mtx = tmp_path / "unit.mtx"
        mtx.write_text("  A C G T N\n" + "".join("%s %s\n" % (r, " ".join("0" if r == c else "-1" for c in "ACGTN")) for r in "ACGTN"))
        with pytest.raises(OSError):
            cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m, "-t", str(mtx), "-O", "0", "-E", "1"])
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m, "-t", str(mtx)])
        assert FLAGS in str(ex.value)
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", str(tmp_path / "missing.gfa"), "-m", m, "-t", os.path.join(ROOT, "tests", "golden", "HOXD70.mtx"), "-O", "0", "-E", "1"])
        assert FLAGS in str(ex.value)
    for m in ("38", "41", "43", "46", "48"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", m])
        assert str(ex.value).startswith("Alignment mode must be in")


def test_the_kernels_keep_their_rows_in_registers():
    """No scratch, no spilled VGPR and no AGPR in the 17 instantiations of edit/rg_path_edit.hip; LDS: the 32 bytes of the match table."""
    # the state of a lane is 7 W words (Peq of five bases, Pv, Mv) and a row step holds a handful of W more
    cap = lambda name: 16 * (int(re.search(r"<(\d)", name).group(1)) if "<" in name else 1) + 24
    ks = assert_rows_in_registers("edit/rg_path_edit.hip", 17, vgprs=cap, lds=32)
    want = ["rg::k_edit_%s<%d, %s>" % (k, w, s) for k in ("score", "dirs") for w in (1, 2, 4, 8) for s in ("false", "true")] + ["rg::k_edit_trace"]
    assert sorted(k["name"] for k in ks) == sorted(want) and len(ks) == 17
    assert all(k["SGPRs Spill"] == 0 for k in ks), [(k["name"], k["SGPRs Spill"]) for k in ks]
