"""CPU: the affine-gap pathwise modes for reads of up to 131071 bases (-m 56 / -m 57 / -m 62 = modes 6 / 7 / 12, `mode + 50`): admission
and refusals of rg_batch_create (answered before a device is needed), the plan's routes (tests/c/gap_xlong_plan_check.cpp), the API
and CLI surface and the registers of the new kernels."""
import inspect
import os

import pytest

import plan_check_build

from pathwise_support import TWO_BUBBLES, assert_rows_in_registers, create_rc, no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XLONG = {56: 6, 57: 7, 62: 12}
KERNELS = (["rg::k_gap_ckpt_long<%d>" % k for k in range(3)] + ["rg::k_gap_redo_long<%d>" % k for k in range(3)] +
           ["rg::k_gap_walk_long", "rg::k_gap_walk_local_long"])


@pytest.mark.parametrize("mode", sorted(XLONG))
def test_the_modes_are_admitted_and_refuse_before_a_device_is_needed(mode):
    ok = -3 if no_device() else 0
    rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode)
    # (on the parent commit: RG_ERR_ARG "unsupported mode")
    assert rc == ok, (rc, msg)
    # both sides of the limits of the base modes and of the long modes, and the new limit itself
    for n in (2047, 2048, 16383, 16384, 131071):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * n], mode)
        assert rc == ok, (n, rc, msg)
    rc, msg = create_rc(TWO_BUBBLES, ["ATG", "A" * 131072], mode)
    assert rc == -1 and "131071" in msg, (rc, msg)
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=1)[0] == -1
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, e=1)[0] == -1
    assert create_rc(TWO_BUBBLES, ["A" * 50000], mode, o=1)[0] == -1
    assert create_rc(TWO_BUBBLES, ["A" * 50000], mode, e=1)[0] == -1
    for amb in (1, 2, 4, 8, 12):
        assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, amb=amb)[0] == -1, amb
        assert create_rc(TWO_BUBBLES, ["A" * 30000], mode, amb=amb)[0] == -1, amb
    # the two capacity edges: (5 rows + 5 bases) * 2^25 >= 2^28, and (5 rows + 131067 bases) * 2^11 = 2^28
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25)[0] == -5
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=-(1 << 25))[0] == -5
    assert create_rc(TWO_BUBBLES, ["A" * 131067], mode, match=1 << 11)[0] == -5
    assert create_rc(TWO_BUBBLES, ["A" * 131066], mode, match=1 << 11)[0] == ok


def test_the_earlier_modes_keep_their_limits_and_the_gaps_between_the_modes_stay_closed():
    for mode in (6, 7, 12):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * 2048], mode)
        assert rc == -1 and "2047" in msg, (mode, rc, msg)
    for mode in (16, 17, 22, 26, 27, 32):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * 16384], mode)
        assert rc == -1 and "16383" in msg, (mode, rc, msg)
    for other in (36, 37, 42, 46, 47, 52, 50, 51, 53, 54, 55, 58, 59, 60, 61, 63, 66, 67, 72):
        rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], other)
        assert rc == -1 and "unsupported mode" in msg, (other, rc, msg)


def test_no_new_entry_point():
    from recgraph_amd import _lib
    assert len(_lib.SYMBOLS) == 63
    exports = open(os.path.join(ROOT, "recgraph_amd", "csrc", "exports.map")).read()
    assert "xlong" not in exports and "walk" not in exports


def test_the_api_refuses_both_strands_and_the_wrappers_take_the_modes():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for mode in sorted(XLONG):
        for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
            for kw in ({"both_strands": True}, {"strand_vote": True}):
                with pytest.raises(api._lib.RecGraphError) as ex:
                    fn(g, ["ATG"], mode=mode, **kw)
                assert "56, 57, 62" in str(ex.value)
    for fn in (api.pathwise_alignment_gap_exec, api.pathwise_alignment_gap_semi_exec, api.pathwise_alignment_gap_local_exec):
        par = inspect.signature(fn).parameters
        assert par["very_long_reads"].default is False and par["long_reads"].default is False and par["both_strands"].default is False
        with pytest.raises(api._lib.RecGraphError) as ex:
            fn(list("$ATG"), g, very_long_reads=True, both_strands=True)
        assert "very_long_reads" in str(ex.value)
    assert inspect.signature(api._gap_exec_mode).parameters["very_long_reads"].default is False
    assert [api._gap_exec_mode(m, False, False, True) for m in (6, 7, 12)] == [56, 57, 62]
    assert [api._gap_exec_mode(m, True, False, True) for m in (6, 7, 12)] == [56, 57, 62]
    assert [api._gap_exec_mode(m, True, False) for m in (6, 7, 12)] == [16, 17, 22]
    assert [api._gap_exec_mode(m, False, True) for m in (6, 7, 12)] == [26, 27, 32]
    with pytest.raises(api._lib.RecGraphError):
        api._gap_exec_mode(6, True, True, True)


def test_the_cli_takes_the_modes():
    from recgraph_amd import cli
    for m in sorted(XLONG):
        a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", str(m), "-O", "6", "-E", "1"])
        assert a.alignment_mode == m and (a.gap_open, a.gap_extension) == (6, 1)
        for flag in ("--both-strands", "--strand-vote"):
            with pytest.raises(SystemExit) as ex:
                cli.main(["reads.fa", "graph.gfa", "-m", str(m), flag])
            assert "56, 57 and 62" in str(ex.value)
        # admitted: the run gets as far as the graph file
        with pytest.raises((OSError, api_error())):
            cli.main(["no_such_reads.fa", "no_such_graph.gfa", "-m", str(m)])
    for m in ("36", "42", "46", "52", "55", "58", "61", "63", "66"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", m])
        assert str(ex.value) == "Alignment mode must be in [0..9], or 12"


def api_error():
    from recgraph_amd import api
    return api._lib.RecGraphError


def test_gap_xlong_plan_routes(tmp_path):
    plan_check_build.run_ok("gap_xlong_plan_check", tmp_path, "gap xlong plan ok")


def test_the_kernels_keep_their_rows_in_registers():
    """The family's bar: no scratch, no spilled VGPR, no AGPR, at most 200 VGPRs and no LDS beyond the score table's 160 B in every
    instantiation of gap_xlong/rg_path_gap_xlong.hip (DESIGN 4.12 lists the counts)."""
    ks = assert_rows_in_registers("gap_xlong/rg_path_gap_xlong.hip", len(KERNELS), vgprs=200, lds=160)
    assert sorted(k["name"] for k in ks) == sorted(KERNELS)


def test_the_shared_row_step_left_the_long_kernels_as_they_were():
    """gap_long/ keeps its one kernel file and its eight instantiations; what it shares with gap_xlong/ is a header, and no
    `__global__` lives there."""
    gl = os.path.join(ROOT, "recgraph_amd", "csrc", "gap_long")
    assert sorted(os.listdir(gl)) == ["rg_path_gap_long.hip", "rg_path_gap_long.hpp", "rg_path_gap_long_rows.hpp"]
    assert "__global__" not in open(os.path.join(gl, "rg_path_gap_long_rows.hpp")).read()
    gx = os.path.join(ROOT, "recgraph_amd", "csrc", "gap_xlong")
    assert sorted(f for f in os.listdir(gx) if f.endswith(".hip")) == ["rg_path_gap_xlong.hip"]
    src = open(os.path.join(gx, "rg_path_gap_xlong.hip")).read()
    assert "../gap_long/rg_path_gap_long_rows.hpp" in src and "asm" not in src
