"""CPU: the long-read flavours of the affine-gap pathwise modes (-m 16 / -m 17 / -m 22 = modes 6 / 7 / 12 for reads of up to 16383
bases): admission and refusals of rg_batch_create (answered before a device is needed), the plan's routes
(tests/c/gap_long_plan_check.cpp), the API and CLI surface and the registers of the new kernels."""
import os

import pytest

import plan_check_build

from pathwise_support import TWO_BUBBLES, assert_rows_in_registers, create_rc, no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = {16: 6, 17: 7, 22: 12}


@pytest.mark.parametrize("mode", sorted(LONG))
def test_the_long_modes_are_admitted_and_refuse_before_a_device_is_needed(mode):
    ok = -3 if no_device() else 0
    rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], mode)
    # (on the parent commit: RG_ERR_ARG "unsupported mode")
    assert rc == ok, (rc, msg)
    # what the base modes refuse at 2048 bases is admitted up to 16383
    for n in (2047, 2048, 16383):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * n], mode)
        assert rc == ok, (n, rc, msg)
    rc, msg = create_rc(TWO_BUBBLES, ["ATG", "A" * 16384], mode)
    assert rc == -1 and "16383" in msg, (rc, msg)
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=1)[0] == -1
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, e=1)[0] == -1
    assert create_rc(TWO_BUBBLES, ["A" * 5000], mode, o=1)[0] == -1
    for amb in (1, 2, 4, 8, 12):
        assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, amb=amb)[0] == -1, amb
        assert create_rc(TWO_BUBBLES, ["A" * 3000], mode, amb=amb)[0] == -1, amb
    # (5 rows + 5 bases) * 2^25 >= 2^28, and (5 rows + 16379 bases) * 2^14 = 2^28
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, match=1 << 25)[0] == -5
    assert create_rc(TWO_BUBBLES, ["ATGCT"], mode, o=-(1 << 25))[0] == -5
    assert create_rc(TWO_BUBBLES, ["A" * 16379], mode, match=1 << 14)[0] == -5
    assert create_rc(TWO_BUBBLES, ["A" * 16378], mode, match=1 << 14)[0] == ok


def test_the_base_modes_keep_their_limit_and_the_gaps_between_the_modes_stay_closed():
    for mode in (6, 7, 12):
        rc, msg = create_rc(TWO_BUBBLES, ["A" * 2048], mode)
        assert rc == -1 and "2047" in msg, (mode, rc, msg)
    for other in (13, 14, 15, 18, 19, 20, 21, 23, -1):
        rc, msg = create_rc(TWO_BUBBLES, ["ATGCT"], other)
        assert rc == -1 and "unsupported mode" in msg, (other, rc, msg)


def test_no_new_entry_point():
    from recgraph_amd import _lib
    assert len(_lib.SYMBOLS) == 63
    exports = open(os.path.join(ROOT, "recgraph_amd", "csrc", "exports.map")).read()
    assert "long" not in exports


def test_the_api_refuses_both_strands_and_the_wrappers_take_the_long_modes():
    import inspect
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    for mode in sorted(LONG):
        assert mode in api.PATHWISE_GAP_MODES
        for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
            with pytest.raises(api._lib.RecGraphError):
                fn(g, ["ATG"], mode=mode, both_strands=True)
            with pytest.raises(api._lib.RecGraphError):
                fn(g, ["ATG"], mode=mode, strand_vote=True)
    for fn in (api.pathwise_alignment_gap_exec, api.pathwise_alignment_gap_semi_exec, api.pathwise_alignment_gap_local_exec):
        assert inspect.signature(fn).parameters["long_reads"].default is False


def test_the_cli_takes_the_modes():
    from recgraph_amd import cli
    for m in sorted(LONG):
        a = cli.build_parser().parse_args(["reads.fa", "graph.gfa", "-m", str(m), "-O", "6", "-E", "1"])
        assert a.alignment_mode == m and (a.gap_open, a.gap_extension) == (6, 1)
        for flag in ("--both-strands", "--strand-vote"):
            with pytest.raises(SystemExit) as ex:
                cli.main(["reads.fa", "graph.gfa", "-m", str(m), flag])
            assert "16, 17 and 22" in str(ex.value)
    for m in ("13", "14", "15", "18", "19", "20", "21", "23"):
        with pytest.raises(SystemExit) as ex:
            cli.main(["reads.fa", "graph.gfa", "-m", m])
        assert str(ex.value).startswith("Alignment mode must be in")


def test_gap_long_plan_routes(tmp_path):
    plan_check_build.run_ok("gap_long_plan_check", tmp_path, "gap long plan ok")


def test_the_kernels_keep_their_rows_in_registers():
    """The family's bar: no scratch, no spilled VGPR, no AGPR, at most 200 VGPRs and no LDS beyond the score table's 160 B in every
    instantiation of gap_long/rg_path_gap_long.hip (DESIGN 4.10 lists the counts)."""
    ks = assert_rows_in_registers("gap_long/rg_path_gap_long.hip", 8, vgprs=200, lds=160)
    assert sorted(k["name"] for k in ks) == sorted(["rg::k_gap_score_long<%d>" % k for k in range(3)] + ["rg::k_gap_dirs_long<%d>" % k for k in range(3)] +
                                                  ["rg::k_gap_trace_long", "rg::k_gap_trace_local_long"])
