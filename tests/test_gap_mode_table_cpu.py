"""CPU: the one table of the affine-gap pathwise modes (recgraph_amd/csrc/rg_gap_modes.hpp, recgraph_amd/_lib.py): every mode's value
in the header, _lib, api and the Rust shim, `value == base + offset`, api's tuples — and, byte for byte, every refusal of the plan and
of the API's and the CLI's flag rules as the commit before the table gave them (tests/golden/gap_plan_refusals.txt,
gap_mode_flag_refusals.txt)."""
import os
import subprocess

import pytest

import gap_mode_flag_dump
import plan_check_build

ROOT = plan_check_build.ROOT
BASES = {"": 6, "_SEMI": 7, "_LOCAL": 12}
OFFSETS = {"": 0, "_LONG": 10, "_STRANDS": 20, "_XLONG": 50, "_XSTRANDS": 70}
# what each of the fifteen names is worth, written out: the table must give these, not the other way round
VALUES = {
    "MODE_PATHWISE_GAP": 6, "MODE_PATHWISE_GAP_SEMI": 7,
    "MODE_PATHWISE_GAP_LOCAL": 12,
    "MODE_PATHWISE_GAP_LONG": 16, "MODE_PATHWISE_GAP_SEMI_LONG": 17,
    "MODE_PATHWISE_GAP_LOCAL_LONG": 22,
    "MODE_PATHWISE_GAP_STRANDS": 26, "MODE_PATHWISE_GAP_SEMI_STRANDS": 27,
    "MODE_PATHWISE_GAP_LOCAL_STRANDS": 32,
    "MODE_PATHWISE_GAP_XLONG": 56, "MODE_PATHWISE_GAP_SEMI_XLONG": 57,
    "MODE_PATHWISE_GAP_LOCAL_XLONG": 62,
    "MODE_PATHWISE_GAP_XSTRANDS": 76, "MODE_PATHWISE_GAP_SEMI_XSTRANDS": 77,
    "MODE_PATHWISE_GAP_LOCAL_XSTRANDS": 82,
}


def _family(suffix):
    return tuple(VALUES["MODE_PATHWISE_GAP%s%s" % (rule, suffix)] for rule in BASES)


@pytest.mark.parametrize("name", sorted(VALUES))
def test_the_constants(name):
    from recgraph_amd import api
    rule, suffix = next((r, s) for s in OFFSETS for r in BASES if name == "MODE_PATHWISE_GAP%s%s" % (r, s))
    v = VALUES[name]
    assert v == BASES[rule] + OFFSETS[suffix]
    assert getattr(api, name) == v and getattr(api._lib, name) == v
    assert getattr(api, "MODE_PATHWISE_GAP" + rule) + OFFSETS[suffix] == v
    assert "#define RG_%s %d\n" % (name, v) in open(os.path.join(ROOT, "include", "recgraph_hip.h")).read()
    assert "pub const RG_%s: i32 = %d;\n" % (name, v) in open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    gm = api._lib.gap_mode(v)
    assert (gm.family.suffix, gm.family.offset, api._lib.GAP_RULES[gm.rule]) == (suffix, OFFSETS[suffix], (rule, BASES[rule]))


def test_the_tuples_and_the_lookup():
    from recgraph_amd import api
    assert api.PATHWISE_GAP_MODES == _family("") + _family("_LONG")
    assert api.PATHWISE_GAP_STRANDS_MODES == _family("_STRANDS")
    assert api.PATHWISE_GAP_XLONG_MODES == _family("_XLONG")
    assert api.PATHWISE_GAP_XSTRANDS_MODES == _family("_XSTRANDS")
    tuples = (api.PATHWISE_GAP_MODES, api.PATHWISE_GAP_STRANDS_MODES, api.PATHWISE_GAP_XLONG_MODES, api.PATHWISE_GAP_XSTRANDS_MODES)
    assert sum(len(t) for t in tuples) == len(set().union(*tuples)) == len(VALUES)
    assert api._lib.GAP_MODE_NAMES == VALUES
    assert [m for m in range(-1, 200) if api._lib.gap_mode(m)] == sorted(VALUES.values())
    # the rows of the two tables agree: csrc/rg_gap_modes.hpp states each as {offset, max stripes, three flags, ...
    hpp = open(os.path.join(ROOT, "recgraph_amd", "csrc", "rg_gap_modes.hpp")).read()
    stripes = {1: "1", 8: "GAP_LONG_MAX_STRIPES", 64: "GAP_XLONG_MAX_STRIPES"}
    assert "GAP_LONG_MAX_STRIPES = 8;" in hpp and "GAP_XLONG_MAX_STRIPES = 64;" in hpp
    for f in api._lib.GAP_FAMILIES:
        flags = ", ".join(str(bool(x)).lower() for x in (f.both_strands, f.one_stripe_dirs, f.staged))
        assert "    {%d, %s, %s,\n" % (f.offset, stripes[f.max_stripes], flags) in hpp, f.suffix


def test_the_plan_refuses_what_it_refused(tmp_path):
    """tests/c/gap_plan_refusals_dump.cpp: every mode x amb_mode x length class x gap sign, return code, message and geometry."""
    out = subprocess.run([plan_check_build.build("gap_plan_refusals_dump", tmp_path)], capture_output=True, timeout=120).stdout
    assert out.count(b"\n") == 15 * 7 * 7 * 2
    assert out == open(os.path.join(ROOT, "tests", "golden", "gap_plan_refusals.txt"), "rb").read()


def test_the_flag_rules_refuse_what_they_refused():
    """api._both_strands_kw and cli.check_mode_flags in every mode the CLI admits, every combination of the two flags."""
    from recgraph_amd import cli
    modes = list(range(10)) + [v for v in sorted(VALUES.values()) if v >= 10]
    out = gap_mode_flag_dump.dump(modes, cli.check_mode_flags)
    assert out.count("\n") == len(modes) * 4 * 3
    assert out.encode() == open(os.path.join(ROOT, "tests", "golden", "gap_mode_flag_refusals.txt"), "rb").read()
