"""CPU: the one table of the edit-distance pathwise modes (recgraph_amd/csrc/rg_edit_modes.hpp, recgraph_amd/_lib.py): every mode's value
in the header, _lib, api and the Rust shim, `value == base + offset`, the lookup with the rule and reach of each mode — and, byte for
byte, every answer of the plan and of the API's and the CLI's flag and scoring rules as the commit before the table gave them
(tests/golden/edit_plan_refusals.txt, edit_mode_flag_refusals.txt)."""
import os
import subprocess

import pytest

import gap_mode_flag_dump
import plan_check_build

ROOT = plan_check_build.ROOT
BASES = {"": 44, "_SEMI": 45}
OFFSETS = {"": 0, "_XLONG": 50}
# what each of the four names is worth, written out: the table must give these, not the other way round
VALUES = {"MODE_PATHWISE_EDIT": 44, "MODE_PATHWISE_EDIT_SEMI": 45, "MODE_PATHWISE_EDIT_XLONG": 94, "MODE_PATHWISE_EDIT_SEMI_XLONG": 95}


@pytest.mark.parametrize("name", sorted(VALUES))
def test_the_constants(name):
    from recgraph_amd import api
    rule, suffix = next((r, s) for s in OFFSETS for r in BASES if name == "MODE_PATHWISE_EDIT%s%s" % (r, s))
    v = VALUES[name]
    assert v == BASES[rule] + OFFSETS[suffix]
    assert getattr(api, name) == v and getattr(api._lib, name) == v
    assert getattr(api, "MODE_PATHWISE_EDIT" + rule) + OFFSETS[suffix] == v
    assert "#define RG_%s %d\n" % (name, v) in open(os.path.join(ROOT, "include", "recgraph_hip.h")).read()
    assert "pub const RG_%s: i32 = %d;\n" % (name, v) in open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    em = api._lib.edit_mode(v)
    assert (em.family.suffix, em.family.offset, api._lib.EDIT_RULES[em.semi]) == (suffix, OFFSETS[suffix], (rule, BASES[rule]))


def test_the_tuples_and_the_lookup():
    from recgraph_amd import api
    _lib = api._lib
    assert api.PATHWISE_EDIT_MODES == (44, 45) and api.PATHWISE_EDIT_XLONG_MODES == (94, 95)
    assert _lib.EDIT_MODE_NAMES == VALUES
    assert [m for m in range(-2, 200) if _lib.edit_mode(m)] == [44, 45, 94, 95]
    reach = {44: (False, 16383), 45: (True, 16383), 94: (False, 131071), 95: (True, 131071)}
    for m, (semi, max_read) in reach.items():
        em = _lib.edit_mode(m)
        assert (em.semi, em.family.max_read) == (semi, max_read) and em.semi is semi, m
        assert _lib.gap_mode(m) is None and m not in _lib.GAP_MODE_NAMES.values(), m
        # the gap family whose reads these are: the same reach
        assert _lib.gap_family(em.family.gap_suffix).max_stripes * 2048 - 1 == max_read, m
    # the rows of the two tables agree: csrc/rg_edit_modes.hpp states each as {offset, longest read, gap family, ...
    hpp = open(os.path.join(ROOT, "recgraph_amd", "csrc", "rg_edit_modes.hpp")).read()
    longest = {16383: "EDIT_MAX_READ", 131071: "EDIT_XLONG_MAX_READ"}
    assert "EDIT_MAX_READ == 16383" in hpp and "EDIT_XLONG_MAX_READ == 131071" in hpp
    assert hpp.count("\n    {") == len(_lib.EDIT_FAMILIES) == 2
    for f in _lib.EDIT_FAMILIES:
        assert "    {%d, %s, GAP_FAM%s,\n" % (f.offset, longest[f.max_read], f.gap_suffix) in hpp, f.suffix


def test_the_plan_answers_what_it_answered(tmp_path):
    """tests/c/edit_plan_refusals_dump.cpp: every mode x amb_mode x length class x scoring, return code, message and geometry."""
    out = subprocess.run([plan_check_build.build("edit_plan_refusals_dump", tmp_path)], capture_output=True, timeout=120).stdout
    assert out.count(b"\n") == 4 * 7 * 6 * 7
    assert out == open(os.path.join(ROOT, "tests", "golden", "edit_plan_refusals.txt"), "rb").read()


def test_the_flag_and_scoring_rules_answer_what_they_answered():
    """api._both_strands_kw and cli.check_mode_flags at every combination of the two flags, and cli.check_edit_scores at the unit
    costs, the default scores and a 0 / -1 matrix without -O 0 -E 1."""
    from recgraph_amd import cli
    modes = sorted(VALUES.values())
    out = gap_mode_flag_dump.dump(modes, cli.check_mode_flags) + gap_mode_flag_dump.dump_edit_scores(modes, cli.check_edit_scores)
    assert out.count("\n") == len(modes) * 4 * 3 + len(modes) * 3
    assert out.encode() == open(os.path.join(ROOT, "tests", "golden", "edit_mode_flag_refusals.txt"), "rb").read()
