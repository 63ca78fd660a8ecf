"""What the tests of the both-strands edit-distance pathwise modes (-m 64 / -m 65) share, beside tests/pathwise_support.py: the batch
runner at unit costs, the checker — every read against the composed rule of mode 26 / 27 at unit costs (expect_strands / check_strands
of tests/pathwise_support.py: line, status, strand / score / query accessors, CIGAR re-scored on the chosen strand) and both cell
counters against the formulas of include/recgraph_hip.h, computed from the rule's answers — and the builder of the stand-alone host
programs of tests/c/ that are also run under AddressSanitizer + UBSan.  A plain module: every assert carries its own message."""
import os
import subprocess

import pathwise_edit_strands_rule as ES
from pathwise_support import ROOT, check_strands, expect_strands, run_batch_strands, unit_costs

MODES = (64, 65)
BASE = ES.EDIT_STRANDS               # 64 -> 26, 65 -> 27: the modes whose answers these are
ONE_STRAND = {64: 44, 65: 45}        # ... and the modes whose kernels trace the strand that won
KERNELS = {"k_edit_score_pair", "k_gap_pick", "k_edit_strands_duel", "k_strand_orient", "k_edit_dirs", "k_edit_trace", "k_gap_xstrands_mark"}


def pair_words(longest):
    """W of k_edit_score_pair: the smallest of 1, 2, 4, 8, 16 with longest read <= 1024 W (a strand takes half a wave)."""
    return next(w for w in (1, 2, 4, 8, 16) if longest <= 1024 * w)


def dirs_words(longest):
    """W of k_edit_dirs, mode 44's: the smallest of 1, 2, 4, 8 with longest read <= 2048 W."""
    return next(w for w in (1, 2, 4, 8) if longest <= 2048 * w)


def instantiations(mode, longest):
    """The instantiations a chunk of a batch launches, by the launch log's names."""
    semi = "true" if mode == 65 else "false"
    return {"rg::k_edit_score_pair<%d, %s>" % (pair_words(longest), semi), "rg::k_gap_pick", "rg::k_edit_strands_duel", "rg::k_strand_orient",
            "rg::k_edit_dirs<%d, %s>" % (dirs_words(longest), semi), "rg::k_edit_trace", "rg::k_gap_xstrands_mark"}


def run(gg, reads, mode, scores=None, amb=None, log=False):
    """One batch of mode 64 / 65 at unit costs (or with the 0 / -1 table `scores`) through run_batch_strands."""
    return run_batch_strands(gg, reads, mode, amb=amb, log=log, scores=unit_costs() if scores is None else scores, o=0, e=-1)


def expect(graph, reads, mode, scores=None):
    """The answers of the exact rule of mode 26 / 27 at unit costs, read by read."""
    return expect_strands(graph, reads, BASE[mode], scores=unit_costs() if scores is None else scores, o=0, e=-1)


def check(graph, reads, mode, res=None, exp=None, scores=None):
    """Every read of a batch of mode 64 / 65 (run here, or `res`) against the rule of mode 26 / 27 at unit costs, the two counters
    against the header's formulas and the kernel set; returns (the batch, the rule's answers)."""
    from recgraph_amd import api
    sc = unit_costs() if scores is None else scores
    if res is None:
        res = run(graph[1], reads, mode, scores)
    exp = check_strands(graph, reads, BASE[mode], res, exp=exp, scores=sc, o=0, e=-1)
    want = ES.counters(mode, reads, exp, graph[2], graph[3], api._table_from_dict(sc))
    print("mode %d: cell counters %s, the formulas give %s" % (mode, res["cells"], want))
    assert res["cells"] == want, (mode, res["cells"], want)
    assert set(res["stats"]) == KERNELS, sorted(res["stats"])
    # per chunk: the pick twice, everything else once
    assert res["stats"]["k_gap_pick"] == 2 * res["stats"]["k_edit_trace"] == 2 * res["stats"]["k_edit_score_pair"], res["stats"]
    return res, exp


def build_host_program(name, out_dir, sanitize=False):
    """tests/c/<name>.cpp, a stand-alone main that needs nothing but the headers of csrc -> the path of the program, in out_dir."""
    exe = os.path.join(str(out_dir), name + ("_asan" if sanitize else ""))
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "recgraph_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", name + ".cpp")])
    return exe


def run_host_program(name, out_dir, ok_line, sanitize=False):
    r = subprocess.run([build_host_program(name, out_dir, sanitize)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == ok_line, (r.stdout, r.stderr[-4000:])
