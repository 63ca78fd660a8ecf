"""The kernel matrix of recgraph_amd/csrc/edit/rg_path_edit.hip (-m 44 / -m 45): one entry per compiled `__global__` instantiation, as
data — the contract of tests/kernel_matrix.py applied to the bit-vector edit-distance kernels, in the style of
tests/kernel_matrix_gap_long.py.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as "inst:<name>")
to the id of a CASE that launches it.  tests/test_kernel_matrix_edit_cpu.py checks that the key set equals what hipcc compiles and that
the rule answers every case within the cell cap; tests/test_gpu_kernel_matrix_edit.py runs every case with the log on, checks every read
against the rule and asserts that the entry's instantiation was launched by every batch.

One case per (mode, W).  W is the smallest with longest read <= 2048 W, and the two batches of a case reach it from both sides: the
shortest longest read that needs W (W = 1: one base) and the longest it takes (2048 W; W = 8: 16383, the modes' limit), on 3 paths of
about 250 rows.  Reads per batch: the longest, built as random flank + noisy path + random flank; a piece of a path; one 1-base read."""
from collections import namedtuple

from kernel_matrix_gap_long import CELL_CAP

MODES = {44: False, 45: True}            # mode -> kSemi
WORDS = {1: [1, 2048], 2: [2049, 4096], 4: [4097, 8192], 8: [8193, 16383]}

Case = namedtuple("Case", "mode words graph batches")
CASES = {}
MATRIX = {}


def _fill():
    for mode, semi in MODES.items():
        for w, longest in WORDS.items():
            cid = "edit-m%d-w%d" % (mode, w)
            CASES[cid] = Case(mode, w, ("haplotype", dict(target_rows=330, n_paths=3, path_len=250, seed=440 + mode + w)), list(longest))
            targs = "<%d, %s>" % (w, "true" if semi else "false")
            MATRIX["rg::k_edit_score" + targs] = cid
            MATRIX["rg::k_edit_dirs" + targs] = cid
    MATRIX["rg::k_edit_trace"] = "edit-m45-w2"


_fill()

PICK = "rg::k_gap_pick"          # what else a batch launches: the pick kernel of modes 6 / 7
TRACE = "rg::k_edit_trace"


def instantiations(case):
    """The four instantiations every batch of a case launches."""
    targs = "<%d, %s>" % (case.words, "true" if MODES[case.mode] else "false")
    return {"rg::k_edit_score" + targs, PICK, "rg::k_edit_dirs" + targs, TRACE}


def build(case):
    """(SynthGraph, [reads of batch 0, ...]); batch b, whose longest read has case.batches[b] bases: [flanked path, piece, 1-base read]
    (a 1-base longest read: that read alone)."""
    import numpy as np
    from recgraph_amd import synth
    kind, args = case.graph
    g = {"haplotype": synth.haplotype_graph}[kind](**args)
    batches = []
    for bi, hi in enumerate(case.batches):
        rng = np.random.default_rng(13 * args["seed"] + bi)
        flank = lambda k: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=k))
        w = list(g.path_sequence((bi + 1) % len(g.paths)))
        for k in range(40, len(w), 83):
            w[k] = "ACGT"[("ACGT".index(w[k]) + 1) % 4]
        w = "".join(w)
        if hi == 1:
            batches.append([w[len(w) // 3]])
            continue
        # the path ends on the read's last column when the read fills its W words, well inside otherwise
        left = hi - len(w) - (0 if hi % 2048 == 0 else 700)
        flanked = flank(left) + w + flank(hi - left - len(w))
        v = g.path_sequence((bi + 2) % len(g.paths))
        batches.append([flanked, v[len(v) // 4: len(v) // 4 + 150], w[len(w) // 2]])
    return g, batches


def rule_cells(rows, batches):
    """rows x bases summed over the paths and reads of a case: the rule's cost in cells."""
    return sum(len(r) for r in rows) * sum(len(r) for b in batches for r in b)
