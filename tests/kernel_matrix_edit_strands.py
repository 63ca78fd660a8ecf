"""The kernel matrix of recgraph_amd/csrc/edit_strands/rg_edit_strands.hip (-m 64 / -m 65): one entry per compiled `__global__`
instantiation, as data — the contract of tests/kernel_matrix.py applied to the both-strands edit-distance kernels, in the style of
tests/kernel_matrix_edit.py.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as "inst:<name>")
to the id of a CASE that launches it.  tests/test_kernel_matrix_edit_strands_cpu.py checks that the key set equals what hipcc compiles
and that the rule answers every case within the cell cap; tests/test_gpu_kernel_matrix_edit_strands.py runs every case with the log on,
checks every read against the rule of mode 26 / 27 at unit costs and asserts that the entry's instantiation was launched by every batch.

One case per (mode, W).  W is the smallest with longest read <= 1024 W (a strand takes half a wave), and the two batches of a case reach
it from both sides: the shortest longest read that needs W (W = 1: one base) and the longest it takes (1024 W; W = 16: 16383, the modes'
limit), on 3 paths of about 250 rows.  Reads per batch: the longest, built as N-rich random flank + noisy path + N-rich random flank and given on the
REVERSE strand in the second batch; a piece of a path, reverse-complemented in the first; one 1-base read."""
from collections import namedtuple

from kernel_matrix_gap_long import CELL_CAP

MODES = {64: False, 65: True}            # mode -> kSemi
WORDS = {1: [1, 1024], 2: [1025, 2048], 4: [2049, 4096], 8: [4097, 8192], 16: [8193, 16383]}

Case = namedtuple("Case", "mode words graph batches")
CASES = {}
MATRIX = {}


def _fill():
    for mode, semi in MODES.items():
        for w, longest in WORDS.items():
            cid = "edit-strands-m%d-w%d" % (mode, w)
            CASES[cid] = Case(mode, w, ("haplotype", dict(target_rows=330, n_paths=3, path_len=250, seed=640 + mode + w)), list(longest))
            MATRIX["rg::k_edit_score_pair<%d, %s>" % (w, "true" if semi else "false")] = cid
    MATRIX["rg::k_edit_strands_duel"] = "edit-strands-m65-w2"


_fill()

DUEL = "rg::k_edit_strands_duel"


def _rc(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, c) for c in reversed(s))      # (N stays)


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
        # (at unit costs a path is a subsequence of any long random read, on either strand: the flanks are N, which matches
        # nothing, but for about a hundred random bases, so that the path's own strand decides)
        flank = lambda k: "".join("ACGT"[int(x)] if u < min(0.25, 100 / max(k, 1)) else "N" for x, u in zip(rng.integers(0, 4, size=k), rng.random(k)))
        w = list(g.path_sequence((bi + 1) % len(g.paths)))
        for k in range(40, len(w), 83):
            w[k] = "ACGT"[("ACGT".index(w[k]) + 1) % 4]
        w = "".join(w)
        if hi == 1:
            batches.append([w[len(w) // 3]])
            continue
        # the path ends on the read's last column when the read fills its W words, well inside otherwise
        left = max(0, hi - len(w) - (0 if hi % 1024 == 0 else 300))
        flanked = (flank(left) + w + flank(max(0, hi - left - len(w))))[:hi]
        v = g.path_sequence((bi + 2) % len(g.paths))
        piece = v[len(v) // 4: len(v) // 4 + 150]
        batches.append([_rc(flanked) if bi else flanked, piece if bi else _rc(piece), w[len(w) // 2]])
    return g, batches


def rule_cells(rows, batches):
    """rows x bases summed over the paths and reads of a case, both strands: the rule's cost in cells."""
    return 2 * sum(len(r) for r in rows) * sum(len(r) for b in batches for r in b)
