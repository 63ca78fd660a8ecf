"""The kernel matrix of recgraph_amd/csrc/edit_xlong/rg_path_edit_xlong.hip (-m 94 / -m 95 with a read over 16383 bases): one entry per
compiled `__global__` instantiation, as data — the contract of tests/kernel_matrix.py, in the style of tests/kernel_matrix_edit.py.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as "inst:<name>")
to the id of a CASE that launches it.  tests/test_kernel_matrix_edit_xlong_cpu.py checks that the key set equals what hipcc compiles and
that the rule answers every case within the cell cap; tests/test_gpu_kernel_matrix_edit_xlong.py runs every case with the log on, checks
every read against the rule and asserts that the entry's instantiation was launched by every batch.

One case per mode.  The two batches of a case have the shortest longest read that runs these kernels (16384 bases: it fills stripe 0 to
its last bit, and the second stripe of the batch's S = 2 stays empty) and one that needs a third stripe for one column (32769), on 3
paths of about 250 rows.  Reads per batch: the longest,
built as random flank + noisy path + random flank; a piece of a path; one 1-base read."""
from collections import namedtuple

from kernel_matrix_gap_long import CELL_CAP

MODES = {94: False, 95: True}            # mode -> kSemi
LONGEST = [16384, 32769]

Case = namedtuple("Case", "mode graph batches")
CASES = {}
MATRIX = {}


def _fill():
    for mode, semi in MODES.items():
        cid = "edit-xlong-m%d" % mode
        CASES[cid] = Case(mode, ("haplotype", dict(target_rows=330, n_paths=3, path_len=250, seed=940 + mode)), list(LONGEST))
        MATRIX["rg::k_edit_score_xlong<%s>" % ("true" if semi else "false")] = cid
    MATRIX["rg::k_edit_redo_xlong"] = "edit-xlong-m94"
    MATRIX["rg::k_edit_walk_xlong"] = "edit-xlong-m95"


_fill()

PICK = "rg::k_gap_pick"          # what else a batch launches: the pick kernel of modes 6 / 7


def instantiations(case):
    """The four instantiations every batch of a case launches."""
    return {"rg::k_edit_score_xlong<%s>" % ("true" if MODES[case.mode] else "false"), PICK, "rg::k_edit_redo_xlong", "rg::k_edit_walk_xlong"}


def build(case):
    """(SynthGraph, [reads of batch 0, ...]); batch b, whose longest read has case.batches[b] bases: [flanked path, piece, 1-base read].
    The path ends on the read's last column in batch 0 (the walk starts with a diagonal on the stripe's last bit) and 700 columns
    short of it in batch 1."""
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
        left = hi - len(w) - (0 if bi == 0 else 700)
        flanked = flank(left) + w + flank(hi - left - len(w))
        v = g.path_sequence((bi + 2) % len(g.paths))
        batches.append([flanked, v[len(v) // 4: len(v) // 4 + 150], w[len(w) // 2]])
    return g, batches


def rule_cells(rows, batches):
    """rows x bases summed over the paths and reads of a case: the rule's cost in cells."""
    return sum(len(r) for r in rows) * sum(len(r) for b in batches for r in b)
