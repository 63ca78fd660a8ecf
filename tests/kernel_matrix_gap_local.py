"""The kernel matrix of recgraph_amd/csrc/gap_local/rg_path_gap_local.hip (-m 12): one entry per compiled `__global__` instantiation,
as data — the contract of tests/kernel_matrix.py applied to the local gap kernels, which live in a subdirectory of their own.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as
"inst:<name>") to the id of a CASE that launches it.  tests/test_kernel_matrix_gap_local_cpu.py checks that the key set equals what
hipcc compiles and that the rule (tests/pathwise_gap_local_rule.py) answers every case within the cell cap;
tests/test_gpu_kernel_matrix_gap_local.py runs every case with the log on, checks every read against the rule and asserts that the
entry's instantiation was launched by every batch.

Shapes as in tests/kernel_matrix_gap.py: the longest read of a batch sits ON a boundary of C (255; 511 and 256; 1023 and 512; 2047 and
1024), 65 / 256 / 6 / 3 paths, the rule's cost under 5e7 cells per case.  Reads per batch: the longest, built as random flank + path
piece + random flank (query start > 0, end column < n); a whole path where it fits (the alignment ends on the read's last column, in
the boundary lane of that read) or a piece of one; one 1-base read (idle lanes)."""
from collections import namedtuple

import kernel_matrix_gap as KG

CS = KG.CS
CELL_CAP = KG.CELL_CAP
LONGEST = KG.LONGEST
PATHS = KG.PATHS
PATH_ROWS = {4: 200, 8: 100, 16: 1000, 32: 1100}

Case = namedtuple("Case", "mode graph batches kw")
CASES = {}
MATRIX = {}


def score(C):
    return "rg::k_gap_score_local<%d>" % C


def dirs(C):
    return "rg::k_gap_dirs_local<%d>" % C


def _fill():
    for C in CS:
        cid = "gap-local-C%d" % C
        n = PATH_ROWS[C]
        seed = 600 + C
        graph = (("haplotype", dict(target_rows=n * 13 // 10, n_paths=PATHS[C], path_len=n, seed=seed)) if C in (16, 32) else
                 ("random_dag", dict(n_segments=max(8, n * 10 // 36), n_paths=PATHS[C], seed=seed, max_seg=9, max_jump=2, similar=0.5)))
        CASES[cid] = Case(12, graph, list(LONGEST[C]), {"o": -6, "e": -1} if C == 8 else {})
        MATRIX[score(C)] = cid
        MATRIX[dirs(C)] = cid
    MATRIX["rg::k_gap_pick_local"] = "gap-local-C16"
    MATRIX["rg::k_gap_trace_local"] = "gap-local-C16"


_fill()


def build(case):
    """(SynthGraph, [reads of batch 0, ...]); batch b, whose longest read has case.batches[b] bases: [flanked piece, whole path or a
    piece of one, 1-base read]."""
    import numpy as np
    from recgraph_amd import synth
    kind, args = case.graph
    g = {"random_dag": synth.random_dag_graph, "haplotype": synth.haplotype_graph}[kind](**args)
    batches = []
    for bi, hi in enumerate(case.batches):
        rng = np.random.default_rng(11 * args["seed"] + bi)
        w = g.path_sequence((3 * bi + 1) % len(g.paths))
        piece = w[len(w) // 5: len(w) // 5 + min(hi // 2, len(w) // 2)]
        left = (hi - len(piece)) // 2
        flank = lambda k: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=k))
        flanked = flank(left) + piece + flank(hi - len(piece) - left)
        v = g.path_sequence((3 * bi + 2) % len(g.paths))
        whole = v if len(v) <= hi else v[len(v) // 3: len(v) // 3 + hi // 2]
        batches.append([flanked, whole, w[len(w) // 2]])
    return g, batches


def rule_cells(rows, batches):
    """rows x bases summed over the paths and reads of a case: the rule's cost in cells."""
    return sum(len(r) for r in rows) * sum(len(r) for b in batches for r in b)
