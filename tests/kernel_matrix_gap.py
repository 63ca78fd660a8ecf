"""The kernel matrix of recgraph_amd/csrc/gap/rg_path_gap.hip (-m 6 / -m 7): one entry per compiled `__global__` instantiation, as
data — the contract of tests/kernel_matrix.py applied to the gap kernels, which live in a subdirectory of their own.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as
"inst:<name>") to the id of a CASE that launches it.  A case is one or more batches of one mode on one synthetic graph.
tests/test_kernel_matrix_gap_cpu.py checks that the key set equals what hipcc compiles and that the rule
(tests/pathwise_gap_rule.py) answers every case within the cell cap; tests/test_gpu_kernel_matrix_gap.py runs every case with the
log on, checks every read against the rule and asserts that the entry's instantiation was launched by every batch.

How the cases are shaped: the plan doubles C (columns per lane) from 4 while 64 C < n + 1, so the longest read of a batch sits ON a
boundary — 255 (C = 4), 511 and 256 (8), 1023 and 512 (16), 2047 and 1024 (32) — beside a 1-base read (idle lanes) and one of
32 C bases.  Paths: 65 (more than one stride of k_gap_pick's lanes) at C = 4, 256 at C = 8, 6 at C = 16, 3 at C = 32; the graphs
keep rows x bases x paths, the rule's cost, under 5e7 cells per case."""
from collections import namedtuple

CS = (4, 8, 16, 32)
CELL_CAP = 5 * 10 ** 7
LONGEST = {4: (255,), 8: (511, 256), 16: (1023, 512), 32: (2047, 1024)}
PATHS = {4: 65, 8: 256, 16: 6, 32: 3}
PATH_ROWS = {4: 255, 8: 100, 16: 1000, 32: 1100}

Case = namedtuple("Case", "mode graph batches kw")
CASES = {}
MATRIX = {}


def _b(x):
    return "true" if x else "false"


def score(C, semi):
    return "rg::k_gap_score<%d, %s>" % (C, _b(semi))


def dirs(C, semi):
    return "rg::k_gap_dirs<%d, %s>" % (C, _b(semi))


def _fill():
    seed = 500
    for C in CS:
        hi, lo = LONGEST[C][0], LONGEST[C][-1]
        batches = [[hi, 32 * C, 1]] + ([[lo, 1, lo // 2]] if lo != hi else [])
        for semi in (False, True):
            seed += 1
            cid = "gap-C%d-%s" % (C, "semi" if semi else "global")
            n = PATH_ROWS[C]
            graph = (("haplotype", dict(target_rows=n * 13 // 10, n_paths=PATHS[C], path_len=n, seed=seed)) if C in (16, 32) else
                     ("random_dag", dict(n_segments=max(8, n * 10 // 36), n_paths=PATHS[C], seed=seed, max_seg=9, max_jump=2, similar=0.5)))
            CASES[cid] = Case(7 if semi else 6, graph, batches, {"o": -6, "e": -1} if C == 8 else {})
            MATRIX[score(C, semi)] = cid
            MATRIX[dirs(C, semi)] = cid
    MATRIX["rg::k_gap_pick"] = "gap-C16-global"
    MATRIX["rg::k_gap_trace"] = "gap-C16-global"


_fill()


def build(case):
    """(SynthGraph, [reads of batch 0, ...]): a read of n bases repeats a path's bases, with a substitution every 37 bases, a
    10-base deletion and a 7-base insertion where it is long enough."""
    import numpy as np
    from recgraph_amd import synth
    kind, args = case.graph
    g = {"random_dag": synth.random_dag_graph, "haplotype": synth.haplotype_graph}[kind](**args)
    batches = []
    for bi, lens in enumerate(case.batches):
        reads = []
        for k, n in enumerate(lens):
            rng = np.random.default_rng(7 * args["seed"] + 100 * bi + k)
            w = g.path_sequence((3 * bi + k) % len(g.paths))
            s = list((w * (n // len(w) + 2))[:n + 3])
            for q in range(5, len(s), 37):
                s[q] = "ACGT"[int(rng.integers(0, 4))]
            s = "".join(s)
            if n >= 64:
                s = s[:20] + s[30:40] + "GATTACA" + s[40:]
            reads.append(s[:n])
        batches.append(reads)
    return g, batches


def rule_cells(rows, case):
    """rows x bases summed over the paths and reads of a case: the rule's cost in cells."""
    return sum(len(r) for r in rows) * sum(sum(b) for b in case.batches)
