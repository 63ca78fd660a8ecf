"""The kernel matrix of recgraph_amd/csrc/gap_xlong/rg_path_gap_xlong.hip (-m 56 / -m 57 / -m 62): one entry per compiled
`__global__` instantiation, as data — the contract of tests/kernel_matrix.py applied to the one-stripe traceback, in the style of
tests/kernel_matrix_gap_long.py.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as
"inst:<name>") to the id of a CASE that launches it.  tests/test_kernel_matrix_gap_xlong_cpu.py checks that the key set equals what
hipcc compiles and that the rules answer every case within the cell cap; tests/test_gpu_kernel_matrix_gap_xlong.py runs every case
with the log on, checks every read against the rule and asserts that the entry's instantiation was launched by every batch.

One case per kind (the template argument: 0 global, 1 semi, 2 local).  The longest read of a batch has 2048 bases (column 2048 alone
in stripe 1: what modes 16 / 17 / 22 take as well) or 16384 (nine stripes: what no earlier mode takes), on 3 paths of about 300 rows.
Reads per batch: the longest, built as random flank + noisy path + random flank; a piece of a path (one stripe inside a striped
batch); one 1-base read."""
from collections import namedtuple

CELL_CAP = 5e7
ROW_CAP = 12_000_000          # rows of the longest path x (n + 1) per read: the rule's four int64 matrices stay under about 400 MB
KINDS = {0: 56, 1: 57, 2: 62}
LONGEST = [2048, 16384]

Case = namedtuple("Case", "mode graph batches kw")
CASES = {}
MATRIX = {}


def _fill():
    for kind, mode in KINDS.items():
        cid = "gap-xlong-m%d" % mode
        CASES[cid] = Case(mode, ("haplotype", dict(target_rows=390, n_paths=3, path_len=300, seed=900 + mode)), list(LONGEST),
                          {"o": -6, "e": -1} if kind == 1 else {})
        MATRIX["rg::k_gap_ckpt_long<%d>" % kind] = cid
        MATRIX["rg::k_gap_redo_long<%d>" % kind] = cid
    MATRIX["rg::k_gap_walk_long"] = "gap-xlong-m57"
    MATRIX["rg::k_gap_walk_local_long"] = "gap-xlong-m62"


_fill()

# what else a batch of a case launches: the score pass of gap_long/ and the pick kernel of the base mode's file, told the striped width
SCORE = {56: "rg::k_gap_score_long<0>", 57: "rg::k_gap_score_long<1>", 62: "rg::k_gap_score_long<2>"}
PICK = {56: "rg::k_gap_pick", 57: "rg::k_gap_pick", 62: "rg::k_gap_pick_local"}
WALK = {56: "rg::k_gap_walk_long", 57: "rg::k_gap_walk_long", 62: "rg::k_gap_walk_local_long"}


def build(case):
    """(SynthGraph, [reads of batch 0, ...]); batch b, whose longest read has case.batches[b] bases: [flanked path, piece, 1-base read]."""
    import numpy as np
    from recgraph_amd import synth
    kind, args = case.graph
    g = {"haplotype": synth.haplotype_graph}[kind](**args)
    batches = []
    for bi, hi in enumerate(case.batches):
        rng = np.random.default_rng(11 * args["seed"] + bi)
        flank = lambda k: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=k))
        w = list(g.path_sequence((bi + 1) % len(g.paths)))
        for k in range(40, len(w), 83):
            w[k] = "ACGT"[("ACGT".index(w[k]) + 1) % 4]
        w = "".join(w)
        # the path ends on the last column of the 2048-base read — column 2048, alone in stripe 1 — and inside stripe 7 of 9 of the other
        left = hi - len(w) - (0 if hi == 2048 else 700)
        flanked = flank(left) + w + flank(hi - left - len(w))
        v = g.path_sequence((bi + 2) % len(g.paths))
        batches.append([flanked, v[len(v) // 4: len(v) // 4 + 150], w[len(w) // 2]])
    return g, batches


def rule_cells(rows, batches):
    """rows x bases summed over the paths and reads of a case: the rule's cost in cells."""
    return sum(len(r) for r in rows) * sum(len(r) for b in batches for r in b)
