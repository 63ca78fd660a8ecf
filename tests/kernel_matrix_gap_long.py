"""The kernel matrix of recgraph_amd/csrc/gap_long/rg_path_gap_long.hip (-m 16 / -m 17 / -m 22): one entry per compiled `__global__`
instantiation, as data — the contract of tests/kernel_matrix.py applied to the long-read gap kernels, in the style of
tests/kernel_matrix_gap_local.py.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as
"inst:<name>") to the id of a CASE that launches it.  tests/test_kernel_matrix_gap_long_cpu.py checks that the key set equals what
hipcc compiles and that the rules answer every case within the cell cap; tests/test_gpu_kernel_matrix_gap_long.py runs every case with
the log on, checks every read against the rule and asserts that the entry's instantiation was launched by every batch.

One case per kind (the template argument: 0 global, 1 semi, 2 local).  The longest read of a batch sits on either side of a stripe
boundary (2048: column 2048 alone in stripe 1; 4096: three stripes), on 3 paths of about 400 rows.  Reads per batch: the longest,
built as random flank + noisy path + random flank; a piece of a path (one stripe inside a striped batch); one 1-base read."""
from collections import namedtuple

CELL_CAP = 5e7
KINDS = {0: 16, 1: 17, 2: 22}
LONGEST = [2048, 4096]

Case = namedtuple("Case", "mode graph batches kw")
CASES = {}
MATRIX = {}


def _fill():
    for kind, mode in KINDS.items():
        cid = "gap-long-m%d" % mode
        CASES[cid] = Case(mode, ("haplotype", dict(target_rows=520, n_paths=3, path_len=400, seed=800 + mode)), list(LONGEST),
                          {"o": -6, "e": -1} if kind == 1 else {})
        MATRIX["rg::k_gap_score_long<%d>" % kind] = cid
        MATRIX["rg::k_gap_dirs_long<%d>" % kind] = cid
    MATRIX["rg::k_gap_trace_long"] = "gap-long-m17"
    MATRIX["rg::k_gap_trace_local_long"] = "gap-long-m22"


_fill()

# what else a batch of a case launches: the pick kernel of the base mode's file, told the striped width
PICK = {16: "rg::k_gap_pick", 17: "rg::k_gap_pick", 22: "rg::k_gap_pick_local"}
TRACE = {16: "rg::k_gap_trace_long", 17: "rg::k_gap_trace_long", 22: "rg::k_gap_trace_local_long"}


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
        # the path ends on the last column of the 2048-base read — column 2048, alone in stripe 1 — and inside stripe 1 of the 4096-base read
        left = hi - len(w) - (0 if hi == 2048 else 700)
        flanked = flank(left) + w + flank(hi - left - len(w))
        v = g.path_sequence((bi + 2) % len(g.paths))
        batches.append([flanked, v[len(v) // 4: len(v) // 4 + 150], w[len(w) // 2]])
    return g, batches


def rule_cells(rows, batches):
    """rows x bases summed over the paths and reads of a case: the rule's cost in cells."""
    return sum(len(r) for r in rows) * sum(len(r) for b in batches for r in b)
