"""The kernel matrix of recgraph_amd/csrc/gap_xstrands/rg_gap_xstrands.hip (-m 76 / -m 77 / -m 82: the pick out of the pipeline and
back into it, the duel of the two strands' picks, the strand marks): one entry per compiled `__global__` instantiation, as data —
the contract of tests/kernel_matrix.py, in the style of tests/kernel_matrix_gap_strands.py.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as
"inst:<name>") to the id of a CASE that launches it.  tests/test_kernel_matrix_gap_xstrands_cpu.py checks that the key set equals
what hipcc compiles and that the rule answers the cases; tests/test_gpu_kernel_matrix_gap_xstrands.py runs the cases with the log
on, checks every read against the composed rule and asserts that the entry's instantiation was launched by every batch.

All four kernels take one lane per read in blocks of 256, so each case has a batch of more than 256 reads (two blocks, the second
partial; reads without a record among them, so that slots and read indices differ) beside a small one whose stages are striped (a
read over 2047 bases on the reverse strand).  Mode 82 picks every read on both strands; mode 77's case runs the duel on the reads
the gate lets through only."""
from collections import namedtuple

CELL_CAP = 5e7
Case = namedtuple("Case", "mode graph batches kw")
CASES = {"gap-xstrands-m82": Case(82, ("haplotype", dict(target_rows=160, n_paths=2, path_len=120, seed=832)), [300, 3], {}),
         "gap-xstrands-m77": Case(77, ("haplotype", dict(target_rows=160, n_paths=2, path_len=120, seed=877)), [300, 3], {})}
MATRIX = {"rg::k_gap_pick_out": "gap-xstrands-m82", "rg::k_gap_seed_pick": "gap-xstrands-m82",
          "rg::k_gap_xstrands_duel": "gap-xstrands-m77", "rg::k_gap_xstrands_mark": "gap-xstrands-m77"}


def build(case):
    """(SynthGraph, [reads of batch 0, ...]).  Batch of 300: 40-base pieces of the paths, every third on the reverse strand, every
    seventh with a bad base, every eleventh N only.  Batch of 3: a piece, a 2100-base read (flank + path + flank) on the reverse
    strand, an N-only read."""
    import numpy as np
    from recgraph_amd import synth
    import strand_vote_rule as V
    kind, args = case.graph
    g = {"haplotype": synth.haplotype_graph}[kind](**args)
    rng = np.random.default_rng(args["seed"])
    flank = lambda k: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=k))
    w = [g.path_sequence(k) for k in range(len(g.paths))]
    big = []
    for i in range(case.batches[0]):
        p = w[i % len(w)]
        q = (7 * i) % (len(p) - 40)
        rd = p[q:q + 40]
        if i % 3 == 1:
            rd = V.rc(rd)
        if i % 7 == 3:
            rd = rd[:20] + "?" + rd[21:]
        if i % 11 == 5:
            rd = "N" * 14
        big.append(rd)
    long_rd = flank(1200) + w[1] + flank(2100 - 1200 - len(w[1]))
    return g, [big, [w[0][10:70], V.rc(long_rd), "N" * 20]]


def rule_cells(rows, batches):
    """rows x bases summed over the paths and reads of a case, both strands: the rule's cost in cells."""
    return 2 * sum(len(r) for r in rows) * sum(len(r) for b in batches for r in b)
