"""CPU: tests/kernel_matrix.py is complete and the oracle answers every case of it.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from recgraph_amd/csrc/*.hip
(tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU): a new instantiation without an entry fails here, and
so does an entry whose kernel is gone — deleting a `case` from a launcher's switch or adding a template member shows up
without a GPU.  Oracle wall time over the whole matrix, 8 threads: see test_the_oracle_answers_every_case."""
import os
import sys
import time

import kernel_matrix as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recgraph_amd", "csrc")
CELL_CAP = 10 ** 9        # oracle cells per case (rows x bases x paths), the budget stated in kernel_matrix.py


def _compiled():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    names = []
    for src in sorted(f for f in os.listdir(CSRC) if f.endswith(".hip")):
        names += [k["name"] for k in kernel_resources.report(src)]
    return names


def test_the_matrix_has_exactly_the_compiled_instantiations():
    names = _compiled()
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    compiled, keys = set(names), set(KM.MATRIX)
    assert compiled == keys, {"compiled without an entry": sorted(compiled - keys), "entries without a kernel": sorted(keys - compiled)}
    assert len(compiled) > 100


def test_every_entry_names_a_case_or_a_proved_impossibility():
    for name, v in KM.MATRIX.items():
        if isinstance(v, KM.Unreachable):
            # an instantiation may only be called unreachable with the host-only check that proves it: a file under tests/ and
            # a function in it (the check itself runs in its own test)
            path, func = v.proof
            assert v.reason and func in open(os.path.join(ROOT, path)).read(), name
        else:
            assert v in KM.CASES, name
    assert set(KM.CASES) == {v for v in KM.MATRIX.values() if not isinstance(v, KM.Unreachable)}      # no case without an entry
    # both sides of every C boundary, the first striped length, both sides of the LDS cut, the path counts at the page edges
    longest = {max(b) for c in KM.CASES.values() for b in c.batches}
    assert {255, 256, 511, 512, 1023, 1024, 2047, 2048, 16000, 16001} <= longest
    paths = {c.graph[1].get("n_paths") for c in KM.CASES.values()}
    assert {1, 64, 65, 129, 256} <= paths
    assert {c.graph[0] for c in KM.CASES.values()} == {"random_dag", "haplotype", "linear"}


def test_the_oracle_answers_every_case(oracle):
    """The expected text of every read of every case is computable: the oracle returns text and does not report would_panic.
    Cost: every case stays under CELL_CAP oracle cells.  Measured wall time of this test: printed below (-s)."""
    t0 = time.perf_counter()
    worst = (0, None)
    for cid, case in KM.CASES.items():
        g, batches = KM.build(case)
        assert [len(r) for r in batches[0]][:len(case.batches[0])] == case.batches[0], cid
        cells = KM.oracle_cells(g, case)
        worst = max(worst, (cells, cid))
        assert cells <= CELL_CAP, (cid, cells)
        for reads in batches:
            for i, (text, panic) in enumerate(KM.oracle_texts(oracle, case, g.gfa(), reads)):
                assert text and text.endswith("\n") and not panic, (cid, i, len(reads[i]), panic, text[-200:])
    print("kernel matrix: %d cases, oracle wall time %.1f s, largest case %s at %.2e cells" % (len(KM.CASES), time.perf_counter() - t0, worst[1], worst[0]))
