"""CPU: tests/kernel_matrix_gap_local.py is complete and the rule answers every case of it.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/gap_local/rg_path_gap_local.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no other
file of that directory may hold a kernel without a matrix."""
import time

import kernel_matrix_gap_local as KL
import pathwise_gap_local_rule as L
from kernel_matrix_checks import assert_matrix_is_complete


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert_matrix_is_complete(KL, "gap_local/rg_path_gap_local.hip", 10)


def test_every_entry_names_a_case():
    assert set(KL.MATRIX.values()) == set(KL.CASES)
    assert {n for c in KL.CASES.values() for n in c.batches} == {255, 256, 511, 512, 1023, 1024, 2047}
    assert {c.graph[1]["n_paths"] for c in KL.CASES.values()} == {3, 6, 65, 256}
    assert {c.mode for c in KL.CASES.values()} == {12}


def test_the_rule_answers_every_case():
    from recgraph_amd import api
    t0 = time.perf_counter()
    worst = (0, None)
    whole_paths = 0
    for cid, case in KL.CASES.items():
        g, batches = KL.build(case)
        assert [max(len(r) for r in b) for b in batches] == case.batches and all(len(b[-1]) == 1 for b in batches), cid
        lnz, rows = L.graph_paths(api.Graph.from_gfa_text(g.gfa()))
        cells = KL.rule_cells(rows, batches)
        worst = max(worst, (cells, cid))
        assert cells <= KL.CELL_CAP, (cid, cells)
        for reads in batches:
            res = [L.align_local(lnz, rows, rd, None, case.kw.get("o", -4), case.kw.get("e", -2)) for rd in reads]
            assert all(r is not None and r[0] > 0 for r in res), cid
            score, k, end_row, end_col, stop_col, ops, pseq = res[0]
            # the flanked read is clipped on both sides; a whole path ends on its own last column
            assert stop_col > 0 and end_col < len(reads[0]), (cid, stop_col, end_col)
            if reads[1] in [g.path_sequence(q) for q in range(len(g.paths))]:
                whole_paths += 1
                assert (res[1][3], res[1][4], res[1][0]) == (len(reads[1]), 0, 2 * len(reads[1])), cid
    assert whole_paths >= len(KL.CASES)
    print("local gap kernel matrix: %d cases, rule wall time %.1f s, largest case %s at %.2e cells" % (len(KL.CASES), time.perf_counter() - t0, worst[1], worst[0]))
