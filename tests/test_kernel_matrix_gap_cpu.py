"""CPU: tests/kernel_matrix_gap.py is complete and the rule answers every case of it.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/gap/rg_path_gap.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no other file of
that directory may hold a kernel without a matrix."""
import time

import kernel_matrix_gap as KG
import pathwise_gap_rule as R
from kernel_matrix_checks import assert_matrix_is_complete


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert_matrix_is_complete(KG, "gap/rg_path_gap.hip", 18)


def test_every_entry_names_a_case():
    assert set(KG.MATRIX.values()) == set(KG.CASES)
    longest = {max(b) for c in KG.CASES.values() for b in c.batches}
    assert longest == {255, 256, 511, 512, 1023, 1024, 2047}
    assert {c.graph[1]["n_paths"] for c in KG.CASES.values()} == {3, 6, 65, 256}
    assert {c.mode for c in KG.CASES.values()} == {6, 7}


def test_the_rule_answers_every_case():
    from recgraph_amd import api
    t0 = time.perf_counter()
    worst = (0, None)
    for cid, case in KG.CASES.items():
        g, batches = KG.build(case)
        assert [[len(r) for r in b] for b in batches] == case.batches, cid
        lnz, rows = R.graph_paths(api.Graph.from_gfa_text(g.gfa()))
        cells = KG.rule_cells(rows, case)
        worst = max(worst, (cells, cid))
        assert cells <= KG.CELL_CAP, (cid, cells)
        for reads in batches:
            for rd in reads:
                score, k, end_row, ops, pseq = R.align(lnz, rows, rd, None, case.kw.get("o", -4), case.kw.get("e", -2), case.mode == 7)
                assert 0 <= k < len(rows) and end_row in rows[k] and ops.count("D") + ops.count("L") == len(rd), (cid, len(rd))
    print("gap kernel matrix: %d cases, rule wall time %.1f s, largest case %s at %.2e cells" % (len(KG.CASES), time.perf_counter() - t0, worst[1], worst[0]))
