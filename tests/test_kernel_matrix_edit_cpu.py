"""CPU: tests/kernel_matrix_edit.py is complete and the rule answers every case of it.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/edit/rg_path_edit.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no other file of
that directory may hold a kernel without a matrix."""
import time

import kernel_matrix_edit as KE
import kernel_matrix_gap_long as KG
import pathwise_gap_rule as R
from kernel_matrix_checks import assert_matrix_is_complete


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert_matrix_is_complete(KE, "edit/rg_path_edit.hip", 17)


def test_every_entry_names_a_case_and_every_width_is_reached_from_both_sides():
    assert set(KE.MATRIX.values()) == set(KE.CASES)
    assert {c.mode for c in KE.CASES.values()} == {44, 45} and {c.words for c in KE.CASES.values()} == {1, 2, 4, 8}
    for cid, case in KE.CASES.items():
        lo, hi = case.batches
        # the plan's rule: the smallest W with longest read <= 2048 W
        assert hi <= 2048 * case.words and (hi == 2048 * case.words or hi == 16383), cid
        assert lo == (2048 * case.words // 2 + 1 if case.words > 1 else 1), cid
    for name, cid in KE.MATRIX.items():
        assert name in KE.instantiations(KE.CASES[cid]), (name, cid)
    assert KE.CELL_CAP == KG.CELL_CAP


def test_the_rule_answers_every_case():
    from recgraph_amd import api
    t0 = time.perf_counter()
    worst = (0, None)
    scores = R.default_scores(0, -1)
    for cid, case in KE.CASES.items():
        g, batches = KE.build(case)
        assert [max(len(r) for r in b) for b in batches] == case.batches and all(len(b[-1]) == 1 for b in batches), cid
        assert all(len(b[0]) == hi for b, hi in zip(batches, case.batches)), cid
        lnz, rows = R.graph_paths(api.Graph.from_gfa_text(g.gfa()))
        cells = KE.rule_cells(rows, batches)
        worst = max(worst, (cells, cid))
        assert cells <= KE.CELL_CAP, (cid, cells)
        for reads in batches:
            for rd in reads:
                res = R.align(lnz, rows, rd, scores, 0, -1, case.mode == 45)
                assert len(res[3]) >= len(rd) and res[0] <= 0, cid
    print("edit kernel matrix: %d cases, rule wall time %.1f s, largest case %s at %.2e cells" % (len(KE.CASES), time.perf_counter() - t0, worst[1], worst[0]))
