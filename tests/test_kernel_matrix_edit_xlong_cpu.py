"""CPU: tests/kernel_matrix_edit_xlong.py is complete and the rule answers every case of it.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/edit_xlong/rg_path_edit_xlong.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no
other file of that directory may hold a kernel without a matrix."""
import time

import kernel_matrix_edit_xlong as KX
import kernel_matrix_gap_long as KG
import pathwise_gap_rule as R
from kernel_matrix_checks import assert_matrix_is_complete


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert_matrix_is_complete(KX, "edit_xlong/rg_path_edit_xlong.hip", 4)


def test_every_entry_names_a_case_and_both_stripe_counts_are_reached():
    assert set(KX.MATRIX.values()) == set(KX.CASES)
    assert {c.mode for c in KX.CASES.values()} == {94, 95}
    for cid, case in KX.CASES.items():
        lo, hi = case.batches
        # the plan's rule: striped from 16384 bases on, S = ceil(longest / 16384) and at least 2
        assert lo == 16384 and hi == 2 * 16384 + 1, cid
    for name, cid in KX.MATRIX.items():
        assert name in KX.instantiations(KX.CASES[cid]), (name, cid)
    assert KX.CELL_CAP == KG.CELL_CAP


def test_the_rule_answers_every_case():
    from recgraph_amd import api
    t0 = time.perf_counter()
    worst = (0, None)
    scores = R.default_scores(0, -1)
    for cid, case in KX.CASES.items():
        g, batches = KX.build(case)
        assert [max(len(r) for r in b) for b in batches] == case.batches and all(len(b[-1]) == 1 for b in batches), cid
        assert all(len(b[0]) == hi for b, hi in zip(batches, case.batches)), cid
        lnz, rows = R.graph_paths(api.Graph.from_gfa_text(g.gfa()))
        cells = KX.rule_cells(rows, batches)
        worst = max(worst, (cells, cid))
        assert cells <= KX.CELL_CAP, (cid, cells)
        # what check_reads asks of the caller's shapes
        assert max(len(r) for r in rows) * (max(case.batches) + 1) <= 12_000_000, cid
        for reads in batches:
            for rd in reads:
                res = R.align(lnz, rows, rd, scores, 0, -1, case.mode == 95)
                assert len(res[3]) >= len(rd) and res[0] <= 0, cid
    print("edit xlong kernel matrix: %d cases, rule wall time %.1f s, largest case %s at %.2e cells" % (len(KX.CASES), time.perf_counter() - t0, worst[1], worst[0]))
