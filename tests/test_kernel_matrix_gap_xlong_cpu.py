"""CPU: tests/kernel_matrix_gap_xlong.py is complete and the rules answer every case of it.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/gap_xlong/rg_path_gap_xlong.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no other
file of that directory may hold a kernel without a matrix."""
import time

import kernel_matrix_gap_xlong as KX
import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
from kernel_matrix_checks import assert_matrix_is_complete


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert_matrix_is_complete(KX, "gap_xlong/rg_path_gap_xlong.hip", 8)


def test_every_entry_names_a_case():
    assert set(KX.MATRIX.values()) == set(KX.CASES)
    assert {n for c in KX.CASES.values() for n in c.batches} == {2048, 16384}
    assert {c.mode for c in KX.CASES.values()} == {56, 57, 62}
    for name, cid in KX.MATRIX.items():
        mode = KX.CASES[cid].mode
        assert "<%d>" % (0, 1, 2)[(56, 57, 62).index(mode)] in name or name == KX.WALK[mode], (name, cid)


def test_the_rule_answers_every_case():
    from recgraph_amd import api
    t0 = time.perf_counter()
    worst = (0, None)
    for cid, case in KX.CASES.items():
        g, batches = KX.build(case)
        assert [max(len(r) for r in b) for b in batches] == case.batches and all(len(b[-1]) == 1 for b in batches), cid
        assert all(len(b[0]) == hi for b, hi in zip(batches, case.batches)), cid
        lnz, rows = R.graph_paths(api.Graph.from_gfa_text(g.gfa()))
        cells = KX.rule_cells(rows, batches)
        worst = max(worst, (cells, cid))
        assert cells <= KX.CELL_CAP, (cid, cells)
        assert max(len(r) for r in rows) * (max(case.batches) + 1) <= KX.ROW_CAP, cid
        o, e = case.kw.get("o", -4), case.kw.get("e", -2)
        for reads in batches:
            for rd in reads:
                if case.mode == 62:
                    res = L.align_local(lnz, rows, rd, None, o, e)
                    assert res is not None and res[0] > 0, cid
                else:
                    res = R.align(lnz, rows, rd, None, o, e, case.mode == 57)
                    assert len(res[3]) >= len(rd), cid
            if case.mode == 62:
                # the flanked read is clipped on the left, and its alignment ends beyond the first stripe boundary
                score, k, end_row, end_col, stop_col, ops, pseq = L.align_local(lnz, rows, reads[0], None, o, e)
                assert stop_col > 0 and 2048 <= end_col <= len(reads[0]), (cid, stop_col, end_col)
    print("xlong gap kernel matrix: %d cases, rule wall time %.1f s, largest case %s at %.2e cells" % (len(KX.CASES), time.perf_counter() - t0, worst[1], worst[0]))
