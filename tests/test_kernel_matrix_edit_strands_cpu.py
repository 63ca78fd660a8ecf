"""CPU: tests/kernel_matrix_edit_strands.py is complete and the rule answers every case of it.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/edit_strands/rg_edit_strands.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no other
file of that directory may hold a kernel without a matrix."""
import time

import kernel_matrix_edit_strands as KS
import kernel_matrix_gap_long as KG
import pathwise_gap_rule as R
import strand_vote_rule as V
from edit_strands_support import instantiations, pair_words
from kernel_matrix_checks import assert_matrix_is_complete


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert_matrix_is_complete(KS, "edit_strands/rg_edit_strands.hip", 11)


def test_every_entry_names_a_case_and_every_width_is_reached_from_both_sides():
    assert set(KS.MATRIX.values()) == set(KS.CASES)
    assert {c.mode for c in KS.CASES.values()} == {64, 65} and {c.words for c in KS.CASES.values()} == {1, 2, 4, 8, 16}
    for cid, case in KS.CASES.items():
        lo, hi = case.batches
        # the plan's rule: the smallest W with longest read <= 1024 W
        assert hi <= 1024 * case.words and (hi == 1024 * case.words or hi == 16383), cid
        assert lo == (1024 * case.words // 2 + 1 if case.words > 1 else 1), cid
        assert pair_words(lo) == pair_words(hi) == case.words, cid
    for name, cid in KS.MATRIX.items():
        case = KS.CASES[cid]
        assert all(name in instantiations(case.mode, n) for n in case.batches), (name, cid)
    assert KS.CELL_CAP == KG.CELL_CAP


def test_the_rule_answers_every_case_and_both_strands_win():
    from recgraph_amd import api
    t0 = time.perf_counter()
    worst = (0, None)
    scores = R.default_scores(0, -1)
    for cid, case in KS.CASES.items():
        g, batches = KS.build(case)
        assert [max(len(r) for r in b) for b in batches] == case.batches and all(len(b[-1]) == 1 for b in batches), cid
        assert all(len(b[0]) == hi for b, hi in zip(batches, case.batches)), cid
        lnz, rows = R.graph_paths(api.Graph.from_gfa_text(g.gfa()))
        cells = KS.rule_cells(rows, batches)
        worst = max(worst, (cells, cid))
        assert cells <= KS.CELL_CAP, (cid, cells)
        # the long read of the second batch and the piece of the first are given on the reverse strand, and win there
        for bi, reads in enumerate(batches):
            if len(reads) < 3:
                continue
            fwd, rev = reads[1 if bi else 0], reads[0 if bi else 1]
            f = [R.align(lnz, rows, s, scores, 0, -1, case.mode == 65)[0] for s in (rev, V.rc(rev))]
            assert f[1] > f[0], (cid, bi, f)
            f = [R.align(lnz, rows, s, scores, 0, -1, case.mode == 65)[0] for s in (fwd, V.rc(fwd))]
            assert f[0] > f[1], (cid, bi, f)
    print("edit strands kernel matrix: %d cases, rule wall time %.1f s, largest case %s at %.2e cells" % (len(KS.CASES), time.perf_counter() - t0, worst[1], worst[0]))
