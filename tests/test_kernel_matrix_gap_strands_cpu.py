"""CPU: tests/kernel_matrix_gap_strands.py is complete and the composed rule answers its case.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/gap_strands/rg_gap_strands.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no
other file of that directory may hold a kernel without a matrix."""
import time

import kernel_matrix_gap_strands as KS
import pathwise_gap_rule as R
import pathwise_gap_strands_rule as S
from kernel_matrix_checks import assert_matrix_is_complete


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert_matrix_is_complete(KS, "gap_strands/rg_gap_strands.hip", 1)


def test_every_entry_names_a_case():
    assert set(KS.MATRIX.values()) == set(KS.CASES)
    assert {c.mode for c in KS.CASES.values()} == {32}


def test_the_rule_answers_the_case():
    from recgraph_amd import api
    t0 = time.perf_counter()
    for cid, case in KS.CASES.items():
        g, batches = KS.build(case)
        assert [len(b) for b in batches] == case.batches and case.batches[0] > 256 and case.batches[0] % 256, cid
        assert max(len(r) for r in batches[0]) <= 2047 < max(len(r) for r in batches[1]) == 2100, cid
        gg = api.Graph.from_gfa_text(g.gfa())
        lnz, rows = R.graph_paths(gg)
        node_ids = R.graph_node_ids(gg)
        cells = KS.rule_cells(rows, batches)
        assert cells <= KS.CELL_CAP, (cid, cells)
        exps = []
        for reads in batches:
            exp = [S.expected(case.mode, rd, S.line_fn(case.mode, lnz, rows, node_ids, "r%d" % i)) for i, rd in enumerate(reads)]
            # both strands win somewhere, and reads without a record (bad base: no pass at all; N only: unaligned both ways) sit among them
            assert {e[2] for e in exp} == {"+", "-", " "}, cid
            assert S.READ_UNALIGNED in {e[1] for e in exp}, cid
            assert all(e[3] == ["+", "-"] for e in exp if e[1] != S.READ_BAD_BASE), cid
            exps.append(exp)
        big = exps[0]
        assert any(e[1] == S.READ_BAD_BASE for e in big[:256]) and any(e[1] == S.READ_BAD_BASE for e in big[256:]), cid
        assert exps[1][1][2] == "-", cid            # the 2100-base read is chosen on the reverse strand: the merge moves its record
    print("gap strands kernel matrix: %d case, rule wall time %.1f s, %.2e cells" % (len(KS.CASES), time.perf_counter() - t0, cells))
