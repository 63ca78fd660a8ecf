"""CPU: tests/kernel_matrix_gap_xstrands.py is complete and the composed rule answers its cases.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/gap_xstrands/rg_gap_xstrands.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no
other file of that directory may hold a kernel without a matrix."""
import time

import kernel_matrix_gap_xstrands as KX
import pathwise_gap_rule as R
import pathwise_gap_xstrands_rule as X
from kernel_matrix_checks import assert_matrix_is_complete


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert_matrix_is_complete(KX, "gap_xstrands/rg_gap_xstrands.hip", 4)


def test_every_entry_names_a_case():
    assert set(KX.MATRIX.values()) == set(KX.CASES)
    assert {c.mode for c in KX.CASES.values()} == {77, 82}


def test_the_rule_answers_the_cases():
    from recgraph_amd import api
    t0 = time.perf_counter()
    total = 0
    for cid, case in KX.CASES.items():
        g, batches = KX.build(case)
        assert [len(b) for b in batches] == case.batches and case.batches[0] > 256 and case.batches[0] % 256, cid
        assert max(len(r) for r in batches[0]) <= 2047 < max(len(r) for r in batches[1]) == 2100, cid
        gg = api.Graph.from_gfa_text(g.gfa())
        lnz, rows = R.graph_paths(gg)
        node_ids = R.graph_node_ids(gg)
        cells = KX.rule_cells(rows, batches)
        total += cells
        assert cells <= KX.CELL_CAP, (cid, cells)
        exps = []
        for reads in batches:
            striped = max(len(r) for r in reads) > 2047
            exp = [X.expected(case.mode, rd, lnz, rows, node_ids, "r%d" % i, striped=striped) for i, rd in enumerate(reads)]
            # both strands win somewhere, and a second pick runs for some read: every batch launches the duel
            assert {"+", "-"} <= {e["strand"] for e in exp}, cid
            assert any(len(e["picked"]) == 2 for e in exp), cid
            if case.mode == 82:
                assert X.READ_UNALIGNED in {e["status"] for e in exp}, cid
                assert all(e["picked"] == ["+", "-"] for e in exp if e["status"] != X.READ_BAD_BASE), cid
            exps.append(exp)
        big = exps[0]
        assert any(e["status"] == X.READ_BAD_BASE for e in big[:256]) and any(e["status"] == X.READ_BAD_BASE for e in big[256:]), cid
        assert any(e["strand"] == "-" for e in big[:256]) and any(e["strand"] == "-" for e in big[256:]), cid
        if case.mode == 77:
            # the gate lets only some reads through: slots and read indices differ
            assert any(e["picked"] == ["+"] for e in big) and any(e["picked"] == ["+", "-"] for e in big), cid
        assert exps[1][1]["strand"] == "-", cid            # the 2100-base read wins on the reverse strand: its trace is striped
    print("gap xstrands kernel matrix: %d cases, rule wall time %.1f s, %.2e cells" % (len(KX.CASES), time.perf_counter() - t0, total))
