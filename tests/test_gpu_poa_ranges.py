"""POA kernels at their ranges, on the GPU against the oracle: the f32 range of -m 0 SIMD / AVX2 -m 1, reads past the
16 000-base LDS cut, band widths at the 64-column chunk edges and at the 256-column register limit of `k_m0_simd`, and
the regrowth of the band arena."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _compare(oracle, gfa, reads, mode, omode, scores=None, stats=None, **kw):
    """Byte-identical text and the same Batch.score(i) as the oracle for every read; returns the scores (stats: a dict that
    receives the batch's kernel_stats())."""
    from recgraph_amd import api
    og = oracle.Graph.from_gfa_text(gfa, want_path=False)
    g = api.Graph.from_gfa_text(gfa)
    b = api.Batch(g, reads, api.make_params(mode, score_matrix=scores, **kw))
    b.run()
    b.fetch()
    if stats is not None:
        stats.update(b.kernel_stats())
    bad, out = [], []
    for i, rd in enumerate(reads):
        name = "r%d" % i
        exp, score, panic, _ = og.align(omode, rd, name=name, idx=i + 1, scores=scores, **kw)
        out.append(score)
        if panic:
            if not b.status(i) & api.READ_WOULD_PANIC:
                bad.append((i, "expected the panic status", b.status(i)))
            continue
        got = b.gaf_text(i, name, i + 1)
        if got != exp or b.score(i) != score:
            bad.append((i, len(rd), b.score(i), score, got[-300:], exp[-300:]))
    assert not bad, (len(bad), bad[:2])
    return out


# ---- f32 range -------------------------------------------------------------------------------------------------------------
# The reference computes -m 0 (exec_simd) and AVX2 -m 1 in f32, the kernels in int32.  rg_batch_create refuses a batch whose
# f32 values could reach 2^24 in magnitude: |value| <= 2 W G + (L + W) E for -m 0 (min_score = 2 W g(read[1], '-') of the
# cells outside the band, global_abpoa.rs:20, plus one alignment path), (L + W) E for -m 1 (cells start from 0), with
# W = longest read + 1, E = max |entry|, G = max |(b, '-')|.
def _f32_case():
    """(gfa, walk) of test_oracle_golden.f32_chain: a 2 478-row chain whose 2 476-base walk scores 17 334 476 at 7001."""
    from test_oracle_golden import f32_chain
    return f32_chain()


def _largest_admitted(mode, L, W):
    from recgraph_amd import api
    per_unit = (3 * W + L) if mode == api.MODE_GLOBAL_POA else (L + W)     # scores_match_mis(x, -x, f32): E = G = x
    return ((1 << 24) - 1) // per_unit


def test_f32_bound_inside_exact_outside_refused(oracle):
    from recgraph_amd import _lib, api
    gfa, walk = _f32_case()
    L, W = api.Graph.from_gfa_text(gfa).rows, len(walk) + 1
    reads = [walk, walk[:300], walk[1000:1700]]
    for mode, omode in ((api.MODE_GLOBAL_POA, oracle.M0_SIMD), (api.MODE_LOCAL_POA, oracle.M1_SIMD)):
        x = _largest_admitted(mode, L, W)
        assert 1000 < x < 7001
        # just inside: the reference's f32 is exact there, and so is the kernel
        sc = oracle.scores_match_mis(x, -x, f32_variant=True)
        _compare(oracle, gfa, reads, mode, omode, scores=sc, bta=50)
        # just outside, and the measured case where the reference rounds (7001: 17 334 396 for the exact 17 334 476): refused
        for y in (x + 1, 7001):
            with pytest.raises(_lib.RecGraphError) as e:
                api.Batch(api.Graph.from_gfa_text(gfa), reads, api.make_params(mode, score_matrix=oracle.scores_match_mis(y, -y, True), bta=50))
            assert e.value.code == -5 and "2^24" in str(e.value)
        # the longest read of the batch sets W wherever it stands
        with pytest.raises(_lib.RecGraphError):
            api.Batch(api.Graph.from_gfa_text(gfa), [walk[:300], walk], api.make_params(mode, score_matrix=oracle.scores_match_mis(x + 1, -x - 1, True)))


def test_i32_modes_are_not_refused_at_the_same_inputs(oracle):
    """-m 0 scalar, -m 1 scalar, -m 2 and -m 3 compute in i32 in the reference: the 7001 case runs there, exactly."""
    from recgraph_amd import api
    gfa, walk = _f32_case()
    sc = oracle.scores_match_mis(7001, -7001, f32_variant=True)
    reads = [walk, walk[:300]]
    for mode, omode, kw in ((api.MODE_GLOBAL_POA_SCALAR, oracle.M0_SCALAR, {"bta": 50}), (api.MODE_GAP_POA, oracle.M2, {"bta": 50}),
                            (api.MODE_LOCAL_POA_SCALAR, oracle.M1_SCALAR, {}), (api.MODE_GAP_LOCAL_POA, oracle.M3, {})):
        assert _compare(oracle, gfa, reads, mode, omode, scores=sc, **kw)[0] == 17334476


def test_realistic_inputs_are_admitted():
    """HOXD70 with 16 kbp reads on a graph of ~16 k rows, and the default matrices with reads of 200 kbp."""
    from recgraph_amd import api, synth
    sg = synth.linear_graph(16000, seed=5)
    g = api.Graph.from_gfa_text(sg.gfa())
    walk = sg.path_sequence(0)
    hox = api.create_score_matrix_i32(matrix_file_path=os.path.join(HERE, "golden", "HOXD70.mtx"))
    long_read = (walk * 13)[:200000]
    for mode in (api.MODE_GLOBAL_POA, api.MODE_LOCAL_POA):
        api.Batch(g, [walk[:16000], walk[:500]], api.make_params(mode, score_matrix=hox))
        api.Batch(g, [long_read, walk[:500]], api.make_params(mode))                                       # (2, -4), gaps -8
        api.Batch(g, [long_read], api.make_params(mode, score_matrix=api._score_matrix_match_mis_f32(2, -4)))  # the CLI's f32 matrix


# ---- reads past the LDS cut ------------------------------------------------------------------------------------------------
# lds_read = max_n <= 16000 (rg_poa_driver.hip): a batch whose longest read has 16 000 bases runs the LDS variants of all three POA
# kernels, one with a longer read the variants that read the bases from global memory.
def _long_reads(walk, n, rng):
    tail = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n - len(walk)))
    return walk + tail


@pytest.mark.parametrize("longest", [16000, 16001, 16400])
def test_reads_past_the_lds_cut_every_poa_mode(oracle, longest):
    from recgraph_amd import api, synth
    rng = np.random.default_rng(longest)
    sg = synth.linear_graph(1200, seed=13)
    walk = sg.path_sequence(0)
    reads = [_long_reads(walk, longest, rng), walk, walk[:64], walk[200:329], "ACGTN"]
    if longest > 16001:
        reads.insert(2, _long_reads(walk[:900], 16001, rng))
    modes = ((api.MODE_GLOBAL_POA, oracle.M0_SIMD, {"bta": 2000}), (api.MODE_GLOBAL_POA_SCALAR, oracle.M0_SCALAR, {"bta": 2000}),
             (api.MODE_GAP_POA, oracle.M2, {"bta": 2000, "o": -4, "e": -2}), (api.MODE_LOCAL_POA, oracle.M1_SIMD, {}),
             (api.MODE_LOCAL_POA_SCALAR, oracle.M1_SCALAR, {}), (api.MODE_GAP_LOCAL_POA, oracle.M3, {"o": -6, "e": -1}))
    for mode, omode, kw in modes:
        _compare(oracle, sg.gfa(), reads, mode, omode, **kw)


# ---- band widths at the chunk edges and at the register limit; arena regrowth ------------------------------------------------
# An inner row that follows the diagonal has the band [ms - bta, me + bta): 2 bta columns (band_plain); band_simd widens it to a
# multiple of 8.  bta 29..33, 61..65 and 125..132 put the widths on 58-66, 122-130 and 250-264 columns: both sides of the
# 64- and 128-column chunk edges and of the 256 columns up to which k_m0_simd keeps the row above in registers.
BTAS = list(range(29, 34)) + list(range(61, 66)) + list(range(125, 133))


def test_band_widths_at_chunk_edges_and_register_limit(oracle):
    from recgraph_amd import api, synth
    rng = np.random.default_rng(5)
    for sg in (synth.linear_graph(800, seed=17), synth.haplotype_graph(800, 4, path_len=700, seed=18)):
        walk = sg.path_sequence(0)
        reads = synth.full_walk_reads(sg, 4, seed=int(rng.integers(1, 1000))) + [walk[:600], walk[:640]]
        assert min(len(r) for r in reads) >= 600
        for bta in BTAS:
            for mode, omode in ((api.MODE_GLOBAL_POA, oracle.M0_SIMD), (api.MODE_GLOBAL_POA_SCALAR, oracle.M0_SCALAR),
                                (api.MODE_GAP_POA, oracle.M2)):
                _compare(oracle, sg.gfa(), reads, mode, omode, bta=bta)


KERNEL = {0: "k_m0_simd", 10: "k_m0_scalar", 2: "k_m2_gap", 1: "k_m1_local_simd", 11: "k_m1_local_scalar", 3: "k_m3_gap_local"}   # by api.MODE_*


def test_band_arena_regrowth(oracle, capfd):
    """Reads 200 bases longer than a linear graph with a small bta: their bands are ~200 columns wider than the first arena
    (L * (2 bta + 40) cells per read), the first attempt overflows and run_poa runs again with a doubled arena."""
    from recgraph_amd import api, synth
    rng = np.random.default_rng(9)
    sg = synth.linear_graph(400, seed=19)
    walk = sg.path_sequence(0)
    reads = [walk + "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=200)) for _ in range(3)] + [walk[:100]]
    api.set_option("debug", 1)
    try:
        for mode, omode in ((api.MODE_GLOBAL_POA, oracle.M0_SIMD), (api.MODE_GLOBAL_POA_SCALAR, oracle.M0_SCALAR), (api.MODE_GAP_POA, oracle.M2)):
            capfd.readouterr()
            stats = {}
            _compare(oracle, sg.gfa(), reads, mode, omode, stats=stats, bta=4)
            err = capfd.readouterr().err
            assert "run_poa attempt 0" in err and "run_poa attempt 1" in err, (mode, err[-600:])
            # the statistics are those of the last attempt alone (one launch of the four reads), and the launch log is off
            assert stats[KERNEL[mode]][1] == 1 and not [k for k in stats if k.startswith("inst:")], (mode, stats)
    finally:
        api.set_option("debug", 0)


# ---- launches behind the first: read_base > 0 ----------------------------------------------------------------------------------
# A POA batch goes through as many launches as the free HBM asks for, which is one below full-size batches; "chunk_reads" caps
# the reads of a launch, so 5 reads at chunk_reads = 2 are 3 launches (2, 2, 1) with read_base 0, 2, 4 and launch-relative arena
# slots.  Rows with several predecessors (a 4-path haplotype graph), reads of different lengths, one with a bad base.
def test_poa_launches_with_a_read_base(oracle):
    from recgraph_amd import api, synth
    assert {getattr(api, n) for n in ("MODE_GLOBAL_POA", "MODE_GLOBAL_POA_SCALAR", "MODE_GAP_POA", "MODE_LOCAL_POA", "MODE_LOCAL_POA_SCALAR",
                                      "MODE_GAP_LOCAL_POA")} == set(KERNEL)
    sg = synth.haplotype_graph(300, 4, path_len=250, seed=23)
    gfa = sg.gfa()
    w = [sg.path_sequence(k) for k in range(4)]
    assert min(len(x) for x in w) >= 200
    reads = [w[0][:250], w[1][20:80], w[2][:90] + "X" + w[2][91:180], w[3][40:160], w[1][:97]]
    assert sorted(len(r) for r in reads) == [60, 97, 120, 180, min(250, len(w[0]))]
    og = oracle.Graph.from_gfa_text(gfa, want_path=False)
    g = api.Graph.from_gfa_text(gfa)
    modes = ((api.MODE_GLOBAL_POA, oracle.M0_SIMD, {"bta": 30}), (api.MODE_GLOBAL_POA_SCALAR, oracle.M0_SCALAR, {"bta": 30}),
             (api.MODE_GAP_POA, oracle.M2, {"bta": 30, "o": -4, "e": -2}), (api.MODE_LOCAL_POA, oracle.M1_SIMD, {}),
             (api.MODE_LOCAL_POA_SCALAR, oracle.M1_SCALAR, {}), (api.MODE_GAP_LOCAL_POA, oracle.M3, {"o": -6, "e": -1}))
    try:
        api.set_option("launch_log", 1)
        for mode, omode, kw in modes:
            exp = [og.align(omode, rd, name="r%d" % i, idx=i + 1, **kw) for i, rd in enumerate(reads)]
            assert [bool(e[2]) for e in exp] == [False, False, True, False, False]        # the oracle refuses the bad base alone
            runs = []
            for cap, launches in ((2, 3), (0, 1)):
                api.set_option("chunk_reads", cap)
                b = api.Batch(g, reads, api.make_params(mode, **kw))
                b.run()
                b.fetch()
                texts = [b.gaf_text(i, "r%d" % i, i + 1) for i in range(len(reads))]
                for i, (text, score, panic, _) in enumerate(exp):
                    if panic:
                        assert b.status(i) & api.READ_BAD_BASE and texts[i] == "", (mode, cap, i)
                    else:
                        assert texts[i] == text and b.score(i) == score, (mode, cap, i, texts[i][-300:], text[-300:])
                st = b.kernel_stats()
                inst = {k: v[1] for k, v in st.items() if k.startswith("inst:")}
                assert st[KERNEL[mode]][1] == launches and list(inst.values()) == [launches], (mode, cap, st)
                runs.append((texts, b.cell_updates))
            assert runs[0] == runs[1], mode
    finally:
        api.set_option("chunk_reads", 0)
        api.set_option("launch_log", 0)
