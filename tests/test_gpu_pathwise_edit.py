"""-m 44 / -m 45 (modes 16 / 17 restricted to unit costs, on the bit-vector kernels of edit/rg_path_edit.hip) on the GPU.

Expected lines come from the numpy rule of modes 6 / 7 at unit costs, pathwise_gap_rule.line(..., default_scores(0, -1), 0, -1, semi),
through check_long of tests/test_gpu_pathwise_gap_long.py (whole line, re-scored CIGAR, status).  Where the rule would be slow — long
reads on long paths — the test is identity with mode 16 / 17 on the same rg_params: texts, statuses, scores and both cell counters."""
import functools

import numpy as np
import pytest

import kernel_matrix_edit as KE
import pathwise_gap_rule as R
from test_gpu_pathwise_gap_long import _graph, _noisy, _of_length, _rand, check_long

pytestmark = pytest.mark.gpu
EDIT = (44, 45)
BASE = {44: 16, 45: 17}
EDIT_KERNELS = {"k_edit_score", "k_gap_pick", "k_edit_dirs", "k_edit_trace"}


def _unit():
    from recgraph_amd import api
    return api.create_score_matrix_i32(0, -1)


def _run(gg, reads, mode, scores=None):
    """(texts, statuses, scores, counted cells, performed cells), kernel statistics of one batch at unit costs."""
    from recgraph_amd import api
    b = api.Batch(gg, reads, api.make_params(mode, score_matrix=_unit() if scores is None else scores, o=0, e=-1))
    b.run()
    b.fetch()
    n = len(reads)
    return ([b.gaf_text(i, "r%d" % i, i + 1) for i in range(n)], [b.status(i) for i in range(n)], [b.score(i) for i in range(n)],
            b.cell_updates, b.cell_updates_performed), b.kernel_stats()


def check_edit(graph, reads, mode, scores=None, out=None):
    """Every read against the rule of mode 16 / 17 at unit costs; returns the batch's results."""
    if out is None:
        out = _run(graph[1], reads, mode, scores)[0]
    check_long(graph, reads, BASE[mode], scores=_unit() if scores is None else scores, o=0, e=-1, texts=out[0], status=out[1])
    return out


def identical(gg, reads, mode, scores=None):
    """Mode 44 / 45 and mode 16 / 17 on the same parameters: bytes, statuses, scores and both counters; returns them."""
    got, ks = _run(gg, reads, mode, scores)
    exp, _ = _run(gg, reads, BASE[mode], scores)
    for name, a, b in zip(("texts", "statuses", "scores", "counted cells", "performed cells"), got, exp):
        assert a == b, (mode, name, [i for i in range(len(reads)) if isinstance(a, list) and a[i] != b[i]][:5], a if not isinstance(a, list) else None, b if not isinstance(b, list) else None)
    assert {k for k in ks if k.startswith("k_")} == EDIT_KERNELS, sorted(ks)
    return got


@functools.lru_cache(maxsize=None)
def _bubble_graph(alphabet, n_paths, seed, blocks=9, seg=12):
    """(SynthGraph, api.Graph, lnz, rows, node ids) of shared segments with two-allele bubbles between them over `alphabet`: at most
    300 rows."""
    from recgraph_amd import api, synth
    rng = np.random.default_rng(seed)
    segments, links, paths = [], set(), [[] for _ in range(n_paths)]

    def add(k):
        segments.append((len(segments) + 1, _rand(rng, k, alphabet)))
        return len(segments)
    for b in range(blocks):
        s = add(seg)
        for p in paths:
            if p:
                links.add((p[-1], s))
            p.append(s)
        if b == blocks - 1:
            break
        alleles = [add(int(rng.integers(1, seg))) for _ in range(2)]
        for k, p in enumerate(paths):
            a = alleles[(k + (k >> 1) * b) % 2]
            links.add((s, a))
            p.append(a)
    g = synth.SynthGraph(segments, sorted(links), paths)
    assert g.rows <= 300
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    return g, gg, lnz, rows, R.graph_node_ids(gg)


def _small_reads(g, alphabet, seed):
    rng = np.random.default_rng(seed)
    w = [g.path_sequence(k) for k in range(len(g.paths))]
    sub = lambda s: "".join(c if rng.random() > 0.08 else alphabet[int(rng.integers(0, len(alphabet)))] for c in s)
    reads = [w[0][3], w[1][:31], w[2][:32], sub(w[0][:33]), sub(w[1]), w[2][20:90], sub(w[0])[:63] + sub(w[0])[70:], _rand(rng, 64, alphabet),
             _rand(rng, 20, alphabet) + w[1][30:] + _rand(rng, 40, alphabet), (sub(w[2]) + _rand(rng, 300, alphabet))[:300], alphabet[0] * 65]
    assert all(1 <= len(r) <= 300 for r in reads)
    return reads


@pytest.mark.parametrize("alphabet,n_paths", [("ACGT", 3), ("AC", 6), ("ACGTN", 4)])
@pytest.mark.parametrize("mode", EDIT)
def test_small_graphs_against_the_rule(mode, alphabet, n_paths):
    graph = _bubble_graph(alphabet, n_paths, 7 * n_paths)
    reads = _small_reads(graph[0], alphabet, 100 + n_paths)
    out = check_edit(graph, reads, mode)
    assert all(s <= 0 for s in out[2])
    identical(graph[1], reads, mode)


@pytest.mark.parametrize("mode", EDIT)
def test_mixed_batch_is_mode_16_or_17(mode):
    """Every word, lane and width edge in ONE batch (W = 4) on paths of about 2200 rows: the bytes, statuses, scores and counters of
    mode 16 / 17."""
    g, gg = _graph(2200)[:2]
    rng = np.random.default_rng(mode)
    lengths = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4096, 4097]
    reads = [_of_length(rng, g.path_sequence(i % 2)[(7 * i) % 50:], n) for i, n in enumerate(lengths)]
    assert [len(r) for r in reads] == lengths
    identical(gg, reads, mode)


@functools.lru_cache(maxsize=None)
def _homopolymer_graph(n):
    from recgraph_amd import api, synth
    g = synth.SynthGraph([(1, "A" * 1000), (2, "A" * (n - 1000))], [(1, 2)], [[1, 2], [1, 2]])
    return api.Graph.from_gfa_text(g.gfa())


@pytest.mark.parametrize("n", [2048, 2049, 4097])
@pytest.mark.parametrize("mode", EDIT)
def test_homopolymer_carry(mode, n):
    """A^n against a linear path A^n: Eq and Pv are all ones, so the carry of the wide addition ripples through every word of every lane
    that holds the read; one C at the last bit of a lane's chunk and at the first bit of the next one's stops and restarts it."""
    gg = _homopolymer_graph(n)
    w = 1 if n <= 2048 else 2 if n <= 4096 else 4
    last = (n - 1) // (32 * w)
    reads = ["A" * n]
    for lane in sorted({last // 2, last, min(63, last)}):
        for t in (32 * w * lane - 1, 32 * w * lane):
            if 0 <= t < n:
                reads.append("A" * t + "C" + "A" * (n - t - 1))
    assert len(reads) >= 4 and all(len(r) == n for r in reads)
    got = identical(gg, reads, mode)
    assert got[2] == [0] + [-1] * (len(reads) - 1) and got[0][0].split("\t")[12].startswith("%dM," % n)


@pytest.mark.parametrize("n", [1, 32, 33, 2048, 4096])
@pytest.mark.parametrize("mode", EDIT)
def test_the_score_bit_at_a_word_a_lane_and_a_wave_edge(mode, n):
    graph = _graph(300, 3)
    rng = np.random.default_rng(n)
    rd = _of_length(rng, graph[0].path_sequence(n % 3), n)
    check_edit(graph, [rd, rd[:-1] + ("A" if rd[-1] != "A" else "C")], mode)


def test_a_repeat_rich_path_ties_between_rows_and_between_paths():
    """ACAC...: in mode 45 every other row attains the best value, on two paths that spell the same bases — the first row and the lowest
    path win; mode 44 ties between the paths."""
    from recgraph_amd import api, synth
    g = synth.SynthGraph([(1, "AC" * 20), (2, "AC" * 5), (3, "AC" * 5), (4, "AC" * 30)], [(1, 2), (1, 3), (2, 4), (3, 4)], [[1, 3, 4], [1, 2, 4], [1, 3, 4]])
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    graph = (g, gg, lnz, rows, R.graph_node_ids(gg))
    reads = ["ACACAC", "CACA", "AC" * 55, "ACACGACAC", "A", "C", "ACAACAC", "AC" * 20 + "CA" * 20]
    for mode in EDIT:
        out = check_edit(graph, reads, mode)
        assert all("best path: 0," in t for t in out[0])
        identical(gg, reads, mode)
    assert out[2][:3] == [0, 0, 0] and out[0][0].split("\t")[12].startswith("6M,")


@pytest.mark.parametrize("n_paths", [65, 256])
def test_many_paths(n_paths):
    from recgraph_amd import api, synth
    g = synth.random_dag_graph(60, n_paths, seed=100 + n_paths)
    g.paths[n_paths - 1] = list(g.paths[3])
    used = {i for p in g.paths for i in p}
    g = synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths)
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    graph = (g, gg, lnz, rows, R.graph_node_ids(gg))
    rng = np.random.default_rng(n_paths)
    w = g.path_sequence(n_paths - 1)
    reads = [w, _rand(rng, 20) + _noisy(rng, g.path_sequence(n_paths // 2), 13) + _rand(rng, 9), w[5:40]]
    for mode in EDIT:
        out = check_edit(graph, reads, mode)
        identical(gg, reads, mode)
    seqs = [g.path_sequence(q) for q in range(n_paths)]
    assert "best path: %d," % seqs.index(w) in out[0][0] and seqs.index(w) < n_paths - 1       # the lowest of the identical paths


@pytest.mark.parametrize("mode", EDIT)
def test_the_longest_read(mode):
    """One 16383-base read (W = 8, every bit of the wave but the last) on two paths of about 1000 rows: mode 16 / 17, with half its
    direction buffer."""
    g, gg = _graph(1000)[:2]
    rng = np.random.default_rng(16383)
    w = g.path_sequence(1)
    rd = _rand(rng, 7000) + _noisy(rng, w) + _rand(rng, 16383 - 7000 - len(w))
    assert len(rd) == 16383
    got, ks = _run(gg, [rd], mode)
    exp, ks16 = _run(gg, [rd], BASE[mode])
    assert got == exp and got[1] == [0]
    assert ks["mem:work_bytes_per_read"][0] < 0.55 * ks16["mem:work_bytes_per_read"][0]


@pytest.mark.parametrize("mode", EDIT)
def test_a_bad_base_in_the_middle_of_a_batch(mode):
    from recgraph_amd import api
    graph = _graph(300, 3)
    g, gg, lnz, rows, _ = graph
    rng = np.random.default_rng(8 + mode)
    w = g.path_sequence(0)
    long_rd = _rand(rng, 1000) + _noisy(rng, w) + _rand(rng, 2500 - 1000 - len(w))
    reads = [long_rd, long_rd[:2200] + "?" + long_rd[2201:], w[10:200]]
    got = identical(gg, reads, mode)
    assert got[1] == [0, api.READ_BAD_BASE, 0] and got[0][1] == ""
    check_edit(graph, [reads[0], reads[2]], mode, out=([got[0][0], got[0][2].replace("r2\t", "r1\t", 1)], [0, 0]))
    # rows_k * n over the paths and the two clean reads; the direction pass adds the rows of the picked path (mode 45: up to the end row) times n
    counted = sum(len(r) for r in rows) * (len(reads[0]) + len(reads[2]))
    performed = counted
    for i in (0, 2):
        _, k, end_row = R.align(lnz, rows, reads[i], R.default_scores(0, -1), 0, -1, mode == 45)[:3]
        performed += (rows[k].index(end_row) + 1 if mode == 45 else len(rows[k])) * len(reads[i])
    assert (got[3], got[4]) == (counted, performed)


@pytest.mark.parametrize("mode", EDIT)
def test_a_custom_table_in_which_n_matches_n(mode):
    graph = _bubble_graph("ACGTN", 4, 28)
    sc = dict(_unit())
    sc[("N", "N")] = 0
    sc[("A", "G")] = 0                               # and a transition that costs nothing one way
    reads = _small_reads(graph[0], "ACGTN", 45) + ["N" * 40, "NANGN"]
    out = check_edit(graph, reads, mode, scores=sc)
    identical(graph[1], reads, mode, scores=sc)
    plain = _run(graph[1], reads, mode)[0]
    assert out[2] != plain[2] and all(a >= b for a, b in zip(out[2], plain[2]))


def test_stream_multi_wrapper_and_cli_give_the_batch_text(tmp_path, capsys):
    from recgraph_amd import api, cli
    graph = _graph(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(44)
    reads = [_rand(rng, 7) + g.path_sequence(i % 3)[5: 25 + 20 * i] + _rand(rng, i) for i in range(6)]
    reads += [_rand(rng, 1500) + _noisy(rng, g.path_sequence(1)) + _rand(rng, 700), "NNNN", _rand(rng, 2060) + g.path_sequence(2)[30:230]]
    names = ["r%d" % i for i in range(len(reads))]
    for mode in EDIT:
        texts, status = check_edit(graph, reads, mode)[:2]
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4, score_matrix=_unit(), o=0, e=-1)
        assert [x.decode() if isinstance(x, bytes) else x for x in st] == texts and list(sstatus) == status
    mt, mstatus = api.align_batch_multi(gg, reads, names, mode=45, device_ids=[0], score_matrix=_unit(), o=0, e=-1)
    assert mt == texts and mstatus == status
    rd = reads[6]
    for semi in (False, True):
        line = api.pathwise_alignment_edit_exec(["$"] + list(rd), gg, semi=semi).to_string()
        assert line == _run(gg, [rd], 45 if semi else 44)[0][0][0].replace("r0\t", "Temp\t", 1).rstrip("\n")
    with pytest.raises(api._lib.RecGraphError):
        api.pathwise_alignment_edit_exec(["$"] + list(rd), gg, score_matrix=api.create_score_matrix_i32(2, -4))
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "45", "-M", "0", "-X", "1", "-O", "0", "-E", "1", "--devices", "0"])
    assert capsys.readouterr().out == "".join(texts)


def run_matrix_case(cid, results):
    """One case of tests/kernel_matrix_edit.py with the launch log on, cached in `results`: every read checked against the rule; returns
    (the instantiations each batch launched, the coarse kernel names of all batches)."""
    if cid in results:
        return results[cid]
    from recgraph_amd import api
    case = KE.CASES[cid]
    g, batches = KE.build(case)
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    graph = (g, gg, lnz, rows, R.graph_node_ids(gg))
    per_batch, coarse = [], set()
    try:
        for reads in batches:
            api.set_option("launch_log", 1)
            out, stats = _run(gg, reads, case.mode)
            api.set_option("launch_log", 0)
            assert out[1] == [0] * len(reads), cid
            per_batch.append({k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")})
            coarse |= {k for k in stats if k.startswith("k_")}
            check_edit(graph, reads, case.mode, out=out)
    finally:
        api.set_option("launch_log", 0)
    results[cid] = (per_batch, coarse)
    return results[cid]
