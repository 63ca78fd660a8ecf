"""-m 44 / -m 45 (modes 16 / 17 restricted to unit costs, on the bit-vector kernels of edit/rg_path_edit.hip) on the GPU.

Expected lines come from the numpy rule of modes 6 / 7 at unit costs, pathwise_gap_rule.line(..., default_scores(0, -1), 0, -1, semi),
through check_reads of tests/pathwise_support.py (whole line, re-scored CIGAR, status).  Where the rule would be slow — long
reads on long paths — the test is identity with mode 16 / 17 on the same rg_params: texts, statuses, scores and both cell counters."""
import functools

import numpy as np
import pytest

import pathwise_gap_rule as R
from pathwise_support import EDIT_BASE as BASE
from pathwise_support import EDIT_KERNELS, check_edit, graph_tuple, haplotype, noisy, of_length, rand_bases, unit_costs
from pathwise_support import run_batch_unit as _run

pytestmark = pytest.mark.gpu
EDIT = (44, 45)


def identical(gg, reads, mode, scores=None):
    """Mode 44 / 45 and mode 16 / 17 on the same parameters: bytes, statuses, scores and both counters; returns them."""
    got = _run(gg, reads, mode, scores)
    exp = _run(gg, reads, BASE[mode], scores)
    for name, a, b in zip(("texts", "statuses", "scores", "counted cells", "performed cells"), got[:5], exp[:5]):
        assert a == b, (mode, name, [i for i in range(len(reads)) if isinstance(a, list) and a[i] != b[i]][:5], a if not isinstance(a, list) else None, b if not isinstance(b, list) else None)
    assert got.kernels == EDIT_KERNELS, sorted(got.stats)
    return got


@functools.lru_cache(maxsize=None)
def _bubble_graph(alphabet, n_paths, seed, blocks=9, seg=12):
    """(SynthGraph, api.Graph, lnz, rows, node ids) of shared segments with two-allele bubbles between them over `alphabet`: at most
    300 rows."""
    from recgraph_amd import synth
    rng = np.random.default_rng(seed)
    segments, links, paths = [], set(), [[] for _ in range(n_paths)]

    def add(k):
        segments.append((len(segments) + 1, rand_bases(rng, k, alphabet)))
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
    return graph_tuple(g)


def _small_reads(g, alphabet, seed):
    rng = np.random.default_rng(seed)
    w = [g.path_sequence(k) for k in range(len(g.paths))]
    sub = lambda s: "".join(c if rng.random() > 0.08 else alphabet[int(rng.integers(0, len(alphabet)))] for c in s)
    reads = [w[0][3], w[1][:31], w[2][:32], sub(w[0][:33]), sub(w[1]), w[2][20:90], sub(w[0])[:63] + sub(w[0])[70:], rand_bases(rng, 64, alphabet),
             rand_bases(rng, 20, alphabet) + w[1][30:] + rand_bases(rng, 40, alphabet), (sub(w[2]) + rand_bases(rng, 300, alphabet))[:300], alphabet[0] * 65]
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
    g, gg = haplotype(2200)[:2]
    rng = np.random.default_rng(mode)
    lengths = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4096, 4097]
    reads = [of_length(rng, g.path_sequence(i % 2)[(7 * i) % 50:], n) for i, n in enumerate(lengths)]
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
    graph = haplotype(300, 3)
    rng = np.random.default_rng(n)
    rd = of_length(rng, graph[0].path_sequence(n % 3), n)
    check_edit(graph, [rd, rd[:-1] + ("A" if rd[-1] != "A" else "C")], mode)


def test_a_repeat_rich_path_ties_between_rows_and_between_paths():
    """ACAC...: in mode 45 every other row attains the best value, on two paths that spell the same bases — the first row and the lowest
    path win; mode 44 ties between the paths."""
    from recgraph_amd import synth
    g = synth.SynthGraph([(1, "AC" * 20), (2, "AC" * 5), (3, "AC" * 5), (4, "AC" * 30)], [(1, 2), (1, 3), (2, 4), (3, 4)], [[1, 3, 4], [1, 2, 4], [1, 3, 4]])
    graph = graph_tuple(g)
    gg = graph[1]
    reads = ["ACACAC", "CACA", "AC" * 55, "ACACGACAC", "A", "C", "ACAACAC", "AC" * 20 + "CA" * 20]
    for mode in EDIT:
        out = check_edit(graph, reads, mode)
        assert all("best path: 0," in t for t in out[0])
        identical(gg, reads, mode)
    assert out[2][:3] == [0, 0, 0] and out[0][0].split("\t")[12].startswith("6M,")


@pytest.mark.parametrize("n_paths", [65, 256])
def test_many_paths(n_paths):
    from recgraph_amd import synth
    g = synth.random_dag_graph(60, n_paths, seed=100 + n_paths)
    g.paths[n_paths - 1] = list(g.paths[3])
    used = {i for p in g.paths for i in p}
    g = synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths)
    graph = graph_tuple(g)
    gg = graph[1]
    rng = np.random.default_rng(n_paths)
    w = g.path_sequence(n_paths - 1)
    reads = [w, rand_bases(rng, 20) + noisy(rng, g.path_sequence(n_paths // 2), 13) + rand_bases(rng, 9), w[5:40]]
    for mode in EDIT:
        out = check_edit(graph, reads, mode)
        identical(gg, reads, mode)
    seqs = [g.path_sequence(q) for q in range(n_paths)]
    assert "best path: %d," % seqs.index(w) in out[0][0] and seqs.index(w) < n_paths - 1       # the lowest of the identical paths


@pytest.mark.parametrize("mode", EDIT)
def test_the_longest_read(mode):
    """One 16383-base read (W = 8, every bit of the wave but the last) on two paths of about 1000 rows: mode 16 / 17, with half its
    direction buffer."""
    g, gg = haplotype(1000)[:2]
    rng = np.random.default_rng(16383)
    w = g.path_sequence(1)
    rd = rand_bases(rng, 7000) + noisy(rng, w) + rand_bases(rng, 16383 - 7000 - len(w))
    assert len(rd) == 16383
    got, exp = _run(gg, [rd], mode), _run(gg, [rd], BASE[mode])
    assert got[:5] == exp[:5] and got[1] == [0]
    assert got.stats["mem:work_bytes_per_read"][0] < 0.55 * exp.stats["mem:work_bytes_per_read"][0]


@pytest.mark.parametrize("mode", EDIT)
def test_a_bad_base_in_the_middle_of_a_batch(mode):
    from recgraph_amd import api
    graph = haplotype(300, 3)
    g, gg, lnz, rows, _ = graph
    rng = np.random.default_rng(8 + mode)
    w = g.path_sequence(0)
    long_rd = rand_bases(rng, 1000) + noisy(rng, w) + rand_bases(rng, 2500 - 1000 - len(w))
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
    sc = dict(unit_costs())
    sc[("N", "N")] = 0
    sc[("A", "G")] = 0                               # and a transition that costs nothing one way
    reads = _small_reads(graph[0], "ACGTN", 45) + ["N" * 40, "NANGN"]
    out = check_edit(graph, reads, mode, scores=sc)
    identical(graph[1], reads, mode, scores=sc)
    plain = _run(graph[1], reads, mode)
    assert out[2] != plain[2] and all(a >= b for a, b in zip(out[2], plain[2]))


def test_stream_multi_wrapper_and_cli_give_the_batch_text(tmp_path, capsys):
    from recgraph_amd import api, cli
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(44)
    reads = [rand_bases(rng, 7) + g.path_sequence(i % 3)[5: 25 + 20 * i] + rand_bases(rng, i) for i in range(6)]
    reads += [rand_bases(rng, 1500) + noisy(rng, g.path_sequence(1)) + rand_bases(rng, 700), "NNNN", rand_bases(rng, 2060) + g.path_sequence(2)[30:230]]
    names = ["r%d" % i for i in range(len(reads))]
    for mode in EDIT:
        texts, status = check_edit(graph, reads, mode)[:2]
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4, score_matrix=unit_costs(), o=0, e=-1)
        assert [x.decode() if isinstance(x, bytes) else x for x in st] == texts and list(sstatus) == status
    mt, mstatus = api.align_batch_multi(gg, reads, names, mode=45, device_ids=[0], score_matrix=unit_costs(), o=0, e=-1)
    assert mt == texts and mstatus == status
    rd = reads[6]
    for semi in (False, True):
        line = api.pathwise_alignment_edit_exec(["$"] + list(rd), gg, semi=semi).to_string()
        assert line == _run(gg, [rd], 45 if semi else 44)[0][0].replace("r0\t", "Temp\t", 1).rstrip("\n")
    with pytest.raises(api._lib.RecGraphError):
        api.pathwise_alignment_edit_exec(["$"] + list(rd), gg, score_matrix=api.create_score_matrix_i32(2, -4))
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "45", "-M", "0", "-X", "1", "-O", "0", "-E", "1", "--devices", "0"])
    assert capsys.readouterr().out == "".join(texts)

