"""-m 16 / -m 17 / -m 22 (modes 6 / 7 / 12 for reads of up to 16383 bases) on the GPU against the rules of tests/pathwise_gap_rule.py
and tests/pathwise_gap_local_rule.py, which have no length limit.

Every read is checked as check_batch of the base modes' tests does (check_long): (a) the whole line equals the line built from the
rule's record, and is empty for a read the local rule leaves unaligned; (b) the printed CIGAR, re-scored against the printed path
bases and the read (mode 22: its slice [query start, query end]) with o, e and the matrix, gives exactly the printed score; (c) the
status is 0, or RG_READ_UNALIGNED where the local rule finds nothing.

Stripe count is a matter of columns only: the many-stripe cases use short paths, the realistic-row cases two stripes, so that the
rule's four int64 matrices stay under rows * (n + 1) <= 1.2e7 per read."""
import functools
import os
import re

import numpy as np
import pytest

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = (16, 17, 22)
LONG_KERNELS = {16: {"k_gap_score_long", "k_gap_pick", "k_gap_dirs_long", "k_gap_trace_long"},
                17: {"k_gap_score_long", "k_gap_pick", "k_gap_dirs_long", "k_gap_trace_long"},
                22: {"k_gap_score_long", "k_gap_pick_local", "k_gap_dirs_long", "k_gap_trace_local_long"}}


def _rand(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n))


@functools.lru_cache(maxsize=None)
def _graph(path_len, n_paths=2, seed=71):
    """(SynthGraph, api.Graph, lnz, rows, node ids) of a haplotype graph whose paths have about `path_len` rows."""
    from recgraph_amd import api, synth
    g = synth.haplotype_graph(path_len * 13 // 10, n_paths, path_len=path_len, seed=seed)
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    return g, gg, lnz, rows, R.graph_node_ids(gg)


def _align(gg, reads, mode, scores=None, o=-4, e=-2):
    from recgraph_amd import api
    return api.align_batch(gg, reads, ["r%d" % i for i in range(len(reads))], mode=mode, score_matrix=scores, o=o, e=e)


def check_long(graph, reads, mode, scores=None, o=-4, e=-2, texts=None, status=None):
    """Aligns `reads` in the long mode (or takes `texts` and `status`) and checks every read against the rule; returns (texts, status)."""
    from recgraph_amd import api
    g, gg, lnz, rows, node_ids = graph
    table = None if scores is None else api._table_from_dict(scores)
    if texts is None:
        texts, status = _align(gg, reads, mode, scores, o, e)
    for i, rd in enumerate(reads):
        n = len(rd)
        assert rows and max(len(r) for r in rows) * (n + 1) <= 12_000_000, "the rule would need more than ~400 MB"
        if mode == 22:
            exp = L.line_local(lnz, rows, node_ids, "r%d" % i, rd, table, o, e)
        else:
            exp = R.line(lnz, rows, node_ids, "r%d" % i, rd, table, o, e, mode == 17)
        assert texts[i] == exp, (mode, i, n, texts[i].split("\t")[:12], exp.split("\t")[:12], texts[i][-160:], exp[-160:])       # (a)
        assert status[i] == (0 if exp else api.READ_UNALIGNED), (mode, i, status[i])                             # (c)
        if not exp:
            continue
        f = texts[i][:-1].split("\t")
        mm = re.fullmatch(r"([0-9MXID]+), best path: (\d+), score: (-?\d+)", f[12])
        cigar, k, score, pseq = mm.group(1), int(mm.group(2)), int(mm.group(3)), f[13]
        if mode == 22:                                                                                           # (b)
            qs, qe = int(f[2]), int(f[3])
            assert 0 <= qs <= qe <= n - 1 and score > 0
            assert L.rescore(cigar, pseq, rd, qs, qe, table, o, e) == (score, qe - qs + 1, len(pseq)), (mode, i)
        else:
            assert f[2:4] == ["0", str(n - 1)]
            got, ri, pi = R.rescore(cigar, pseq, rd, table, o, e)
            assert (got, ri, pi) == (score, n, len(pseq)), (mode, i, got, score, ri, pi)
        assert pseq in "".join(lnz[r] for r in rows[k])
    return texts, status


def run_matrix_case(K, cid, results):
    """One case of a kernel matrix K (kernel_matrix_gap_long, kernel_matrix_gap_xlong) with the launch log on, cached in `results`: every
    read checked by check_long as a read of the case's rule in the long family (the same rule and bytes); returns (the instantiations
    each batch launched, the coarse kernel names of all batches)."""
    if cid in results:
        return results[cid]
    from recgraph_amd import api
    case = K.CASES[cid]
    long_mode = case.mode - api._lib.gap_mode(case.mode).family.offset + api._lib.gap_family("_LONG").offset
    g, batches = K.build(case)
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    graph = (g, gg, lnz, rows, R.graph_node_ids(gg))
    per_batch, coarse = [], set()
    try:
        api.set_option("launch_log", 1)
        for reads in batches:
            b = api.Batch(gg, reads, api.make_params(case.mode, **case.kw))
            b.run()
            b.fetch()
            status = [b.status(i) for i in range(len(reads))]
            assert status == [0] * len(reads), cid
            texts = [b.gaf_text(i, "r%d" % i, i + 1) for i in range(len(reads))]
            stats = b.kernel_stats()
            per_batch.append({k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")})
            coarse |= {k for k in stats if not k.startswith("inst:")}
            api.set_option("launch_log", 0)
            check_long(graph, reads, long_mode, texts=texts, status=status, **case.kw)
            api.set_option("launch_log", 1)
    finally:
        api.set_option("launch_log", 0)
    results[cid] = (per_batch, coarse)
    return results[cid]


def _noisy(rng, s, every=97):
    """`s` with a substitution every `every` bases (the length is kept)."""
    s = list(s)
    for k in range(every // 2, len(s), every):
        s[k] = "ACGT"[("ACGT".index(s[k]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def _of_length(rng, w, n):
    """A read of exactly n bases from the path bases w: a noisy prefix, or the whole path with random bases inserted in its middle."""
    if n <= len(w):
        return _noisy(rng, w[:n])
    return _noisy(rng, w[:len(w) // 2]) + _rand(rng, n - len(w)) + _noisy(rng, w[len(w) // 2:])


@pytest.mark.parametrize("mode", LONG)
def test_identity_with_the_base_mode(mode):
    """Reads of 1 to 2047 bases: the texts, status and scores of mode m, from the kernels of mode m."""
    from recgraph_amd import api
    graph = _graph(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(mode)
    w = [g.path_sequence(k) for k in range(3)]
    reads = ["A", w[0][:5], w[1][:63], _rand(rng, 64), _noisy(rng, w[2]), w[1][40:260], "N" * 30,
             _of_length(rng, w[0], 1024), _rand(rng, 200) + w[2][50:250] + _rand(rng, 300), _of_length(rng, w[1], 2047)]
    out = {}
    for m in (mode, mode - 10):
        b = api.Batch(gg, reads, api.make_params(m))
        b.run()
        b.fetch()
        out[m] = ([b.gaf_text(i, "r%d" % i, i + 1) for i in range(len(reads))], [b.status(i) for i in range(len(reads))],
                  [b.score(i) for i in range(len(reads))], b.cell_updates, b.cell_updates_performed, set(b.kernel_stats()))
    assert out[mode][:5] == out[mode - 10][:5]
    assert out[mode][5] == out[mode - 10][5] and not any(k.endswith("_long") for k in out[mode][5])
    check_long(graph, reads, mode, texts=out[mode][0], status=out[mode][1])


@pytest.mark.parametrize("mode", LONG)
def test_mixed_batch(mode):
    """5, 2047, 2048 and 5000 bases in one batch (three stripes; the short reads walk one): the texts of batches of their own."""
    graph = _graph(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(100 + mode)
    w = g.path_sequence(1)
    reads = [w[100:105], _of_length(rng, w, 2047), _of_length(rng, g.path_sequence(2), 2048), _rand(rng, 2600) + _noisy(rng, w) + _rand(rng, 2400 - len(w))]
    assert [len(r) for r in reads] == [5, 2047, 2048, 5000]
    texts, status = check_long(graph, reads, mode)
    for i, rd in enumerate(reads):
        t, st = _align(gg, [rd], mode)
        assert t[0].split("\t")[1:] == texts[i].split("\t")[1:] and st[0] == status[i], (mode, i)


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4095, 4096])
@pytest.mark.parametrize("mode", LONG)
def test_stripe_edges(mode, n):
    """Both sides of the first two stripe boundaries on paths of about 2200 rows; a 2048-base read puts column 2048 alone in lane 0 of
    stripe 1."""
    graph = _graph(2200)
    rng = np.random.default_rng(n)
    rd = _of_length(rng, graph[0].path_sequence(n % 2), n)
    assert len(rd) == n
    check_long(graph, [rd], mode)


@functools.lru_cache(maxsize=None)
def _seam_reads():
    g = _graph(2400)[0]
    rng = np.random.default_rng(5)
    w = g.path_sequence(1)
    assert 2300 <= len(w) <= 2600
    exact = w                                                          # the diagonal crosses 2047 | 2048
    inserted = w[:1948] + _rand(rng, 200) + w[1948:2200]               # an L run over columns 1949 .. 2148
    lacking = w[:2040] + w[2240:2300]                                  # a U run of 200 rows that starts 8 columns before the seam
    return exact, inserted, lacking


@pytest.mark.parametrize("mode", LONG)
def test_crossing_the_seam(mode):
    graph = _graph(2400)
    exact, inserted, lacking = _seam_reads()
    # e = 0: a long gap costs 6 and the flanks pay for it, in the local rule too
    t, _ = check_long(graph, [exact, inserted, lacking], mode, o=-6, e=0)
    c = [x.split("\t")[12].split(",")[0] for x in t]
    assert c[0] == "%dM" % len(exact), c[0][:40]
    assert re.search(r"\d{3}D", c[1]) and re.search(r"\d{3}I", c[2]), [x[:60] for x in c]


@pytest.mark.parametrize("oe", [(-4, -2), (0, -2), (-6, 0), (-40, -1)])
def test_an_inserted_run_across_the_seam_at_every_gap_cost(oe):
    graph = _graph(2400)
    inserted = _seam_reads()[1]
    for mode in (16, 22):
        check_long(graph, [inserted], mode, o=oe[0], e=oe[1])


@pytest.mark.parametrize("mode", [16, 17])
def test_eight_stripes(mode):
    graph = _graph(300, 3)
    rng = np.random.default_rng(8)
    w = graph[0].path_sequence(2)
    rd = _rand(rng, 8000) + _noisy(rng, w) + _rand(rng, 16383 - 8000 - len(w))
    assert len(rd) == 16383
    check_long(graph, [rd], mode)


def test_local_pieces_in_every_stripe():
    """A 300-base piece of a path (a) inside stripe 0, (b) across 2047 | 2048, (c) in the last stripe of a 14400-base read."""
    graph = _graph(400, 3)
    rng = np.random.default_rng(22)
    piece = graph[0].path_sequence(1)[40:340]
    reads = [_rand(rng, 500) + piece + _rand(rng, 1300), _rand(rng, 1900) + piece + _rand(rng, 100), _rand(rng, 14000) + piece + _rand(rng, 100)]
    t, _ = check_long(graph, reads, 22)
    q = [(int(x.split("\t")[2]), int(x.split("\t")[3])) for x in t]
    for (qs, qe), left in zip(q, (500, 1900, 14000)):
        assert left - 20 <= qs <= left + 20 and left + 280 <= qe <= left + 320, q


def test_local_ties_across_stripes_go_to_the_smallest_column():
    """The same piece twice, in two stripes: equal score on the same row of the same path — the column decides, and rows repeat per
    stripe, so "the first one met" would be right only by accident."""
    graph = _graph(400, 3)
    rng = np.random.default_rng(23)
    piece = graph[0].path_sequence(2)          # a whole path: no chance match can lengthen one of the two copies
    for left, mid in ((500, 1800), (1900, 500), (100, 3900)):
        rd = _rand(rng, left) + piece + _rand(rng, mid) + piece + _rand(rng, 100)
        t, _ = check_long(graph, [rd], 22)
        f = t[0].split("\t")
        assert (int(f[2]), int(f[3])) == (left, left + len(piece) - 1) and f[12].endswith("score: %d" % (2 * len(piece))), f[:5]


def test_local_unaligned_and_padding_columns():
    from recgraph_amd import api
    graph = _graph(400, 3)
    t, st = check_long(graph, ["N" * 3000, "ACGT", "N" * 2048], 22)
    assert st == [api.READ_UNALIGNED, 0, api.READ_UNALIGNED] and t[0] == t[2] == ""
    # N entries of +3: the padding columns of the last stripe (base code N) grow along every diagonal and overtake the real cells
    sc = dict(api.create_score_matrix_i32(2, -4))
    for b in "ACGTN":
        sc[(b, "N")] = 3
        sc[("N", b)] = 3
    w = graph[0].path_sequence(0)
    rng = np.random.default_rng(24)
    for n in (2048, 2100, 4095):
        rd = (_rand(rng, n - 250) + w[100:350])[:n]
        check_long(graph, [rd, rd[:-1] + "N"], 22, scores=sc)


def test_65_paths():
    from recgraph_amd import api, synth
    g = synth.random_dag_graph(60, 65, seed=105)
    g.paths[64] = list(g.paths[3])
    used = {i for p in g.paths for i in p}
    g = synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths)
    gg = api.Graph.from_gfa_text(g.gfa())
    lnz, rows = R.graph_paths(gg)
    graph = (g, gg, lnz, rows, R.graph_node_ids(gg))
    rng = np.random.default_rng(65)
    w = g.path_sequence(64)
    rd = _rand(rng, 1000) + w + _rand(rng, 2100 - 1000 - len(w))
    assert len(rd) == 2100
    for mode in LONG:
        t, _ = check_long(graph, [rd], mode)
    seqs = [g.path_sequence(q) for q in range(65)]
    best = int(re.search(r"best path: (\d+)", t[0]).group(1))
    assert seqs[best] == w and best == seqs.index(w) and best < 64         # the lowest of the identical paths


@pytest.mark.parametrize("mode", LONG)
def test_hoxd70(mode):
    from recgraph_amd import api
    sc = api.create_score_matrix_i32(matrix_file_path=os.path.join(ROOT, "tests", "golden", "HOXD70.mtx"))
    graph = _graph(400, 3)
    rng = np.random.default_rng(70)
    w = graph[0].path_sequence(1)
    rd = _rand(rng, 900) + w[:200] + _rand(rng, 9) + w[200:] + _rand(rng, 2100 - 909 - len(w))
    assert len(rd) == 2100
    check_long(graph, [rd], mode, scores=sc, o=-400, e=-30)


@pytest.mark.parametrize("mode", LONG)
def test_bad_base_cells_and_kernel_names(mode):
    from recgraph_amd import api
    graph = _graph(300, 3)
    g, gg, lnz, rows, _ = graph
    rng = np.random.default_rng(30 + mode)
    w = g.path_sequence(0)
    long_rd = _rand(rng, 1000) + _noisy(rng, w) + _rand(rng, 2500 - 1000 - len(w))
    reads = [long_rd, long_rd[:2200] + "?" + long_rd[2201:], w[10:200]]
    b = api.Batch(gg, reads, api.make_params(mode))
    b.run()
    b.fetch()
    status = [b.status(i) for i in range(3)]
    assert status == [0, api.READ_BAD_BASE, 0]
    texts = [b.gaf_text(i, "r%d" % i, i + 1) for i in range(3)]
    assert texts[1] == ""
    check_long(graph, [reads[0], reads[2]], mode, texts=[texts[0], texts[2].replace("r2\t", "r1\t", 1)], status=[0, 0])
    # rows_k * n over the paths and the two clean reads; the direction pass adds the rows of the picked path (modes 17 and 22: up to the
    # end row) times n
    counted = sum(len(r) for r in rows) * (len(reads[0]) + len(reads[2]))
    performed = counted
    for i in (0, 2):
        if mode == 22:
            _, k, end_row = L.align_local(lnz, rows, reads[i])[:3]
        else:
            _, k, end_row = R.align(lnz, rows, reads[i], semi=mode == 17)[:3]
        performed += (rows[k].index(end_row) + 1 if mode != 16 else len(rows[k])) * len(reads[i])
    assert (b.cell_updates, b.cell_updates_performed) == (counted, performed)
    ks = {k for k in b.kernel_stats() if k.startswith("k_gap_")}
    assert ks == LONG_KERNELS[mode], ks


def test_stream_and_multi_give_the_batch_text():
    from recgraph_amd import api
    graph = _graph(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(9)
    reads = [_rand(rng, 7) + g.path_sequence(i % 3)[5: 25 + 20 * i] + _rand(rng, i) for i in range(6)]
    reads += [_rand(rng, 1500) + _noisy(rng, g.path_sequence(1)) + _rand(rng, 700), "NNNN", _rand(rng, 2060) + g.path_sequence(2)[30:230]]
    names = ["r%d" % i for i in range(len(reads))]
    for mode in LONG:
        texts, status = check_long(graph, reads, mode)
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4)
        assert [x.decode() if isinstance(x, bytes) else x for x in st] == texts and list(sstatus) == status
        mt, mstatus = api.align_batch_multi(gg, reads, names, mode=mode, device_ids=[0])
        assert mt == texts and mstatus == status
    assert status[7] == api.READ_UNALIGNED
    rd = reads[6]
    assert api.pathwise_alignment_gap_exec(["$"] + list(rd), gg, long_reads=True).to_string() == _align(gg, [rd], 16)[0][0].replace("r0\t", "Temp\t", 1).rstrip("\n")
    with pytest.raises(api._lib.RecGraphError):
        api.pathwise_alignment_gap_exec(["$"] + list(rd), gg)          # mode 6 keeps its limit of 2047 bases


def test_the_cli_runs_the_long_modes(tmp_path, capsys):
    from recgraph_amd import api, cli
    g, gg = _graph(300, 3)[:2]
    rng = np.random.default_rng(11)
    reads = [g.path_sequence(0)[20:120], "NNNN", _rand(rng, 1200) + g.path_sequence(1) + _rand(rng, 900)]
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fa").write_text("".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    for m in (17, 22):
        exp, st = api.align_batch(gg, reads, ["s%d" % i for i in range(3)], mode=m)
        assert st == [0, api.READ_UNALIGNED if m == 22 else 0, 0]
        cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", str(m), "--devices", "0"])
        assert capsys.readouterr().out == "".join(exp)
    out = tmp_path / "out.gaf"
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "22", "--devices", "0", "-o", str(out)])
    assert len(out.read_text().splitlines()) == 2
