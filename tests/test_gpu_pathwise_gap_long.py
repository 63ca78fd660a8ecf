"""-m 16 / -m 17 / -m 22 (modes 6 / 7 / 12 for reads of up to 16383 bases) on the GPU against the rules of tests/pathwise_gap_rule.py
and tests/pathwise_gap_local_rule.py, which have no length limit.

Every read is checked by check_reads of tests/pathwise_support.py, the checker of the base modes (through check_mode, which aligns
first): (a) the whole line equals the line built from the rule's record, and is empty for a read the local rule leaves unaligned;
(b) the printed CIGAR, re-scored against the printed path bases and the read (mode 22: its slice [query start, query end]) with o, e
and the matrix, gives exactly the printed score; (c) the status is 0, or RG_READ_UNALIGNED where the local rule finds nothing.

Stripe count is a matter of columns only: the many-stripe cases use short paths, the realistic-row cases two stripes, so that the
rule's four int64 matrices stay under rows * (n + 1) <= 1.2e7 per read."""
import functools
import os
import re

import numpy as np
import pytest

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
from pathwise_support import align, check_mode, graph_tuple, haplotype, noisy, of_length, rand_bases, run_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = (16, 17, 22)
LONG_KERNELS = {16: {"k_gap_score_long", "k_gap_pick", "k_gap_dirs_long", "k_gap_trace_long"},
                17: {"k_gap_score_long", "k_gap_pick", "k_gap_dirs_long", "k_gap_trace_long"},
                22: {"k_gap_score_long", "k_gap_pick_local", "k_gap_dirs_long", "k_gap_trace_local_long"}}


@pytest.mark.parametrize("mode", LONG)
def test_identity_with_the_base_mode(mode):
    """Reads of 1 to 2047 bases: the texts, status and scores of mode m, from the kernels of mode m."""
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(mode)
    w = [g.path_sequence(k) for k in range(3)]
    reads = ["A", w[0][:5], w[1][:63], rand_bases(rng, 64), noisy(rng, w[2]), w[1][40:260], "N" * 30,
             of_length(rng, w[0], 1024), rand_bases(rng, 200) + w[2][50:250] + rand_bases(rng, 300), of_length(rng, w[1], 2047)]
    new, base = run_batch(gg, reads, mode), run_batch(gg, reads, mode - 10)
    assert new[:5] == base[:5]
    assert set(new.stats) == set(base.stats) and not any(k.endswith("_long") for k in new.stats)
    check_mode(graph, reads, mode, texts=new.texts, status=new.status)


@pytest.mark.parametrize("mode", LONG)
def test_mixed_batch(mode):
    """5, 2047, 2048 and 5000 bases in one batch (three stripes; the short reads walk one): the texts of batches of their own."""
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(100 + mode)
    w = g.path_sequence(1)
    reads = [w[100:105], of_length(rng, w, 2047), of_length(rng, g.path_sequence(2), 2048), rand_bases(rng, 2600) + noisy(rng, w) + rand_bases(rng, 2400 - len(w))]
    assert [len(r) for r in reads] == [5, 2047, 2048, 5000]
    texts, status = check_mode(graph, reads, mode)
    for i, rd in enumerate(reads):
        t, st = align(gg, [rd], mode)
        assert t[0].split("\t")[1:] == texts[i].split("\t")[1:] and st[0] == status[i], (mode, i)


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4095, 4096])
@pytest.mark.parametrize("mode", LONG)
def test_stripe_edges(mode, n):
    """Both sides of the first two stripe boundaries on paths of about 2200 rows; a 2048-base read puts column 2048 alone in lane 0 of
    stripe 1."""
    graph = haplotype(2200)
    rng = np.random.default_rng(n)
    rd = of_length(rng, graph[0].path_sequence(n % 2), n)
    assert len(rd) == n
    check_mode(graph, [rd], mode)


@functools.lru_cache(maxsize=None)
def _seam_reads():
    g = haplotype(2400)[0]
    rng = np.random.default_rng(5)
    w = g.path_sequence(1)
    assert 2300 <= len(w) <= 2600
    exact = w                                                          # the diagonal crosses 2047 | 2048
    inserted = w[:1948] + rand_bases(rng, 200) + w[1948:2200]               # an L run over columns 1949 .. 2148
    lacking = w[:2040] + w[2240:2300]                                  # a U run of 200 rows that starts 8 columns before the seam
    return exact, inserted, lacking


@pytest.mark.parametrize("mode", LONG)
def test_crossing_the_seam(mode):
    graph = haplotype(2400)
    exact, inserted, lacking = _seam_reads()
    # e = 0: a long gap costs 6 and the flanks pay for it, in the local rule too
    t, _ = check_mode(graph, [exact, inserted, lacking], mode, o=-6, e=0)
    c = [x.split("\t")[12].split(",")[0] for x in t]
    assert c[0] == "%dM" % len(exact), c[0][:40]
    assert re.search(r"\d{3}D", c[1]) and re.search(r"\d{3}I", c[2]), [x[:60] for x in c]


@pytest.mark.parametrize("oe", [(-4, -2), (0, -2), (-6, 0), (-40, -1)])
def test_an_inserted_run_across_the_seam_at_every_gap_cost(oe):
    graph = haplotype(2400)
    inserted = _seam_reads()[1]
    for mode in (16, 22):
        check_mode(graph, [inserted], mode, o=oe[0], e=oe[1])


@pytest.mark.parametrize("mode", [16, 17])
def test_eight_stripes(mode):
    graph = haplotype(300, 3)
    rng = np.random.default_rng(8)
    w = graph[0].path_sequence(2)
    rd = rand_bases(rng, 8000) + noisy(rng, w) + rand_bases(rng, 16383 - 8000 - len(w))
    assert len(rd) == 16383
    check_mode(graph, [rd], mode)


def test_local_pieces_in_every_stripe():
    """A 300-base piece of a path (a) inside stripe 0, (b) across 2047 | 2048, (c) in the last stripe of a 14400-base read."""
    graph = haplotype(400, 3)
    rng = np.random.default_rng(22)
    piece = graph[0].path_sequence(1)[40:340]
    reads = [rand_bases(rng, 500) + piece + rand_bases(rng, 1300), rand_bases(rng, 1900) + piece + rand_bases(rng, 100), rand_bases(rng, 14000) + piece + rand_bases(rng, 100)]
    t, _ = check_mode(graph, reads, 22)
    q = [(int(x.split("\t")[2]), int(x.split("\t")[3])) for x in t]
    for (qs, qe), left in zip(q, (500, 1900, 14000)):
        assert left - 20 <= qs <= left + 20 and left + 280 <= qe <= left + 320, q


def test_local_ties_across_stripes_go_to_the_smallest_column():
    """The same piece twice, in two stripes: equal score on the same row of the same path — the column decides, and rows repeat per
    stripe, so "the first one met" would be right only by accident."""
    graph = haplotype(400, 3)
    rng = np.random.default_rng(23)
    piece = graph[0].path_sequence(2)          # a whole path: no chance match can lengthen one of the two copies
    for left, mid in ((500, 1800), (1900, 500), (100, 3900)):
        rd = rand_bases(rng, left) + piece + rand_bases(rng, mid) + piece + rand_bases(rng, 100)
        t, _ = check_mode(graph, [rd], 22)
        f = t[0].split("\t")
        assert (int(f[2]), int(f[3])) == (left, left + len(piece) - 1) and f[12].endswith("score: %d" % (2 * len(piece))), f[:5]


def test_local_unaligned_and_padding_columns():
    from recgraph_amd import api
    graph = haplotype(400, 3)
    t, st = check_mode(graph, ["N" * 3000, "ACGT", "N" * 2048], 22)
    assert st == [api.READ_UNALIGNED, 0, api.READ_UNALIGNED] and t[0] == t[2] == ""
    # N entries of +3: the padding columns of the last stripe (base code N) grow along every diagonal and overtake the real cells
    sc = dict(api.create_score_matrix_i32(2, -4))
    for b in "ACGTN":
        sc[(b, "N")] = 3
        sc[("N", b)] = 3
    w = graph[0].path_sequence(0)
    rng = np.random.default_rng(24)
    for n in (2048, 2100, 4095):
        rd = (rand_bases(rng, n - 250) + w[100:350])[:n]
        check_mode(graph, [rd, rd[:-1] + "N"], 22, scores=sc)


def test_65_paths():
    from recgraph_amd import api, synth
    g = synth.random_dag_graph(60, 65, seed=105)
    g.paths[64] = list(g.paths[3])
    used = {i for p in g.paths for i in p}
    g = synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths)
    graph = graph_tuple(g)
    rng = np.random.default_rng(65)
    w = g.path_sequence(64)
    rd = rand_bases(rng, 1000) + w + rand_bases(rng, 2100 - 1000 - len(w))
    assert len(rd) == 2100
    for mode in LONG:
        t, _ = check_mode(graph, [rd], mode)
    seqs = [g.path_sequence(q) for q in range(65)]
    best = int(re.search(r"best path: (\d+)", t[0]).group(1))
    assert seqs[best] == w and best == seqs.index(w) and best < 64         # the lowest of the identical paths


@pytest.mark.parametrize("mode", LONG)
def test_hoxd70(mode):
    from recgraph_amd import api
    sc = api.create_score_matrix_i32(matrix_file_path=os.path.join(ROOT, "tests", "golden", "HOXD70.mtx"))
    graph = haplotype(400, 3)
    rng = np.random.default_rng(70)
    w = graph[0].path_sequence(1)
    rd = rand_bases(rng, 900) + w[:200] + rand_bases(rng, 9) + w[200:] + rand_bases(rng, 2100 - 909 - len(w))
    assert len(rd) == 2100
    check_mode(graph, [rd], mode, scores=sc, o=-400, e=-30)


@pytest.mark.parametrize("mode", LONG)
def test_bad_base_cells_and_kernel_names(mode):
    from recgraph_amd import api
    graph = haplotype(300, 3)
    g, gg, lnz, rows, _ = graph
    rng = np.random.default_rng(30 + mode)
    w = g.path_sequence(0)
    long_rd = rand_bases(rng, 1000) + noisy(rng, w) + rand_bases(rng, 2500 - 1000 - len(w))
    reads = [long_rd, long_rd[:2200] + "?" + long_rd[2201:], w[10:200]]
    b = run_batch(gg, reads, mode)
    texts, status = b.texts, b.status
    assert status == [0, api.READ_BAD_BASE, 0]
    assert texts[1] == ""
    check_mode(graph, [reads[0], reads[2]], mode, texts=[texts[0], texts[2].replace("r2\t", "r1\t", 1)], status=[0, 0])
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
    assert (b.counted, b.performed) == (counted, performed)
    ks = {k for k in b.stats if k.startswith("k_gap_")}
    assert ks == LONG_KERNELS[mode], ks


def test_stream_and_multi_give_the_batch_text():
    from recgraph_amd import api
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(9)
    reads = [rand_bases(rng, 7) + g.path_sequence(i % 3)[5: 25 + 20 * i] + rand_bases(rng, i) for i in range(6)]
    reads += [rand_bases(rng, 1500) + noisy(rng, g.path_sequence(1)) + rand_bases(rng, 700), "NNNN", rand_bases(rng, 2060) + g.path_sequence(2)[30:230]]
    names = ["r%d" % i for i in range(len(reads))]
    for mode in LONG:
        texts, status = check_mode(graph, reads, mode)
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4)
        assert [x.decode() if isinstance(x, bytes) else x for x in st] == texts and list(sstatus) == status
        mt, mstatus = api.align_batch_multi(gg, reads, names, mode=mode, device_ids=[0])
        assert mt == texts and mstatus == status
    assert status[7] == api.READ_UNALIGNED
    rd = reads[6]
    assert api.pathwise_alignment_gap_exec(["$"] + list(rd), gg, long_reads=True).to_string() == align(gg, [rd], 16)[0][0].replace("r0\t", "Temp\t", 1).rstrip("\n")
    with pytest.raises(api._lib.RecGraphError):
        api.pathwise_alignment_gap_exec(["$"] + list(rd), gg)          # mode 6 keeps its limit of 2047 bases


def test_the_cli_runs_the_long_modes(tmp_path, capsys):
    from recgraph_amd import api, cli
    g, gg = haplotype(300, 3)[:2]
    rng = np.random.default_rng(11)
    reads = [g.path_sequence(0)[20:120], "NNNN", rand_bases(rng, 1200) + g.path_sequence(1) + rand_bases(rng, 900)]
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
