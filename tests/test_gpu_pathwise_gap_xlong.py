"""-m 56 / -m 57 / -m 62 (modes 6 / 7 / 12 for reads of up to 131071 bases) on the GPU against the rules of tests/pathwise_gap_rule.py
and tests/pathwise_gap_local_rule.py, which have no length limit, and against modes 16 / 17 / 22 wherever those take the batch.

Every read is checked by check_reads of tests/pathwise_support.py (whole line, re-scored CIGAR, status), whose cap is a
condition: rows of the longest path x (n + 1) <= 1.2e7 per read.  Stripe count is a matter of columns only, so the many-stripe cases
use paths of about 80 rows and the seam cases paths of about 400 rows behind a random flank.

The traceback of these modes keeps the direction words of one stripe and rebuilds each stripe when the walk enters it, so what can go
wrong sits at the seams (a step, a gap run or a state that crosses column 2048 k), in reads that start or end their walk in different
rounds of one batch, and in the counters."""
import re

import numpy as np
import pytest

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
from pathwise_support import align, check_mode, graph_tuple, haplotype, noisy, of_length, rand_bases, run_batch

pytestmark = pytest.mark.gpu
XLONG = (56, 57, 62)
STRIPE = 2048
NEW = {"k_gap_ckpt_long", "k_gap_redo_long", "k_gap_walk_long", "k_gap_walk_local_long"}
XLONG_KERNELS = {56: {"k_gap_score_long", "k_gap_pick", "k_gap_ckpt_long", "k_gap_redo_long", "k_gap_walk_long"},
                 57: {"k_gap_score_long", "k_gap_pick", "k_gap_ckpt_long", "k_gap_redo_long", "k_gap_walk_long"},
                 62: {"k_gap_score_long", "k_gap_pick_local", "k_gap_ckpt_long", "k_gap_redo_long", "k_gap_walk_local_long"}}
GAP_COSTS = [(-4, -2), (0, -2), (-6, 0), (-40, -1)]


@pytest.mark.parametrize("mode", XLONG)
def test_identity_with_the_base_mode(mode):
    """Reads of 1 to 2047 bases: the texts, statuses, scores and both counters of mode m, from the kernels of mode m."""
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(mode)
    w = [g.path_sequence(k) for k in range(3)]
    reads = ["A", w[0][:5], w[1][:63], rand_bases(rng, 64), noisy(rng, w[2]), w[1][40:260], "N" * 30,
             of_length(rng, w[0], 1024), rand_bases(rng, 200) + w[2][50:250] + rand_bases(rng, 300), of_length(rng, w[1], 2047)]
    new, base = run_batch(gg, reads, mode), run_batch(gg, reads, mode - 50)
    assert new[:5] == base[:5] and new.kernels == base.kernels
    assert not new.kernels & NEW and not any(k.endswith("_long") for k in new.kernels)
    check_mode(graph, reads, mode, texts=new[0], status=new[1])


@pytest.mark.parametrize("longest", [2048, 2100, 4096, 4097, 16383])
@pytest.mark.parametrize("mode", XLONG)
def test_identity_with_the_long_mode(mode, longest):
    """What modes 16 / 17 / 22 take, these modes answer with the same bytes — from one stripe of direction words."""
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(longest + mode)
    w = [g.path_sequence(k) for k in range(3)]
    left = int(rng.integers(0, longest - len(w[1])))
    reads = [w[0][100:105], rand_bases(rng, left) + noisy(rng, w[1]) + rand_bases(rng, longest - left - len(w[1])), of_length(rng, w[2], 2047), w[1][7]]
    assert [len(r) for r in reads] == [5, longest, 2047, 1]
    new, old = run_batch(gg, reads, mode), run_batch(gg, reads, mode - 40)
    assert new[:4] == old[:4]
    assert new.kernels == XLONG_KERNELS[mode], new.kernels
    assert not new.kernels & {"k_gap_dirs_long", "k_gap_trace_long", "k_gap_trace_local_long"} and not old.kernels & NEW
    check_mode(graph, reads, mode, texts=new[0], status=new[1])


def _seam_reads(g, rng):
    """Reads whose alignment to path 1 (about 400 rows, behind a random flank) puts one event on the seam 2047 | 2048."""
    w = g.path_sequence(1)
    assert 350 <= len(w) <= 480
    a = 150                                                            # path bases before the event
    at = lambda col: rand_bases(rng, col - a)                               # a flank after which w[a] sits on column `col` + 1
    return [
        at(1900) + w,                                                  # a diagonal step across 2048 -> 2047
        at(1950) + w[:a] + rand_bases(rng, 200) + w[a:],                    # an L run over columns 1951 .. 2150: starts in stripe 1, opens in stripe 0
        at(2047) + w[:a] + rand_bases(rng, 120) + w[a:],                    # an L run that opens on column 2048
        at(2046) + w[:a] + rand_bases(rng, 120) + w[a:],                    # ... and one that opens on column 2047
        at(2048) + w[:a] + w[a + 120:],                                # a U run in column 2048
        at(2047) + w[:a] + w[a + 120:],                                # ... and one in column 2047
        rand_bases(rng, 300) + w[:a] + rand_bases(rng, 7000) + w[a:],            # two whole stripes inside one gap: state X across 6143 .. 2048 on one row
    ]


@pytest.mark.parametrize("oe", GAP_COSTS)
@pytest.mark.parametrize("mode", XLONG)
def test_seams(mode, oe):
    graph = haplotype(400, 3)
    reads = _seam_reads(graph[0], np.random.default_rng(5))
    assert [(len(r) + STRIPE) // STRIPE for r in reads] == [2, 2, 2, 2, 2, 2, 4]
    t, _ = check_mode(graph, reads, mode, o=oe[0], e=oe[1])
    if mode != 62 and oe == (-40, -1):
        # one opening is dear: the inserted bases are one run, and the walk crosses the whole stripes in state X
        c = [x.split("\t")[12].split(",")[0] for x in t]
        assert re.search(r"\d{3}D", c[1]) and re.search(r"\d{3}I", c[4]) and re.search(r"[67]\d{3}D", c[6]), [x[-60:] for x in c]


@pytest.mark.parametrize("mode", [56, 57])
def test_the_walk_reaches_row_0_in_stripe_2_of_4(mode):
    """The border Ls run through stripes 1 and 0, which are never rebuilt."""
    graph = haplotype(300, 3)
    rng = np.random.default_rng(40 + mode)
    w = graph[0].path_sequence(2)
    rd = rand_bases(rng, 5000) + noisy(rng, w) + rand_bases(rng, 7800 - 5000 - len(w))
    assert len(rd) == 7800
    gg = graph[1]
    texts, status, _, counted, performed, _ = run_batch(gg, [rd], mode)
    check_mode(graph, [rd], mode, texts=texts, status=status)
    lnz, rows = graph[2], graph[3]
    assert counted == sum(len(r) for r in rows) * len(rd)
    seen = {}
    assert performed == counted + _traceback_cells(lnz, rows, rd, mode, seen=seen)
    assert sorted(seen) == [2, 3]                    # stripes 0 and 1 were not rebuilt


def test_local_walks_that_start_late_and_stop_early():
    """A piece whose end column lies in stripe 1 of 5 (the higher rounds do nothing) and one that stops in stripe 3 of 5."""
    graph = haplotype(300, 3)
    rng = np.random.default_rng(62)
    piece = graph[0].path_sequence(1)[20:280]
    reads = [rand_bases(rng, 2500) + piece + rand_bases(rng, 9300 - 2500 - len(piece)), rand_bases(rng, 6500) + piece + rand_bases(rng, 9300 - 6500 - len(piece))]
    assert [(len(r) + STRIPE) // STRIPE for r in reads] == [5, 5]
    t, _ = check_mode(graph, reads, 62)
    q = [(int(x.split("\t")[2]), int(x.split("\t")[3])) for x in t]
    for (qs, qe), left in zip(q, (2500, 6500)):
        assert left - 20 <= qs <= left + 20 and left + len(piece) - 20 <= qe <= left + len(piece) + 20, q
        assert qs // STRIPE == qe // STRIPE == (1 if left == 2500 else 3)


def test_local_ties_across_stripes_go_to_the_smallest_column():
    """Equal local maxima on the same row of the same path in different stripes: the column decides."""
    graph = haplotype(400, 3)
    rng = np.random.default_rng(23)
    piece = graph[0].path_sequence(2)          # a whole path: no chance match can lengthen one of the two copies
    for left, mid in ((500, 1800), (1900, 500), (100, 20000)):
        rd = rand_bases(rng, left) + piece + rand_bases(rng, mid) + piece + rand_bases(rng, 100)
        t, _ = check_mode(graph, [rd], 62)
        f = t[0].split("\t")
        assert (int(f[2]), int(f[3])) == (left, left + len(piece) - 1) and f[12].endswith("score: %d" % (2 * len(piece))), f[:5]


def test_local_unaligned():
    from recgraph_amd import api
    graph = haplotype(80, 2)
    t, st = check_mode(graph, ["N" * 3000, "ACGT", "N" * 20000], 62)
    assert st == [api.READ_UNALIGNED, 0, api.READ_UNALIGNED] and t[0] == t[2] == ""


@pytest.mark.parametrize("mode", XLONG)
def test_beyond_the_old_limit(mode):
    """16384 bases (9 stripes), 131071 bases (64 stripes), 40000 and 5 bases in one batch: the walks start in different rounds, and
    every text is that of a batch of the read's own."""
    graph = haplotype(80, 2)
    g, gg, lnz, rows, _ = graph
    assert max(len(r) for r in rows) * 131072 <= 12_000_000
    rng = np.random.default_rng(1000 + mode)
    w = [g.path_sequence(k) for k in range(2)]
    reads = [rand_bases(rng, 9000) + noisy(rng, w[0], 17) + rand_bases(rng, 16384 - 9000 - len(w[0])),
             rand_bases(rng, 70000) + noisy(rng, w[1], 23) + rand_bases(rng, 131071 - 70000 - len(w[1])),
             rand_bases(rng, 39000) + w[0] + rand_bases(rng, 40000 - 39000 - len(w[0])), w[1][30:35]]
    assert [len(r) for r in reads] == [16384, 131071, 40000, 5]
    run = run_batch(gg, reads, mode)
    texts, status, counted = run.texts, run.status, run.counted
    assert run.kernels == XLONG_KERNELS[mode] and counted == sum(len(r) for r in rows) * sum(len(r) for r in reads)
    check_mode(graph, reads, mode, texts=texts, status=status)
    for i, rd in enumerate(reads):
        t, st = align(gg, [rd], mode)
        assert t[0].split("\t")[1:] == texts[i].split("\t")[1:] and st[0] == status[i], (mode, i)
    # what no earlier mode accepts
    from recgraph_amd import api
    with pytest.raises(api._lib.RecGraphError):
        align(gg, reads[:1], mode - 40)


def _traceback_cells(lnz, rows, rd, mode, scores=None, o=-4, e=-2, seen=None):
    """The cells of the checkpoint pass and of the rebuilt stripes of one read, from the walk the rule returns: rows of the picked
    path up to the end row (mode 56: all of them) x n, and per stripe the walk looks at — every (i, j) with i > 0 and j > 0 on it,
    the last one included — the largest such i x the stripe's columns that belong to the read."""
    n = len(rd)
    if mode == 62:
        res = L.align_local(lnz, rows, rd, scores, o, e)
        if res is None:
            return 0
        _, k, end_row, j, _, ops, _ = res
    else:
        _, k, end_row, ops, _ = R.align(lnz, rows, rd, scores, o, e, mode == 57)
        j = n
    i = rows[k].index(end_row) + 1
    cells = (len(rows[k]) if mode == 56 else i) * n
    top = {}
    for op in [None] + list(ops):
        if op is not None:
            i, j = i - (op in "DU"), j - (op in "DL")
        if i > 0 and j > 0:
            top[j // STRIPE] = max(top.get(j // STRIPE, 0), i)
    if seen is not None:
        seen.update(top)
    for s, r in top.items():
        cells += r * (min(n, s * STRIPE + STRIPE - 1) - max(1, s * STRIPE) + 1)
    return cells


def test_65_paths_and_the_counters():
    from recgraph_amd import api, synth
    g = synth.random_dag_graph(60, 65, seed=105)
    g.paths[64] = list(g.paths[3])
    used = {i for p in g.paths for i in p}
    g = synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths)
    graph = graph_tuple(g)
    gg, lnz, rows = graph[1:4]
    rng = np.random.default_rng(65)
    w = g.path_sequence(64)
    reads = [rand_bases(rng, 1000) + w + rand_bases(rng, 2100 - 1000 - len(w)), rand_bases(rng, 2070) + w, w[3:40]]
    assert [len(r) for r in reads][0] == 2100
    for mode in XLONG:
        texts, status, _, counted, performed, _ = run_batch(gg, reads, mode)
        check_mode(graph, reads, mode, texts=texts, status=status)
        assert counted == sum(len(r) for r in rows) * sum(len(r) for r in reads)
        assert performed == counted + sum(_traceback_cells(lnz, rows, rd, mode) for rd in reads), mode
    seqs = [g.path_sequence(q) for q in range(65)]
    best = int(re.search(r"best path: (\d+)", texts[0]).group(1))
    assert seqs[best] == w and best == seqs.index(w) and best < 64         # the lowest of the identical paths


@pytest.mark.parametrize("mode", XLONG)
def test_bad_base_in_a_striped_batch(mode):
    from recgraph_amd import api
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(30 + mode)
    w = g.path_sequence(0)
    long_rd = rand_bases(rng, 1000) + noisy(rng, w) + rand_bases(rng, 2500 - 1000 - len(w))
    reads = [long_rd, long_rd[:2200] + "?" + long_rd[2201:], w[10:200]]
    texts, status = run_batch(gg, reads, mode)[:2]
    assert status == [0, api.READ_BAD_BASE, 0] and texts[1] == ""
    check_mode(graph, [reads[0], reads[2]], mode, texts=[texts[0], texts[2].replace("r2\t", "r1\t", 1)], status=[0, 0])


def test_stream_multi_and_the_wrappers_give_the_batch_text():
    from recgraph_amd import api
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(9)
    reads = [rand_bases(rng, 7) + g.path_sequence(i % 3)[5: 25 + 20 * i] + rand_bases(rng, i) for i in range(6)]
    reads += [rand_bases(rng, 1500) + noisy(rng, g.path_sequence(1)) + rand_bases(rng, 700), "NNNN", rand_bases(rng, 17000) + g.path_sequence(2)[30:230]]
    names = ["r%d" % i for i in range(len(reads))]
    for mode in XLONG:
        texts, status = check_mode(graph, reads, mode)
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4)
        assert [x.decode() if isinstance(x, bytes) else x for x in st] == texts and list(sstatus) == status
        mt, mstatus = api.align_batch_multi(gg, reads, names, mode=mode, device_ids=[0])
        assert mt == texts and mstatus == status
    assert status[7] == api.READ_UNALIGNED
    rd = reads[8]
    for fn, mode in ((api.pathwise_alignment_gap_exec, 56), (api.pathwise_alignment_gap_semi_exec, 57), (api.pathwise_alignment_gap_local_exec, 62)):
        assert fn(["$"] + list(rd), gg, very_long_reads=True).to_string() == align(gg, [rd], mode)[0][0].replace("r0\t", "Temp\t", 1).rstrip("\n")
    with pytest.raises(api._lib.RecGraphError):
        api.pathwise_alignment_gap_exec(["$"] + list(rd), gg, long_reads=True)          # mode 16 keeps its limit of 16383 bases


def test_the_cli_runs_the_modes(tmp_path, capsys):
    from recgraph_amd import api, cli
    g, gg = haplotype(300, 3)[:2]
    rng = np.random.default_rng(11)
    reads = [g.path_sequence(0)[20:120], "NNNN", rand_bases(rng, 12000) + g.path_sequence(1) + rand_bases(rng, 20000 - 12000 - len(g.path_sequence(1)))]
    assert len(reads[2]) == 20000
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fa").write_text("".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    for m in XLONG:
        exp, st = api.align_batch(gg, reads, ["s%d" % i for i in range(3)], mode=m)
        assert st == [0, api.READ_UNALIGNED if m == 62 else 0, 0]
        cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", str(m), "--devices", "0"])
        assert capsys.readouterr().out == "".join(exp)
    out = tmp_path / "out.gaf"
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "62", "--devices", "0", "-o", str(out)])
    assert len(out.read_text().splitlines()) == 2
