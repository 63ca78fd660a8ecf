"""-m 94 / -m 95 (modes 56 / 57 restricted to unit costs, for reads of up to 131071 bases; a batch with a read over 16383 bases runs the
striped bit-vector kernels of edit_xlong/rg_path_edit_xlong.hip) on the GPU.

Up to 16383 bases the test is identity with modes 44 / 45: texts, statuses, scores, both counters and the kernels.  Beyond, it is
identity with modes 56 / 57 on the same rg_params (texts, statuses, scores, counted cells) and every read against the numpy rule of
modes 6 / 7 at unit costs through check_reads of tests/pathwise_support.py (whole line, re-scored CIGAR, status), whose cap is a
condition: rows of the longest path x (n + 1) <= 1.2e7 per read — so the graphs have about 700 rows at 16500 columns, 300 at 40000
and 80 at 131071.

The traceback keeps D0 and Ph of one stripe and rebuilds a stripe when the walk enters it, and the stripes of the score pass talk
through two bits per row, so what can go wrong sits at the seam 16384 | 16385 (a diagonal, a gap run, a mismatch on either side), in
walks that start or reach row 0 in different rounds of one batch, and in the counters."""
import functools

import numpy as np
import pytest

import pathwise_edit_xlong_rule as X
import pathwise_gap_rule as R
from pathwise_support import EDIT_KERNELS, check_reads, graph_tuple, haplotype, noisy, of_length, rand_bases, run_batch_unit, unit_costs

pytestmark = pytest.mark.gpu
XLONG = (94, 95)
STRIPE = 16384
XLONG_KERNELS = {"k_edit_score_xlong", "k_gap_pick", "k_edit_redo_xlong", "k_edit_walk_xlong"}
GAP_XLONG_NEW = {"k_gap_score_long", "k_gap_ckpt_long", "k_gap_redo_long", "k_gap_walk_long"}


def _rule(mode):
    from recgraph_amd import api
    return api._lib.GAP_SEMI if mode == 95 else api._lib.GAP_GLOBAL


def _checked(graph, reads, mode, scores=None):
    """A batch of mode 94 / 95 with every read checked against the rule at unit costs (or the table `scores`); returns the batch."""
    out = run_batch_unit(graph[1], reads, mode, scores)
    check_reads(graph, reads, _rule(mode), unit_costs() if scores is None else scores, 0, -1, texts=out.texts, status=out.status)
    return out


def _rebuilt(graph, rd, mode, scores=None):
    """(cells, stripes) the traceback of `rd` rebuilds, from the rule's walk (pathwise_edit_xlong_rule.rebuilt)."""
    lnz, rows = graph[2], graph[3]
    _, k, end_row, ops = R.align(lnz, rows, rd, R.default_scores(0, -1) if scores is None else scores, 0, -1, mode == 95)[:4]
    return X.rebuilt("".join(ops), rows[k].index(end_row) + 1, len(rd))


@pytest.mark.parametrize("longest", [1, 2049, 16383])
@pytest.mark.parametrize("mode", XLONG)
def test_identity_with_modes_44_and_45(mode, longest):
    """Everything of mode 44 / 45, both counters included, from that mode's kernels."""
    g, gg = haplotype(300, 3)[:2]
    rng = np.random.default_rng(longest + mode)
    w = [g.path_sequence(k) for k in range(3)]
    reads = [of_length(rng, w[1], longest)] + ([w[0][100:105], of_length(rng, w[2], 2047), w[1][7]] if longest > 1 else [])
    assert max(len(r) for r in reads) == len(reads[0]) == longest
    new, old = run_batch_unit(gg, reads, mode), run_batch_unit(gg, reads, mode - 50)
    assert new[:5] == old[:5] and new.status == [0] * len(reads)
    assert new.kernels == old.kernels == EDIT_KERNELS and not new.kernels & XLONG_KERNELS - {"k_gap_pick"}


@pytest.mark.parametrize("longest", [16384, 16385, 32768, 32769, 40000])
@pytest.mark.parametrize("mode", XLONG)
def test_identity_with_modes_56_and_57_and_the_rule(mode, longest):
    graph = haplotype(250, 3)
    g, gg, lnz, rows, _ = graph
    assert max(len(r) for r in rows) * (longest + 1) <= 12_000_000
    rng = np.random.default_rng(longest + mode)
    w = [g.path_sequence(k) for k in range(3)]
    left = int(rng.integers(0, longest - len(w[1])))
    reads = [w[0][100:105], rand_bases(rng, left) + noisy(rng, w[1]) + rand_bases(rng, longest - left - len(w[1])), of_length(rng, w[2], 2047)]
    assert [len(r) for r in reads] == [5, longest, 2047]
    new, old = _checked(graph, reads, mode), run_batch_unit(gg, reads, mode - 38)
    assert new[:4] == old[:4] and new.status == [0, 0, 0]
    assert new.kernels == XLONG_KERNELS, new.kernels
    assert old.kernels & GAP_XLONG_NEW and not new.kernels & GAP_XLONG_NEW
    assert new.counted == sum(len(r) for r in rows) * sum(len(r) for r in reads)
    assert new.performed == new.counted + sum(_rebuilt(graph, rd, mode)[0] for rd in reads)


def _seam_reads(g, rng):
    """Reads whose alignment to path 1 (about 400 rows, behind a random flank) puts one event on the seam 16384 | 16385."""
    w = g.path_sequence(1)
    assert 350 <= len(w) <= 480
    a = 150                                                            # path bases before the event
    at = lambda col: rand_bases(rng, col - a)                          # a flank after which w[a] sits on column `col` + 1
    return [
        at(16234) + w,                                                 # a diagonal of matches across 16385 -> 16384: hin = -1
        at(16284) + w[:a] + rand_bases(rng, 200) + w[a:],              # an L run over columns 16285 .. 16484: starts in stripe 1, ends in stripe 0
        at(16383) + w[:a] + rand_bases(rng, 120) + w[a:],              # an L run that opens on column 16384
        at(16384) + w[:a] + rand_bases(rng, 120) + w[a:],              # ... and one that opens on column 16385
        at(16384) + w[:a] + w[a + 120:],                               # a U run in column 16384
        at(16385) + w[:a] + w[a + 120:],                               # ... and one in column 16385
    ]


@pytest.mark.parametrize("mode", XLONG)
def test_seams(mode):
    graph = haplotype(400, 3)
    reads = _seam_reads(graph[0], np.random.default_rng(5))
    assert [(len(r) + STRIPE - 1) // STRIPE for r in reads] == [2] * 6
    out = _checked(graph, reads, mode)
    old = run_batch_unit(graph[1], reads, mode - 38)
    assert out[:4] == old[:4] and out.kernels == XLONG_KERNELS


@pytest.mark.parametrize("mode", XLONG)
def test_an_insertion_that_swallows_a_whole_stripe(mode):
    """20000 bases inside the path, over all of stripe 1 (columns 16385 .. 32768), once random and once N.  At unit costs a path is a
    subsequence of any long random read, and the walk takes a diagonal wherever one is optimal: it finds the rows of the path among the
    first random bases it meets and is through in stripe 2.  N matches nothing: that walk crosses stripe 1 on one row, and all three
    stripes are rebuilt.  About 300 rows: at 34650 columns the cap of check_reads leaves no room for the 400 of the other seam reads."""
    graph = haplotype(300, 3)
    rng = np.random.default_rng(20000 + mode)
    w = graph[0].path_sequence(1)
    reads = [rand_bases(rng, 14350) + w[:150] + mid + w[150:] for mid in (rand_bases(rng, 20000), "N" * 20000)]
    assert all((len(rd) + STRIPE - 1) // STRIPE == 3 for rd in reads) and 14500 < STRIPE and 14500 + 20000 > 2 * STRIPE
    assert max(len(r) for r in graph[3]) * (len(reads[0]) + 1) <= 12_000_000
    out = _checked(graph, reads, mode)
    old = run_batch_unit(graph[1], reads, mode - 38)
    assert out[:4] == old[:4] and out.kernels == XLONG_KERNELS
    rebuilt = [_rebuilt(graph, rd, mode) for rd in reads]
    assert rebuilt[1][1] == [2, 1, 0] and out.performed == out.counted + rebuilt[0][0] + rebuilt[1][0]


@functools.lru_cache(maxsize=None)
def _homopolymer_graph(n):
    from recgraph_amd import synth
    return graph_tuple(synth.SynthGraph([(1, "A" * 300), (2, "A" * (n - 300))], [(1, 2)], [[1, 2]]))


@pytest.mark.parametrize("mode", XLONG)
def test_homopolymer_across_the_seam(mode):
    """A^16500 against a path A^600: Eq and Pv are all ones in every stripe, the diagonal of matches crosses the seam on every row
    (hin = -1, the carry that must not be lost); one C on the last bit of stripe 0 and on bit 0 of stripe 1 stops and restarts it."""
    graph = _homopolymer_graph(600)
    n = 16500
    reads = ["A" * n] + ["A" * t + "C" + "A" * (n - t - 1) for t in (16383, 16384)]
    out = _checked(graph, reads, mode)
    old = run_batch_unit(graph[1], reads, mode - 38)
    assert out[:4] == old[:4] and out.kernels == XLONG_KERNELS
    # global: 15900 of the read's bases are inserted (mode 95: every base but 600 as well: the whole read must be used)
    assert out.scores[0] == -(n - 600) and all(s in (-(n - 600), -(n - 600) - 1) for s in out.scores[1:]), out.scores


@pytest.mark.parametrize("mode", XLONG)
def test_the_walk_reaches_row_0_in_stripe_1_of_3(mode):
    """The border Ls run through stripe 0, which is never rebuilt; `performed` is the score pass plus the rebuilt cells of the rule's walk."""
    graph = haplotype(250, 3)
    g, gg, lnz, rows, _ = graph
    rng = np.random.default_rng(40 + mode)
    w = g.path_sequence(2)
    # (a tail of N, which matches nothing: a random tail would hold the path as a subsequence, and the walk would be through in stripe 2)
    rd = rand_bases(rng, 20000) + noisy(rng, w) + "N" * (40000 - 20000 - len(w))
    assert len(rd) == 40000 and (len(rd) + STRIPE - 1) // STRIPE == 3
    out = _checked(graph, [rd], mode)
    assert out.counted == sum(len(r) for r in rows) * len(rd)
    cells, stripes = _rebuilt(graph, rd, mode)
    assert out.performed == out.counted + cells
    assert stripes == [2, 1]                         # stripe 0 was not rebuilt


@pytest.mark.parametrize("mode", XLONG)
def test_walks_that_start_in_different_rounds(mode):
    """16384 bases (one stripe of the batch's 8), 131071 (all 8), 40000 (3) and 5 bases in one batch: the walks start in different
    rounds, and every text is that of a batch of the read's own.  The 40000-base read is the first 30 bases of a path behind bases that
    match nothing: in mode 95 its best row lies early on the path, and its stripe is rebuilt for those rows only."""
    from recgraph_amd import api
    graph = haplotype(80, 2)
    g, gg, lnz, rows, _ = graph
    assert max(len(r) for r in rows) * 131072 <= 12_000_000
    rng = np.random.default_rng(1000 + mode)
    w = [g.path_sequence(k) for k in range(2)]
    reads = [rand_bases(rng, 9000) + noisy(rng, w[0], 17) + rand_bases(rng, 16384 - 9000 - len(w[0])),
             rand_bases(rng, 70000) + noisy(rng, w[1], 23) + "N" * (131071 - 70000 - len(w[1])),      # (its walk crosses stripes 7 .. 4 on one row)
             "N" * (40000 - 30) + w[0][:30], w[1][30:35]]
    assert [len(r) for r in reads] == [16384, 131071, 40000, 5]
    out = _checked(graph, reads, mode)
    assert out.kernels == XLONG_KERNELS and out.counted == sum(len(r) for r in rows) * sum(len(r) for r in reads)
    rebuilt = [_rebuilt(graph, rd, mode) for rd in reads]
    assert out.performed == out.counted + sum(c for c, _ in rebuilt)
    assert rebuilt[0][1] == [0] and rebuilt[1][1][0] == 7 and len(rebuilt[1][1]) >= 4 and rebuilt[2][1][0] == 2 and rebuilt[3][1] == [0]
    # (one round of rebuild and walk per stripe of the longest read)
    assert out.stats["k_edit_redo_xlong"][1] == out.stats["k_edit_walk_xlong"][1] == 8
    for i, rd in enumerate(reads):
        own = run_batch_unit(gg, [rd], mode)
        assert own.texts[0].split("\t")[1:] == out.texts[i].split("\t")[1:] and own.status[0] == out.status[i] and own.scores[0] == out.scores[i], (mode, i)
    if mode == 95:
        _, k, end_row = R.align(lnz, rows, reads[2], R.default_scores(0, -1), 0, -1, True)[:3]
        assert rows[k].index(end_row) < 40
    # what mode 44 / 45 does not accept
    with pytest.raises(api._lib.RecGraphError) as ex:
        run_batch_unit(gg, reads, mode - 50)
    assert "16383" in str(ex.value)


@functools.lru_cache(maxsize=None)
def _graph_of_65_paths():
    from recgraph_amd import synth
    g = synth.random_dag_graph(60, 65, seed=105)
    used = {i for p in g.paths for i in p}
    return graph_tuple(synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths))


@pytest.mark.parametrize("mode", XLONG)
def test_65_paths(mode):
    """The boundary slots of a read run past one 64-path page, and the picked path is the last one: its bases between bases that match
    nothing, so that no other path ties, the walk starting in stripe 1 on its last row."""
    graph = _graph_of_65_paths()
    g, gg, lnz, rows = graph[:4]
    w = g.path_sequence(64)
    assert all(g.path_sequence(q) != w for q in range(64)) and max(len(r) for r in rows) * 16501 <= 12_000_000
    reads = ["N" * 8000 + w + "N" * (16500 - 8000 - len(w)), w[3:40]]
    out = _checked(graph, reads, mode)
    assert out.kernels == XLONG_KERNELS and "best path: 64," in out.texts[0]
    assert out.counted == sum(len(r) for r in rows) * sum(len(r) for r in reads)
    rebuilt = [_rebuilt(graph, rd, mode) for rd in reads]
    assert rebuilt[0][1] == [1, 0] and out.performed == out.counted + rebuilt[0][0] + rebuilt[1][0]


@functools.lru_cache(maxsize=None)
def _graph_with_n():
    """One bubble between two segments of 100 bases over ACGTN: about a fifth of the path bases are N."""
    from recgraph_amd import synth
    rng = np.random.default_rng(28)
    seg = lambda k: rand_bases(rng, k, "ACGTN")
    return graph_tuple(synth.SynthGraph([(1, seg(100)), (2, seg(10)), (3, seg(12)), (4, seg(100))], [(1, 2), (1, 3), (2, 4), (3, 4)], [[1, 2, 4], [1, 3, 4]]))


@pytest.mark.parametrize("mode", XLONG)
def test_a_custom_table_in_which_n_matches_n(mode):
    graph = _graph_with_n()
    g, gg = graph[0], graph[1]
    sc = dict(unit_costs())
    sc[("N", "N")] = 0
    sc[("A", "G")] = 0                               # and a transition that costs nothing one way
    rng = np.random.default_rng(77 + mode)
    w = g.path_sequence(1)
    reads = ["N" * 16300 + w[:100] + "NNN" + w[100:], "NANGN", "N" * 40, rand_bases(rng, 16384, "ACGTN")]
    out = _checked(graph, reads, mode, scores=sc)
    old = run_batch_unit(gg, reads, mode - 38, sc)
    assert out[:4] == old[:4] and out.kernels == XLONG_KERNELS
    # (the N of the reads find the N of the paths: every read scores higher than under the plain 0 / -1 table)
    plain = run_batch_unit(gg, reads, mode)
    assert all(a > b for a, b in zip(out.scores, plain.scores)), (out.scores, plain.scores)


@pytest.mark.parametrize("mode", XLONG)
def test_a_bad_base_among_long_reads(mode):
    from recgraph_amd import api
    graph = haplotype(250, 3)
    g, gg, lnz, rows, _ = graph
    rng = np.random.default_rng(8 + mode)
    w = g.path_sequence(0)
    long_rd = rand_bases(rng, 16200) + noisy(rng, w) + rand_bases(rng, 20000 - 16200 - len(w))
    reads = [long_rd, long_rd[:16390] + "?" + long_rd[16391:], w[10:200], long_rd[:100] + "?" + long_rd[101:]]
    got = run_batch_unit(gg, reads, mode)
    old = run_batch_unit(gg, reads, mode - 38)
    assert got[:4] == old[:4] and got.kernels == XLONG_KERNELS
    assert got.status == [0, api.READ_BAD_BASE, 0, api.READ_BAD_BASE] and got.texts[1] == got.texts[3] == ""
    check_reads(graph, [reads[0], reads[2]], _rule(mode), unit_costs(), 0, -1, texts=[got.texts[0], got.texts[2].replace("r2\t", "r1\t", 1)], status=[0, 0])
    counted = sum(len(r) for r in rows) * (len(reads[0]) + len(reads[2]))
    assert (got.counted, got.performed) == (counted, counted + sum(_rebuilt(graph, reads[i], mode)[0] for i in (0, 2)))


def test_stream_multi_wrapper_and_cli_give_the_batch_text(tmp_path, capsys):
    from recgraph_amd import api, cli
    graph = haplotype(250, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(94)
    reads = [rand_bases(rng, 7) + g.path_sequence(i % 3)[5: 25 + 20 * i] + rand_bases(rng, i) for i in range(4)]
    reads += [rand_bases(rng, 16300) + noisy(rng, g.path_sequence(1)) + rand_bases(rng, 700), "NNNN", rand_bases(rng, 17000) + g.path_sequence(2)[30:230]]
    names = ["r%d" % i for i in range(len(reads))]
    for mode in XLONG:
        out = _checked(graph, reads, mode)
        texts, status = out.texts, out.status
        # tiles of 4: the first tile runs the kernels of mode 44 / 45, the second the striped ones
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4, score_matrix=unit_costs(), o=0, e=-1)
        assert [x.decode() if isinstance(x, bytes) else x for x in st] == texts and list(sstatus) == status
    mt, mstatus = api.align_batch_multi(gg, reads, names, mode=95, device_ids=[0], score_matrix=unit_costs(), o=0, e=-1)
    assert mt == texts and mstatus == status
    rd = reads[4]
    for semi in (False, True):
        line = api.pathwise_alignment_edit_xlong_exec(["$"] + list(rd), gg, semi=semi).to_string()
        assert line == run_batch_unit(gg, [rd], 95 if semi else 94).texts[0].replace("r0\t", "Temp\t", 1).rstrip("\n")
    with pytest.raises(api._lib.RecGraphError):
        api.pathwise_alignment_edit_xlong_exec(["$"] + list(rd), gg, score_matrix=api.create_score_matrix_i32(2, -4))
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "94", "-M", "0", "-X", "1", "-O", "0", "-E", "1", "--devices", "0"])
    want = run_batch_unit(gg, reads, 94).texts
    assert capsys.readouterr().out == "".join(want)
