"""-m 64 / -m 65 (modes 26 / 27 at unit costs: both strands of a read scored by ONE wave of edit_strands/rg_edit_strands.hip, the winner
traced once by the kernels of -m 44 / -m 45) on the GPU.

Expected values come from the exact rule of modes 26 / 27 at unit costs — expect_strands(graph, reads, 26 | 27, unit_costs(), 0, -1) of
tests/pathwise_support.py — through check of tests/edit_strands_support.py: whole line, status, strand / score / query accessors, the
CIGAR re-scored on the chosen strand, and both cell counters against the formulas of include/recgraph_hip.h computed from the rule's
answers.  Every read keeps rows * (n + 1) <= 12 M, the rule's own cap.  Every test fails where mode 64 is RG_ERR_ARG."""
import functools

import numpy as np
import pytest

import pathwise_gap_rule as R
import strand_vote_rule as V
from edit_strands_support import KERNELS, MODES, ONE_STRAND, check, dirs_words, expect, instantiations, pair_words, run
from pathwise_support import NO_A, PALINDROME, graph_tuple, haplotype, noisy, rand_bases, run_batch_unit, unit_costs, with_bad_base

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _edge_graph():
    """Three paths of 1, 64 and 65 rows: the edges of the block of 64 path bases a wave gathers at a time."""
    from recgraph_amd import synth
    rng = np.random.default_rng(65)
    graph = graph_tuple(synth.SynthGraph([(1, "G"), (2, rand_bases(rng, 63)), (3, "T")], [(1, 2), (2, 3)], [[1], [1, 2], [1, 2, 3]]))
    assert [len(r) for r in graph[3]] == [1, 64, 65], [len(r) for r in graph[3]]
    return graph


def _graph_for(n):
    """2 to 3 paths of 40 to 700 rows, by the longest read: rows * (n + 1) stays under the rule's cap."""
    if n <= 33:
        return haplotype(40, 3, seed=64)
    if n <= 2048:
        return haplotype(300, 3)
    if n <= 8192:
        return haplotype(500, 2, seed=65)
    return haplotype(650, 2, seed=66)


# ---- 1. widths and edges ----

_LONGEST = [1, 2, 31, 32, 33, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16383]


@pytest.mark.parametrize("n", _LONGEST)
@pytest.mark.parametrize("mode", MODES)
def test_every_width_from_both_sides(mode, n):
    """The longest read of the batch decides W of the score pass (n <= 1024 W) and of the direction pass (n <= 2048 W); the batch also
    holds a shorter read, whose score lane sits low in its half.  The long read is given on the reverse strand for every other n."""
    graph = _graph_for(n)
    g, rows = graph[0], graph[3]
    assert 40 <= max(len(r) for r in rows) <= 732 and max(len(r) for r in rows) * (n + 1) <= 12_000_000
    rng = np.random.default_rng(100 * mode + n)
    w = g.path_sequence(n % len(g.paths))
    # (at unit costs a path is a subsequence of any long random read, on either strand: the flanks are N, which matches nothing, but for
    # about a hundred random bases, so that the path's own strand decides)
    flank = lambda k: "".join("ACGT"[int(x)] if u < min(0.25, 100 / max(k, 1)) else "N" for x, u in zip(rng.integers(0, 4, size=k), rng.random(k)))
    long_rd = w[7:7 + n] if n <= 2 else noisy(rng, w[:n]) if n <= len(w) else flank((n - len(w)) // 3) + noisy(rng, w) + flank(n - len(w) - (n - len(w)) // 3)
    if _LONGEST.index(n) % 2:
        long_rd = V.rc(long_rd)
    reads = [long_rd]
    if n > 1:
        short = g.path_sequence((n + 1) % len(g.paths))[5:5 + min(n - 1, 37)]
        reads.append(short if _LONGEST.index(n) % 2 else V.rc(short))
    assert max(len(r) for r in reads) == len(reads[0]) == n
    res, exp = check(graph, reads, mode, run(graph[1], reads, mode, log=True))
    inst = res["inst"]
    assert set(inst) == instantiations(mode, n), (sorted(inst), pair_words(n), dirs_words(n))
    assert inst["rg::k_edit_trace"] == 1 and inst["rg::k_gap_pick"] == 2 and not any("k_edit_score<" in k for k in inst), inst
    if n >= 31:       # (a read of one or two bases ties between the strands)
        assert exp[0][2] == "+-"[_LONGEST.index(n) % 2], [x[2] for x in exp]


@pytest.mark.parametrize("mode", MODES)
def test_paths_of_1_64_and_65_rows(mode):
    """The gather block's edge: a path ends with the block (64 rows), one row behind it (65), and after one row."""
    graph = _edge_graph()
    g = graph[0]
    w = g.path_sequence(2)
    rng = np.random.default_rng(mode)
    reads = [w, V.rc(w), w[:64], V.rc(w[:64]), "G", "C", w[10:50], V.rc(noisy(rng, w, 17)), rand_bases(rng, 70), "ACGT"]
    res, exp = check(graph, reads, mode)
    assert {x[2] for x in exp} == {"+", "-"}


# ---- 2. lane 31 | 32 ----

@pytest.mark.parametrize("words", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_nothing_crosses_from_lane_31_into_lane_32(mode, words):
    """n = 1024 W fills both halves to their last bit.  (a) a read that IS a path piece: forward Eq is all ones on the diagonal, and
    the carry of the wide addition runs out of lane 31; (b) the reverse complement of a path piece: the reverse half carries from lane
    32 up; (c) poly-A against paths without an A: the last column goes up in every row, so the top bit of lane 31's Ph is set.  A
    carry or a shifted bit that leaked into lane 32 would change the reverse strand's score, and with it the record or the strand."""
    n = 1024 * words
    graph = haplotype(1200 if words == 1 else 2200)
    g = graph[0]
    w0, w1 = g.path_sequence(0), g.path_sequence(1)
    assert len(w0) >= n + 60 and len(w1) >= n + 60 and max(len(r) for r in graph[3]) * (n + 1) <= 12_000_000
    reads = [w0[50:50 + n], V.rc(w1[60:60 + n]), V.rc(w0[3:40])]
    res, exp = check(graph, reads, mode, run(graph[1], reads, mode, log=True))
    assert set(res["inst"]) == instantiations(mode, n)
    assert [x[2] for x in exp][:2] == ["+", "-"]
    if mode == 65:
        assert res["score"] == [0, 0, 0]              # a piece of a path costs nothing in the semiglobal kind
    no_a = graph_tuple(NO_A)
    assert not any("A" in no_a[2][r] for rows in no_a[3] for r in rows)
    reads = ["A" * n, "T" * n, "A" * (n - 1)]
    res, exp = check(no_a, reads, mode, run(no_a[1], reads, mode, log=True))
    assert set(res["inst"]) == instantiations(mode, n)
    assert exp[0][2] == "-" and exp[1][2] == "+"       # A^n finds its T's on the reverse strand, T^n on the forward one


# ---- 3. strands ----

@functools.lru_cache(maxsize=None)
def _many_paths():
    """70 paths of about 130 rows: the score pass's grid has more than one page of 64 paths in x."""
    from recgraph_amd import synth
    g = synth.random_dag_graph(60, 70, seed=164)
    used = {i for p in g.paths for i in p}
    g = synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths)
    graph = graph_tuple(g)
    assert len(graph[3]) == 70
    return graph


@functools.lru_cache(maxsize=None)
def _equal_score_read(semi):
    """A read that is no reverse palindrome and scores the same on both strands of the 70-path graph (searched with a fixed seed; the
    search must succeed)."""
    g, gg, lnz, rows, _ = _many_paths()
    rng = np.random.default_rng(5 + semi)
    sc = R.default_scores(0, -1)
    for _ in range(200):
        rd = rand_bases(rng, int(rng.integers(5, 12)))
        if rd != V.rc(rd) and R.align(lnz, rows, rd, sc, 0, -1, semi)[0] == R.align(lnz, rows, V.rc(rd), sc, 0, -1, semi)[0]:
            return rd
    raise AssertionError("no short read scores the same on both strands of this graph: the precondition of the case does not hold")


def _mixed_reads(mode):
    g = _many_paths()[0]
    rng = np.random.default_rng(mode)
    w = [g.path_sequence(k) for k in (0, 33, 64, 69)]
    pieces = [w[0], w[1][10:90], noisy(rng, w[2], 23), noisy(rng, w[3][5:100], 11), w[2][:40] + w[2][44:]]
    reads = pieces + [V.rc(p) for p in pieces]
    reads += [PALINDROME, _equal_score_read(mode == 65), with_bad_base(w[1][20:90]), "N" * 30, w[0][:20] + "NNN" + w[0][23:60], V.rc(w[3][:30] + "N" + w[3][31:80])]
    return reads


@pytest.mark.parametrize("table", ["default", "n-matches-n"])
@pytest.mark.parametrize("mode", MODES)
def test_a_mixed_batch_on_70_paths(mode, table):
    """Path pieces forward with 0 and with a few edits; the same as reverse complements; a reverse palindrome and an equal-score pair,
    which tie and stay '+'; a bad base: status, no line, no strand; reads with N, under the default 0 / -1 table and under one in which
    N matches N."""
    from recgraph_amd import api
    graph = _many_paths()
    reads = _mixed_reads(mode)
    sc = dict(unit_costs())
    if table != "default":
        sc[("N", "N")] = 0
    res, exp = check(graph, reads, mode, scores=sc)
    records = [x for x in exp if x[0]]
    assert min(sum(x[2] == s for x in records) for s in "+-") * 4 >= len(records), [x[2] for x in exp]
    assert [x[2] for x in exp[10:12]] == ["+", "+"] and exp[10][3] == ["+", "-"]                 # the ties
    assert res["status"][12] == api.READ_BAD_BASE and res["texts"][12] == "" and res["strand"][12] is None and res["score"][12] == 0
    assert res["strand"][:5] == ["+"] * 5 and res["strand"][5:10] == ["-"] * 5
    assert res["score"][0] == res["score"][5] == 0 and res["score"][2] < 0


@pytest.mark.parametrize("chunk_reads", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_chunks_index_the_second_state_and_the_strand_bytes_per_chunk(mode, chunk_reads):
    """5 reads of different lengths and strands in chunks of 1 (the smallest chunk_reads: 5 chunks) and of 2: every chunk has its own
    reverse picks, strand bytes and oriented reads, at the input's offsets minus the chunk's first."""
    from recgraph_amd import api
    graph = _many_paths()
    g = graph[0]
    w = [g.path_sequence(k) for k in (1, 40, 68)]
    reads = [V.rc(w[0][:70]), w[1][3:50], V.rc(w[2]), w[0][20:31], V.rc(w[1][:99])]
    whole = run(graph[1], reads, mode)
    api.set_option("chunk_reads", chunk_reads)
    try:
        res = run(graph[1], reads, mode)
    finally:
        api.set_option("chunk_reads", 0)
    res, exp = check(graph, reads, mode, res)
    assert [x[2] for x in exp] == ["-", "+", "-", "+", "-"]
    assert res["stats"]["k_edit_score_pair"] == -(-5 // chunk_reads) and whole["stats"]["k_edit_score_pair"] == 1, res["stats"]
    assert (res["texts"], res["status"], res["strand"], res["cells"]) == (whole["texts"], whole["status"], whole["strand"], whole["cells"])


# ---- 4. surface ----

def test_wrapper_cli_and_stream_give_the_batch_text(tmp_path, capsys):
    from recgraph_amd import api, cli
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(64)
    plus, minus = noisy(rng, g.path_sequence(1)[10:200], 31), V.rc(noisy(rng, g.path_sequence(2)[30:250], 29))
    for semi in (False, True):
        mode = 65 if semi else 64
        exp = expect(graph, [plus, minus], mode)
        assert [x[2] for x in exp] == ["+", "-"]
        for rd, name, strand in ((plus, "r0", "+"), (minus, "r1", "-")):
            rec = api.pathwise_alignment_edit_strands_exec(["$"] + list(rd), gg, semi=semi)
            want = exp[0 if strand == "+" else 1][0]
            assert rec.to_string() == want.replace(name + "\t", "Temp\t", 1).rstrip("\n") and rec.to_string().split("\t")[4] == strand
    reads = [plus, minus, rand_bases(rng, 40), g.path_sequence(0)[:33], V.rc(g.path_sequence(0)[100:164]), "NNNN", V.rc(rand_bases(rng, 1100) + g.path_sequence(1))]
    names = ["r%d" % i for i in range(len(reads))]
    for mode in MODES:
        res, exp = check(graph, reads, mode)
        for both in (False, True):       # both_strands=True is redundant
            st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=3, both_strands=both,
                                           score_matrix=unit_costs(), o=0, e=-1)
            assert [x.decode() if isinstance(x, bytes) else x for x in st] == res["texts"] and list(sstatus) == res["status"]
        bt, bstatus = api.align_batch(gg, reads, names, mode=mode, both_strands=True, score_matrix=unit_costs(), o=0, e=-1)
        assert bt == res["texts"] and bstatus == res["status"]
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    capsys.readouterr()                  # (the checker printed its figures)
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "65", "-M", "0", "-X", "1", "-O", "0", "-E", "1", "--both-strands", "--devices", "0"])
    assert capsys.readouterr().out == "".join(res["texts"])


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_without_reverse_winners_is_mode_44_or_45(mode):
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(44 + mode)
    reads = [g.path_sequence(0), noisy(rng, g.path_sequence(1), 19), g.path_sequence(2)[40:41], rand_bases(rng, 900) + noisy(rng, g.path_sequence(2)) + rand_bases(rng, 300),
             PALINDROME, with_bad_base(g.path_sequence(1)[:80])]
    res, exp = check(graph, reads, mode)
    assert all(x[2] in "+ " for x in exp)
    one = run_batch_unit(gg, reads, ONE_STRAND[mode])
    assert (res["texts"], res["status"], res["score"]) == (one.texts, one.status, one.scores)
    # both strands are always scored: twice the counted cells of the one-strand mode, and the same direction pass
    assert res["cells"] == (2 * one.counted, one.counted + one.performed)
    assert set(res["stats"]) == KERNELS and "k_edit_score" not in res["stats"]
