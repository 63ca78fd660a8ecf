"""-m 6 / -m 7 (pathwise alignment with affine gaps) on the GPU against the rule of tests/pathwise_gap_rule.py.

Every read is checked three ways (check_base of tests/pathwise_support.py): (a) the whole line equals the line built from the rule's
record — path string, path length, start and end derived from (best path, end row, ops) as the walkers do — and, where -m 4 walks the
same rows (same CIGAR, path and bases), also -m 4's line with the comments column replaced;
(b) the printed CIGAR, re-scored against the printed path bases with o, e and the matrix, gives exactly the printed score and
consumes the whole read (and, in -m 6, the whole path) — true whatever the tie rules; (c) the status is 0."""
import os
import re

import numpy as np
import pytest

from pathwise_support import DIAMOND, TWO_BUBBLES, check_base, rand_bases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_checked_results():
    t, _ = check_base(DIAMOND, ["ATG"], False)
    assert t[0] == "r0\t3\t0\t2\t+\t>1>2>4\t3\t0\t2\t0\t*\t*\t3M, best path: 0, score: 6\tATG\n"
    t, _ = check_base(TWO_BUBBLES, ["ATGCT", "ATGGGAT"], False)
    assert t[0] == "r0\t5\t0\t4\t+\t>1>2>4>5>7\t5\t0\t4\t0\t*\t*\t3M1X1M, best path: 0, score: 4\tATGAT\n"
    assert t[1].split("\t")[12:] == ["2M2D3M, best path: 0, score: 2", "ATGAT\n"]
    t, _ = check_base(TWO_BUBBLES, ["T"], True)
    assert t[0].split("\t")[5] == ">2" and t[0].split("\t")[12:] == ["1M, best path: 0, score: 2", "T\n"]


@pytest.mark.parametrize("semi", [False, True])
def test_small_graphs(semi):
    rng = np.random.default_rng(3)
    for gfa in (DIAMOND, TWO_BUBBLES):
        reads = [rand_bases(rng, int(rng.integers(1, 9))) for _ in range(40)] + ["A", "N", "ANG", "TTTTTTTT"]
        _, whole = check_base(gfa, reads, semi)
        assert whole >= 1


@pytest.mark.parametrize("semi", [False, True])
def test_example_data(example_gfa, example_reads, semi):
    check_base(example_gfa, example_reads[1], semi)


@pytest.mark.parametrize("P", [1, 2, 64, 65, 256])
def test_path_counts_and_identical_paths(P):
    """Up to 256 paths (one wave per path; k_gap_pick strides over them), with two pairs of identical paths: the lowest index wins."""
    from recgraph_amd import synth
    g = synth.random_dag_graph(60, P, seed=40 + P)
    if P >= 64:
        g.paths[P - 1] = list(g.paths[3])
        g.paths[40] = list(g.paths[17])
    elif P == 2:
        g.paths[1] = list(g.paths[0])
    used = {i for p in g.paths for i in p}              # (a segment on no path has no PathGraph row)
    g = synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths)
    rng = np.random.default_rng(P)
    picks = sorted({0, P - 1, 3 % P, 40 % P, 17 % P})
    walks = [g.path_sequence(k) for k in picks]
    reads = walks + [w[:len(w) // 2] + rand_bases(rng, 5) + w[len(w) // 2 + 3:] for w in walks]
    texts, _ = check_base(g.gfa(), reads, False)
    for k, t in zip(picks, texts):
        best = int(re.search(r"best path: (\d+)", t).group(1))
        seqs = [g.path_sequence(q) for q in range(P)]
        assert best == seqs.index(seqs[k]), (k, best)
    # -m 7: substrings from the middle of a walk
    mids = [w[len(w) // 3: len(w) // 3 + 25] for w in walks] + [w[-12:] for w in walks]
    check_base(g.gfa(), mids, True)


def _haplotype():
    from recgraph_amd import synth
    return synth.haplotype_graph(600, 4, path_len=150, seed=21)


@pytest.mark.parametrize("semi", [False, True])
def test_both_sides_of_every_column_count(semi):
    """63 | 64, 255 | 256, 511 | 512, 1023 | 1024 and 2047 bases: n + 1 <= 64 C picks C = 4, 8, 16, 32; one batch per length (the longest
    read of a batch picks C), the long reads built by repeating a path's bases."""
    g = _haplotype()
    for n in (63, 64, 255, 256, 511, 512, 1023, 1024, 2047):
        k = n % 4
        check_base(g.gfa(), [(g.path_sequence(k) * (n // 100 + 1))[:n]], semi)


def test_mixed_lengths_long_runs_and_flat_reads():
    g = _haplotype()
    rng = np.random.default_rng(8)
    w = g.path_sequence(2)
    reads = [w[:5], (w * 8)[:1000],                                      # 5 and 1000 bases in one batch
             w[:70] + rand_bases(rng, 200) + w[70:],                          # 200 inserted bases: an L run that crosses lanes
             "A" * 90, "N" * 40, "T", w[:40] + "N" * 10 + w[50:]]
    check_base(g.gfa(), reads, False)
    check_base(g.gfa(), reads, True)
    # a read that lacks 200 path rows (a U run): on a graph whose paths are longer than that
    from recgraph_amd import synth
    big = synth.haplotype_graph(1200, 3, path_len=400, seed=22)
    v = big.path_sequence(1)
    check_base(big.gfa(), [v[:100] + v[300:], v[:100] + v[300:350]], False)
    check_base(big.gfa(), [v[:100] + v[300:350]], True)


@pytest.mark.parametrize("oe", [(-4, -2), (0, -2), (-6, 0), (-40, -1)])
def test_gap_costs(oe):
    g = _haplotype()
    rng = np.random.default_rng(5)
    w = g.path_sequence(1)
    reads = [w, w[:30] + w[45:], w[:60] + rand_bases(rng, 12) + w[60:], w[:20] + w[22:90] + "ACG" + w[90:], rand_bases(rng, 50)]
    for semi in (False, True):
        check_base(g.gfa(), reads, semi, o=oe[0], e=oe[1])


def test_hoxd70():
    from recgraph_amd import api
    sc = api.create_score_matrix_i32(matrix_file_path=os.path.join(ROOT, "tests", "golden", "HOXD70.mtx"))
    g = _haplotype()
    rng = np.random.default_rng(6)
    w = g.path_sequence(3)
    reads = [w, w[:50] + w[70:], w[:80] + rand_bases(rng, 9) + w[80:], rand_bases(rng, 130), w[:30] + "N" + w[31:]]
    for semi in (False, True):
        check_base(g.gfa(), reads, semi, scores=sc, o=-400, e=-30)


def test_bad_base_and_cells():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    b = api.Batch(g, ["ATGAT", "AT?AT", "ACG"], api.make_params(api.MODE_PATHWISE_GAP))
    b.run()
    b.fetch()
    assert [b.status(i) for i in range(3)] == [0, api.READ_BAD_BASE, 0]
    # rows_k * n over both paths (5 rows each) and the two clean reads; the direction pass adds the picked path's
    assert b.cell_updates == 2 * 5 * (5 + 3) and b.cell_updates_performed == 2 * 5 * (5 + 3) + 5 * (5 + 3)
    assert {"k_gap_score", "k_gap_pick", "k_gap_dirs", "k_gap_trace"} <= set(b.kernel_stats())


def test_stream_and_multi_give_the_batch_text():
    from recgraph_amd import api
    g = _haplotype()
    rng = np.random.default_rng(9)
    reads = [g.path_sequence(i % 4)[: 20 + 9 * i] for i in range(12)] + [rand_bases(rng, 300)]
    names = ["r%d" % i for i in range(len(reads))]
    gg = api.Graph.from_gfa_text(g.gfa())
    for mode, semi in ((api.MODE_PATHWISE_GAP, False), (api.MODE_PATHWISE_GAP_SEMI, True)):
        texts, _ = check_base(g.gfa(), reads, semi)
        st, status = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=5)
        assert st == texts and status == [0] * len(reads)
        mt, status = api.align_batch_multi(gg, reads, names, mode=mode, device_ids=[0])
        assert mt == texts and status == [0] * len(reads)
    ex = api.pathwise_alignment_gap_exec(["$"] + list(reads[3]), gg)
    assert ex.to_string() == texts_of(gg, reads[3], api.MODE_PATHWISE_GAP)
    with pytest.raises(api._lib.RecGraphError):
        api.align_stream(gg, reads, names, mode=api.MODE_PATHWISE_GAP, both_strands=True, device_ids=[0])


def texts_of(gg, read, mode):
    from recgraph_amd import api
    return api.align_batch(gg, [read], ["Temp"], mode=mode)[0][0].rstrip("\n")
