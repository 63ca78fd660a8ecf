"""-m 12 (local pathwise alignment with affine gaps) on the GPU against the rule of tests/pathwise_gap_local_rule.py.

Every read is checked three ways (check_local of tests/pathwise_support.py): (a) the whole line equals the line built from the rule's
record — query start and end, path string, path length, start and end — and is empty for a read the rule leaves unaligned; (b) the printed CIGAR, re-scored
against the printed path bases and the read slice [query start, query end] with o, e and the matrix, gives exactly the printed
score and consumes exactly that slice — true whatever the tie rules; (c) the status is 0, or RG_READ_UNALIGNED where the rule finds
no local alignment.  Every aligned read also scores > 0 and at least what -m 7 gives the same read."""
import os
import re

import numpy as np
import pytest

from pathwise_support import DIAMOND, NO_G, TWO_BUBBLES, check_local, rand_bases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_checked_lines():
    t, st = check_local(DIAMOND, ["CCATGCC", "ATG", "NNN", "G", "TTCGTT"])
    assert t[0] == "r0\t7\t2\t4\t+\t>1>2>4\t3\t0\t2\t0\t*\t*\t3M, best path: 0, score: 6\tATG\n"
    assert t[1] == "r1\t3\t0\t2\t+\t>1>2>4\t3\t0\t2\t0\t*\t*\t3M, best path: 0, score: 6\tATG\n"
    assert t[2] == "" and t[3].split("\t")[12] == "1M, best path: 0, score: 2"
    assert t[4] == "r4\t6\t2\t3\t+\t>3>4\t2\t0\t1\t0\t*\t*\t2M, best path: 1, score: 4\tCG\n"
    assert st == [0, 0, 16, 0, 0]
    t, _ = check_local(TWO_BUBBLES, ["GGATGATCC", "A", "AA"])
    assert t[0] == "r0\t9\t2\t6\t+\t>1>2>4>5>7\t5\t0\t4\t0\t*\t*\t5M, best path: 0, score: 10\tATGAT\n"
    assert t[2].split("\t")[2:4] == ["0", "0"]              # the smallest column of the tie
    sc = _scores(5, -4)
    t, _ = check_local(TWO_BUBBLES, ["CCATGGATCC"], scores=sc)
    assert t[0].split("\t")[2:4] == ["2", "7"] and t[0].split("\t")[12:] == ["2M1D3M, best path: 0, score: 19", "ATGAT\n"]


def _scores(m, x):
    from recgraph_amd import api
    return api.create_score_matrix_i32(m, x)


def test_small_graphs():
    rng = np.random.default_rng(3)
    for gfa in (DIAMOND, TWO_BUBBLES):
        reads = [rand_bases(rng, int(rng.integers(1, 9))) for _ in range(40)] + ["A", "N", "ANG", "TTTTTTTT", "NNNNN"]
        check_local(gfa, reads)


def _haplotype():
    from recgraph_amd import synth
    return synth.haplotype_graph(600, 4, path_len=150, seed=21)


def test_overhangs_and_exact_substrings():
    from recgraph_amd import api
    g = _haplotype()
    rng = np.random.default_rng(4)
    w, v = g.path_sequence(1), g.path_sequence(3)
    reads = [rand_bases(rng, 50) + w[20:120], w[20:120] + rand_bases(rng, 50), rand_bases(rng, 50) + v[10:140] + rand_bases(rng, 50), rand_bases(rng, 50) + w + rand_bases(rng, 50)]
    t, _ = check_local(g.gfa(), reads)
    # the flanks are clipped (a few flank bases may join the alignment by chance: the rule above decides, this only says "clipped")
    q = [(int(x.split("\t")[2]), int(x.split("\t")[3])) for x in t]
    assert q[0][0] >= 40 and q[0][1] == len(reads[0]) - 1 and q[1][0] == 0 and q[1][1] <= 120, q
    assert q[2][0] >= 40 and q[2][1] <= len(reads[2]) - 41 and q[3][0] >= 40 and q[3][1] <= len(reads[3]) - 41, q
    # an exact substring of a path: the -m 7 line, byte for byte
    subs = [w[30:90], v[:40], v[100:], w, w[75:76]]
    t, st = check_local(g.gfa(), subs)
    m7, _ = api.align_batch(api.Graph.from_gfa_text(g.gfa()), subs, ["r%d" % i for i in range(len(subs))], mode=api.MODE_PATHWISE_GAP_SEMI)
    assert t == m7 and st == [0] * len(subs)


def test_long_runs_that_cross_lanes():
    """200 inserted bases (an L run) and 200 missing path rows (a U run) inside one local alignment: with e = 0 a long gap costs 6 and the
    flanks pay for it."""
    from recgraph_amd import synth
    big = synth.haplotype_graph(1200, 3, path_len=400, seed=22)
    rng = np.random.default_rng(8)
    v = big.path_sequence(1)
    reads = [v[:100] + rand_bases(rng, 200) + v[100:220], v[:100] + v[300:], rand_bases(rng, 30) + v[50:120] + v[320:390] + rand_bases(rng, 30)]
    t, _ = check_local(big.gfa(), reads, o=-6, e=0)
    assert re.search(r"\d{3}D", t[0].split("\t")[12]) and re.search(r"\d{3}I", t[1].split("\t")[12]), [x.split("\t")[12][:80] for x in t]
    # the default costs drop the gap and keep one flank
    check_local(big.gfa(), reads)


def test_free_gap_opening_and_a_long_inserted_run():
    """o = 0 with a match far above |e|: the flanks pay for a long inserted run, and with o = 0 every L of the run costs the walk three
    steps (H -> X, the L, the arrival back in H: `h + o >= x` always holds) — the step bound of k_gap_trace_local must allow 3 per
    column.  Path AT against A + 99 C + T is D, 99 L, D: 299 steps on 2 rows and 101 columns."""
    AT = "S\t1\tA\nS\t2\tT\nL\t1\t+\t2\t+\t0M\nP\tp0\t1+,2+\t*\n"
    for m, e in ((100, -1), (10, -1), (100, 0)):
        sc = _scores(m, -4)
        reads = ["A" + "C" * 99 + "T", "A" + "C" * 9 + "T", "GA" + "C" * 30 + "TG"]
        t, st = check_local(AT, reads, scores=sc, o=0, e=e)
        assert st == [0, 0, 0]
        if m == 100:
            assert t[0].split("\t")[12:] == ["1M99D1M, best path: 0, score: %d" % (200 + 99 * e), "AT\n"], t[0]
            assert t[2].split("\t")[2:4] == ["1", "32"], t[2]
    # the same inside longer reads and paths: 200 inserted bases between two pieces of a path, every C
    g = _haplotype()
    rng = np.random.default_rng(14)
    w = g.path_sequence(0)
    for n_ins in (200, 900):
        check_local(g.gfa(), [w[:60] + rand_bases(rng, n_ins) + w[60:120], rand_bases(rng, 20) + w[10:70] + rand_bases(rng, n_ins) + w[70:140]], scores=_scores(50, -4), o=0, e=-1)


def test_both_sides_of_every_column_count():
    """63 | 64, 255 | 256, 511 | 512, 1023 | 1024 and 2047 bases: n + 1 <= 64 C picks C = 4, 8, 16, 32; one batch per length (the longest
    read of a batch picks C), the long reads built by repeating a path's bases."""
    g = _haplotype()
    for n in (63, 64, 255, 256, 511, 512, 1023, 1024, 2047):
        k = n % 4
        check_local(g.gfa(), [(g.path_sequence(k) * (n // 100 + 1))[:n]])


@pytest.mark.parametrize("P", [1, 2, 64, 65, 256])
def test_path_counts_and_identical_paths(P):
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
    reads = [rand_bases(rng, 9) + w + rand_bases(rng, 9) for w in walks] + [w[len(w) // 3: len(w) // 3 + 25] for w in walks]
    texts, _ = check_local(g.gfa(), reads)
    seqs = [g.path_sequence(q) for q in range(P)]
    for k, t in zip(picks, texts):
        best = int(re.search(r"best path: (\d+)", t).group(1))
        assert seqs[best] == seqs[k] and best == seqs.index(seqs[k]), (k, best)


@pytest.mark.parametrize("oe", [(-4, -2), (0, -2), (-6, 0), (-40, -1)])
def test_gap_costs(oe):
    g = _haplotype()
    rng = np.random.default_rng(5)
    w = g.path_sequence(1)
    reads = [w, w[:30] + w[45:], w[:60] + rand_bases(rng, 12) + w[60:], w[:20] + w[22:90] + "ACG" + w[90:], rand_bases(rng, 50),
             rand_bases(rng, 20) + w[40:100] + rand_bases(rng, 20)]
    check_local(g.gfa(), reads, o=oe[0], e=oe[1])


def test_hoxd70():
    from recgraph_amd import api
    sc = api.create_score_matrix_i32(matrix_file_path=os.path.join(ROOT, "tests", "golden", "HOXD70.mtx"))
    g = _haplotype()
    rng = np.random.default_rng(6)
    w = g.path_sequence(3)
    reads = [w, w[:50] + w[70:], w[:80] + rand_bases(rng, 9) + w[80:], rand_bases(rng, 130), w[:30] + "N" + w[31:], rand_bases(rng, 40) + w[30:110] + rand_bases(rng, 40)]
    check_local(g.gfa(), reads, scores=sc, o=-400, e=-30)


def test_positive_n_entries_do_not_let_padding_columns_win():
    """A matrix whose N entries are +3: the columns past the read (base code N) then grow along every diagonal and overtake the real
    cells.  22 bases: column 23 is padding inside the boundary lane (C = 4: lane 5 owns 20 .. 23), 24 onwards whole padding lanes; 23
    bases: the padding starts with a lane of its own."""
    sc = dict(_scores(2, -4))
    for b in "ACGTN":
        sc[(b, "N")] = 3
        sc[("N", b)] = 3
    g = _haplotype()
    w = g.path_sequence(2)
    for n in (22, 23, 255, 256):
        check_local(g.gfa(), [(w * 3)[5:5 + n], (w * 3)[40:40 + n - 1] + "N"], scores=sc)


def test_unaligned_reads_leave_their_neighbours_alone():
    from recgraph_amd import api
    reads = ["ACTA", "GGGG", "CT", "NNNNNN", "G", "TA"]
    t, st = check_local(NO_G, reads)
    assert st == [0, 16, 0, 16, 16, 0] and [bool(x) for x in t] == [True, False, True, False, False, True]
    g = api.Graph.from_gfa_text(NO_G)
    b = api.Batch(g, reads, api.make_params(api.MODE_PATHWISE_GAP_LOCAL))
    b.run()
    b.fetch()
    assert [b.score(i) for i in (1, 3, 4)] == [0, 0, 0] and b.score(0) == 8
    alone, _ = api.align_batch(g, ["ACTA"], ["r0"], mode=api.MODE_PATHWISE_GAP_LOCAL)
    assert alone[0] == t[0]
    with pytest.raises(api._lib.RecGraphError):
        api.pathwise_alignment_gap_local_exec(["$"] + list("GGGG"), g)
    assert api.pathwise_alignment_gap_local_exec(["$"] + list("GACTAG"), g).to_string() == api.align_batch(g, ["GACTAG"], ["Temp"], mode=12)[0][0].rstrip("\n")


def test_mixed_lengths():
    g = _haplotype()
    rng = np.random.default_rng(8)
    w = g.path_sequence(2)
    reads = [w[:5], (w * 8)[:1000], "A" * 90, "N" * 40, "T", w[:40] + "N" * 10 + w[50:], rand_bases(rng, 300)]
    check_local(g.gfa(), reads)


def test_bad_base_cells_and_kernel_names():
    from recgraph_amd import api
    g = api.Graph.from_gfa_text(TWO_BUBBLES)
    b = api.Batch(g, ["CCATGCC", "AT?AT", "ACG", "NN"], api.make_params(api.MODE_PATHWISE_GAP_LOCAL))
    b.run()
    b.fetch()
    assert [b.status(i) for i in range(4)] == [0, api.READ_BAD_BASE, 0, api.READ_UNALIGNED]
    # rows_k * n over both paths (5 rows each) and the three clean reads; the direction pass adds the picked path's rows up to the end
    # row: ATG ends on row 4, the third row of path 0; ACG on row 4, the third row of path 1; nothing for the unaligned read
    counted = 2 * 5 * (7 + 3 + 2)
    assert b.cell_updates == counted and b.cell_updates_performed == counted + 3 * 7 + 3 * 3
    assert {"k_gap_score_local", "k_gap_pick_local", "k_gap_dirs_local", "k_gap_trace_local"} <= set(b.kernel_stats())
    assert not any(k.startswith("k_gap_") and not k.endswith("_local") for k in b.kernel_stats())


def test_stream_and_multi_give_the_batch_text():
    from recgraph_amd import api
    g = _haplotype()
    rng = np.random.default_rng(9)
    reads = [rand_bases(rng, 7) + g.path_sequence(i % 4)[5: 25 + 9 * i] + rand_bases(rng, i) for i in range(12)] + [rand_bases(rng, 300), "NNNN"]
    names = ["r%d" % i for i in range(len(reads))]
    gg = api.Graph.from_gfa_text(g.gfa())
    texts, status = check_local(g.gfa(), reads)
    assert status[-1] == api.READ_UNALIGNED
    st, sstatus = api.align_stream(gg, reads, names, mode=api.MODE_PATHWISE_GAP_LOCAL, device_ids=[0], handles_per_device=2, tile_reads=5)
    assert [x.decode() if isinstance(x, bytes) else x for x in st] == texts and list(sstatus) == status
    mt, mstatus = api.align_batch_multi(gg, reads, names, mode=api.MODE_PATHWISE_GAP_LOCAL, device_ids=[0])
    assert mt == texts and mstatus == status
    with pytest.raises(api._lib.RecGraphError):
        api.align_stream(gg, reads, names, mode=api.MODE_PATHWISE_GAP_LOCAL, both_strands=True, device_ids=[0])


def test_the_cli_writes_the_aligned_reads_and_skips_the_unaligned(tmp_path, capsys):
    """-m 12 end to end: stdout and -o hold the batch's lines; the unaligned read in the middle has none and stops nothing."""
    from recgraph_amd import api, cli
    reads = ["GACTAG", "GGGG", "CT", "NNNN", "TA"]
    (tmp_path / "g.gfa").write_text(NO_G)
    (tmp_path / "r.fa").write_text("".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    exp, st = api.align_batch(api.Graph.from_gfa_text(NO_G), reads, ["s%d" % i for i in range(5)], mode=api.MODE_PATHWISE_GAP_LOCAL)
    assert st == [0, 16, 0, 16, 0] and exp[1] == exp[3] == ""
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "12", "--devices", "0"])
    assert capsys.readouterr().out == "".join(exp)
    out = tmp_path / "out.gaf"
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "12", "--devices", "0", "-o", str(out)])
    got = out.read_text().splitlines()
    assert len(got) == 3 and [x.split("\t")[:12] for x in got] == [x.rstrip("\n").split("\t")[:12] for x in exp if x]
