"""-m 76 / -m 77 / -m 82 (modes 6 / 7 / 12 on both strands, reads of up to 131071 bases, the traceback run once) on the GPU against
the composed rule of tests/pathwise_gap_xstrands_rule.py: which strands are picked and which one wins by the rules of modes 26 / 27
/ 32 on the picked scores, the report and both counters by the rules of modes 56 / 57 / 62 on the strand that won.

Every read is checked the same way (check_x of tests/pathwise_support.py): check_strands against the rule's answer
(whole line, status, strand and score accessors, query coordinates, the CIGAR re-scored on the chosen strand), and the batch's two
cell counters against the rule's sums.  Beside the rule stand two identities with the same build: the bytes of mode m + 20 wherever
that mode takes the batch, and the line of the winning strand's sequence in mode m + 50.

The shapes are the smallest that can go wrong: paths of 300 rows (2200 where a stage must be striped at realistic rows), the hand
graph of five rows for the reads beyond 16383 bases; the rule's matrices stay under rows * (n + 1) <= 1.2e7 per read."""
import functools
import re

import numpy as np
import pytest

import pathwise_gap_rule as R
import pathwise_gap_xstrands_rule as X
import strand_vote_rule as V
from pathwise_support import (NO_A, PALINDROME, TWO_BUBBLES, check_x, graph_tuple, haplotype, long_read, mixed_reads, noisy, rand_bases, run_batch_strands,
                              with_bad_base, wrong_strand_read_that_scores_above_zero)

pytestmark = pytest.mark.gpu
XSTRANDS = (76, 77, 82)
SMALL = {"k_gap_pick_out", "k_gap_seed_pick", "k_gap_xstrands_duel", "k_gap_xstrands_mark"}


def winners(reads, exp):
    """The sequence that was traced, per read with a record."""
    return [V.rc(X.canonical(rd)) if e["strand"] == "-" else X.canonical(rd) for rd, e in zip(reads, exp) if e["text"]]


def check_traced_as_mode_50(gg, reads, mode, res, exp):
    """Identity with mode m + 50 of the same build: the winning strands' sequences, submitted by themselves, give the same lines
    (column 5 apart) and the same traceback cells — in a batch of the same length class."""
    seqs = winners(reads, exp)
    assert (max(len(s) for s in seqs) > 2047) == (max(len(r) for r in reads) > 2047)
    base = run_batch_strands(gg, seqs, mode - 20)
    mine = [(i, t) for i, t in enumerate(res["texts"]) if t]
    assert len(mine) == len(seqs)
    for (i, t), b in zip(mine, base["texts"]):
        b = b.split("\t")
        b[0], b[4] = "r%d" % i, exp[i]["strand"]
        assert t == "\t".join(b), (mode, i)
    assert res["cells"][1] - res["cells"][0] == base["cells"][1] - base["cells"][0]
    return base


def same_bytes(a, b):
    return (a["texts"], a["status"], a["score"], a["strand"], a["query"]) == (b["texts"], b["status"], b["score"], b["strand"], b["query"])


@pytest.mark.parametrize("amb", [0, 4])
@pytest.mark.parametrize("mode", [76, 77])
def test_mixed_batch(mode, amb):
    """Forward reads, reverse reads, a 1-base read, N only, a bad base (never picked twice), a reverse palindrome (a tie: '+'), and in
    mode 77 the wrong-strand read that scores >= 0 forward and must stay forward; amb_mode 4 is redundant.  The bytes of mode m + 20."""
    from recgraph_amd import api
    graph = haplotype(300, 3)
    reads = list(mixed_reads(mode - 50))
    res = run_batch_strands(graph[1], reads, mode, amb=amb)
    exp = check_x(graph, reads, mode, res)
    assert [e["strand"] for e in exp[:4] + exp[5:10]] == ["+", "+", "-", "-", "+", " ", "+", "-", "+"], [e["strand"] for e in exp]
    assert res["status"][6] == api.READ_BAD_BASE and res["texts"][6] == "" and exp[6]["picked"] == []
    if mode == 77:
        rd, f, r = wrong_strand_read_that_scores_above_zero()
        assert exp[10]["picked"] == ["+"] and res["strand"][10] == "+" and res["score"][10] == f and r > f >= 0
    assert same_bytes(res, run_batch_strands(graph[1], reads, mode - 50, amb=amb))
    # two picks, ONE traceback, no merge and no second op area to merge from
    st = res["stats"]
    assert st["k_gap_score"] == 2 and st["k_gap_pick"] == 2 and st["k_gap_pick_out"] == 2 and st["k_gap_dirs"] == 1 and st["k_gap_trace"] == 1
    assert st["k_strand_gate"] == st["k_revcomp"] == st["k_gap_xstrands_duel"] == st["k_gap_seed_pick"] == st["k_gap_xstrands_mark"] == st["k_strand_orient"] == 1
    assert "k_strand_merge" not in st and "k_gap_strands_gate" not in st and "k_strand_vote" not in st
    check_traced_as_mode_50(graph[1], reads, mode, res, exp)


@functools.lru_cache(maxsize=None)
def _near_palindrome_graph():
    """A bubble graph whose path p0 is A + rc(A) but for two bases of the second half, and p0's reverse complement as the read: on the
    forward strand it meets four mismatches in 80 columns (a score >= 0 in the global rule too), on the reverse strand none."""
    a = rand_bases(np.random.default_rng(76), 40)
    b = list(V.rc(a))
    for q in (5, 20):
        b[q] = "ACGT"[("ACGT".index(b[q]) + 1) % 4]
    p = a + "".join(b)
    alt = "ACGT"[("ACGT".index(p[50]) + 2) % 4]
    gfa = ("S\t1\t%s\nS\t2\t%s\nS\t3\t%s\nS\t4\t%s\n" % (p[:50], p[50], alt, p[51:]) +
           "".join("L\t%d\t+\t%d\t+\t0M\n" % ab for ab in [(1, 2), (1, 3), (2, 4), (3, 4)]) + "P\tp0\t1+,2+,4+\t*\nP\tp1\t1+,3+,4+\t*\n")
    return graph_tuple(gfa), p


@pytest.mark.parametrize("mode", [76, 77])
def test_the_wrong_strand_read_that_scores_above_zero_stays_forward(mode):
    """Modes 76 AND 77 (mixed_reads has such a read for the semiglobal rule only: no piece of a random 300-row path scores >= 0
    globally against the whole path on the wrong strand).  The exact rule never picks the reverse strand of this read, although it
    would score higher; the vote sends it there first."""
    graph, p = _near_palindrome_graph()
    gg, lnz, rows = graph[1], graph[2], graph[3]
    rd = V.rc(p)
    f, r = R.align(lnz, rows, rd, semi=mode == 77)[0], R.align(lnz, rows, p, semi=mode == 77)[0]
    assert r > f >= 0, (f, r)
    reads = [rd, p, V.rc(p[:60])]
    res = run_batch_strands(gg, reads, mode)
    exp = check_x(graph, reads, mode, res)
    assert exp[0]["picked"] == ["+"] and res["strand"][0] == "+" and res["score"][0] == f
    assert exp[1]["picked"] == ["+"] and res["score"][1] == r
    assert same_bytes(res, run_batch_strands(gg, reads, mode - 50))
    check_traced_as_mode_50(gg, reads, mode, res, exp)


def _edge_reads(mode, longest):
    """(graph, the read of exactly `longest` bases on its own strand, two 150-base reads on theirs).  Paths of about 2200 rows for
    2047 | 2048, so that the long read scores >= 0 on its own strand in the global rule too and modes 76 / 77 leave it out of the
    second pick; paths of 300 rows for 4096 | 4097, where rows x columns of 2200-row paths would be beyond the rule's budget."""
    rng = np.random.default_rng(longest + mode)
    if longest < 4096:
        graph = haplotype(2200)
        w = graph[0].path_sequence(1)
        long_rd = noisy(rng, w[:longest], every=53)
        w0 = graph[0].path_sequence(0)
        short = [noisy(rng, w0[700 * k + 20: 700 * k + 170], every=37) for k in range(2)]
    else:
        graph = haplotype(300, 3)
        w = graph[0].path_sequence(1)
        left = 1900 + int(rng.integers(0, 40))           # the piece crosses 2047 | 2048; the flank behind it crosses 4095 | 4096
        long_rd = rand_bases(rng, left) + noisy(rng, w) + rand_bases(rng, longest - left - len(w))
        short = [noisy(rng, graph[0].path_sequence(2 * k)[20:170], every=37) for k in range(2)]
    assert len(long_rd) == longest and [len(s) for s in short] == [150, 150]
    return graph, long_rd, short


@pytest.mark.parametrize("longest", [2047, 2048, 4096, 4097])
@pytest.mark.parametrize("mode", XSTRANDS)
def test_length_class_edges(mode, longest):
    """The longest read at 2047 | 2048 bases, where every stage switches between the one-wave kernels and the striped ones — each by
    its own longest read: PICK(A) and TRACE by the batch's, PICK(B) by the gate's max_len — and at 4096 | 4097, where a third
    stripe begins and the walk of a seeded ReadState crosses into it.  The long read is given on the forward strand and on the
    reverse strand.  Forward, in modes 76 / 77 on the long paths: it scores >= 0 and stays out of PICK(B), whose longest read has 150
    bases.  Mode 82 picks every read twice, so there a long read with a bad base, which is picked on neither strand, puts PICK(B)
    below the edge while PICK(A) and TRACE are above it.  Every batch: the rule, the bytes of mode m + 20, the lines of mode m + 50,
    and the stage kernels from the launch log."""
    graph, long_rd, short = _edge_reads(mode, longest)
    gg = graph[1]
    kind = {76: 0, 77: 1, 82: 2}[mode]
    local = mode == 82
    S = (longest + 2048) // 2048
    striped = longest > 2047
    assert S == {2047: 1, 2048: 2, 4096: 3, 4097: 3}[longest]
    one_wave = "rg::k_gap_score_local<" if local else "rg::k_gap_score<"
    walk = "rg::k_gap_walk_local_long" if local else "rg::k_gap_walk_long"
    batches = [("forward", [V.rc(short[0]), long_rd, short[1]]), ("reverse", [short[0], V.rc(long_rd), V.rc(short[1])])]
    if local:
        batches.append(("bad base", [short[0], with_bad_base(long_rd), V.rc(short[1])]))
    for side, reads in batches:
        res = run_batch_strands(gg, reads, mode, log=True)
        exp = check_x(graph, reads, mode, res)
        if side == "bad base":
            assert exp[1]["picked"] == [] and [e["strand"] for e in exp] == ["+", " ", "-"]
        else:
            assert [e["strand"] for e in exp] == (["-", "+", "+"] if side == "forward" else ["+", "-", "-"]), (side, [e["strand"] for e in exp])
        if not local and longest < 4096:
            assert exp[1]["picked"] == (["+"] if side == "forward" else ["+", "-"]), (side, exp[1]["picked"], exp[1]["score"])
        # the longest read of the second pick, from the rule: on which side of the edge PICK(B) is
        b_longest = max(len(rd) for rd, e in zip(reads, exp) if len(e["picked"]) == 2)
        inst = res["inst"]
        n_long = int(striped) + int(b_longest > 2047)
        assert inst.get("rg::k_gap_score_long<%d>" % kind, 0) == n_long, (side, sorted(inst))
        base = [k for k in inst if k.startswith(one_wave)]
        assert sum(inst[k] for k in base) == 2 - n_long, (side, sorted(inst))
        assert inst.get("rg::k_gap_pick_local" if local else "rg::k_gap_pick") == 2 and inst.get("rg::k_gap_pick_out") == 2
        assert inst.get("rg::k_gap_seed_pick") == 1 and inst.get("rg::k_gap_xstrands_duel") == 1 and inst.get("rg::k_gap_xstrands_mark") == 1
        one_wave_trace = [k for k in inst if k.startswith("rg::k_gap_dirs") or k.startswith("rg::k_gap_trace")]
        if striped:
            assert not one_wave_trace, (side, sorted(inst))
            assert inst.get("rg::k_gap_ckpt_long<%d>" % kind) == 1 and inst.get("rg::k_gap_redo_long<%d>" % kind) == S and inst.get(walk) == S, (side, sorted(inst))
        else:
            assert len(one_wave_trace) == 2 and all(inst[k] == 1 for k in one_wave_trace), (side, sorted(inst))
            assert not [k for k in inst if k.endswith("_long") or "_long<" in k], (side, sorted(inst))
        assert same_bytes(res, run_batch_strands(gg, reads, mode - 50)), side
        if side != "bad base":          # (without the long read its winners are a batch of another length class)
            check_traced_as_mode_50(gg, reads, mode, res, exp)


@pytest.mark.parametrize("mode", [76, 77])
def test_pass_b_empty_and_pass_b_full(mode):
    """No forward score below 0: the bytes and BOTH counters of mode m + 50, and no duel.  Every read on the other strand: '-', the
    lines of mode m + 50 on the reverse complements, its counters plus the forward score cells."""
    graph = haplotype(300, 3)
    g, gg, lnz, rows, _ = graph
    rng = np.random.default_rng(mode)
    w = [g.path_sequence(k) for k in range(3)]
    fwd = [noisy(rng, w[k]) for k in range(3)] if mode == 76 else [noisy(rng, w[0]), w[1][30:180], w[2][100:160], w[0][5:60]]
    res = run_batch_strands(gg, fwd, mode)
    exp = check_x(graph, fwd, mode, res)
    assert all(e["score"] >= 0 and e["picked"] == ["+"] for e in exp)
    base = run_batch_strands(gg, fwd, mode - 20)
    assert same_bytes(res, base) and res["cells"] == base["cells"]
    assert "k_gap_xstrands_duel" not in res["stats"] and res["stats"]["k_strand_gate"] == 1 and res["stats"]["k_gap_score"] == 1
    assert res["stats"]["k_gap_pick_out"] == 1 and res["stats"]["k_gap_trace"] == 1
    rev = [V.rc(r) for r in fwd]
    res = run_batch_strands(gg, rev, mode)
    exp = check_x(graph, rev, mode, res)
    assert [e["strand"] for e in exp] == ["-"] * len(rev) and all(t.split("\t")[4] == "-" for t in res["texts"])
    assert [V.minus(t) for t in base["texts"]] == res["texts"] and res["score"] == base["score"]
    fwd_score_cells = sum(len(r) for r in rows) * sum(len(r) for r in rev)
    assert res["cells"] == (base["cells"][0] + fwd_score_cells, base["cells"][1] + fwd_score_cells)
    assert res["stats"]["k_gap_xstrands_duel"] == 1 and res["stats"]["k_gap_score"] == 2 and res["stats"]["k_gap_trace"] == 1


@pytest.mark.parametrize("mode", [76, 77])
def test_the_stages_run_in_different_length_classes(mode):
    graph = haplotype(2200)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(40 + mode)
    w = g.path_sequence(0)
    short = [noisy(rng, w[300 * k + 20: 300 * k + 170], every=37) for k in range(4)]
    kind = mode - 76
    # (a) the first pick striped (the 2100-base read is on the forward strand and stays there), the second on the base kernels, the trace striped
    reads = [V.rc(short[0]), long_read(), V.rc(short[1]), V.rc(short[2]), short[3]]
    res = run_batch_strands(gg, reads, mode, log=True)
    exp = check_x(graph, reads, mode, res)
    assert [e["strand"] for e in exp] == ["-", "+", "-", "-", "+"] and exp[1]["picked"] == ["+"]
    assert max(len(reads[i]) for i, e in enumerate(exp) if len(e["picked"]) == 2) == 150
    inst = res["inst"]
    assert inst.get("rg::k_gap_score_long<%d>" % kind) == 1 and inst.get("rg::k_gap_ckpt_long<%d>" % kind) == 1, sorted(inst)
    base = [k for k in inst if k.startswith("rg::k_gap_score<")]
    assert len(base) == 1 and inst[base[0]] == 1, sorted(inst)
    assert not [k for k in inst if k.startswith("rg::k_gap_dirs") or k.startswith("rg::k_gap_trace")], sorted(inst)
    assert inst.get("rg::k_gap_redo_long<%d>" % kind) == 2 and inst.get("rg::k_gap_walk_long") == 2
    assert inst.get("rg::k_gap_pick_out") == 2 and inst.get("rg::k_gap_seed_pick") == 1 and inst.get("rg::k_gap_xstrands_duel") == 1
    assert same_bytes(res, run_batch_strands(gg, reads, mode - 50))
    # (b) the 2100-base read on the reverse strand: both picks striped
    reads = [short[0], V.rc(long_read()), short[1]]
    res = run_batch_strands(gg, reads, mode, log=True)
    exp = check_x(graph, reads, mode, res)
    assert exp[1]["strand"] == "-" and exp[1]["picked"] == ["+", "-"]
    inst = res["inst"]
    assert inst.get("rg::k_gap_score_long<%d>" % kind) == 2 and inst.get("rg::k_gap_ckpt_long<%d>" % kind) == 1, sorted(inst)
    assert not [k for k in inst if k.startswith("rg::k_gap_score<")], sorted(inst)
    assert same_bytes(res, run_batch_strands(gg, reads, mode - 50))
    # (c) the other way round under the vote: the long read goes reverse FIRST and stays; the short reads' second pick is the base kernels'
    kmers = V.kmer_set([g.path_sequence(k) for k in range(len(g.paths))])
    reads = [V.rc(long_read()), rand_bases(rng, 150), short[2]]
    assert V.first_reverse(kmers, reads[0])
    res = run_batch_strands(gg, reads, mode, amb=12, log=True)
    exp = check_x(graph, reads, mode, res, kmers=kmers)
    assert exp[0]["picked"] == ["-"] and exp[0]["strand"] == "-" and exp[1]["picked"] == ["+", "-"] and exp[2]["picked"][0] == "+" and exp[2]["strand"] == "+"
    inst = res["inst"]
    assert inst.get("rg::k_gap_score_long<%d>" % kind) == 1 and len([k for k in inst if k.startswith("rg::k_gap_score<")]) == 1, sorted(inst)
    assert inst.get("rg::k_strand_orient") == 2 and inst.get("rg::k_strand_vote") == 1


def test_local_both_strands():
    """Mode 82 with flanks, a reverse palindrome, an N-only read, a bad base: the bytes of mode 32, one traceback."""
    from recgraph_amd import api
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(32)
    w = [g.path_sequence(k) for k in range(3)]
    flanked = [rand_bases(rng, 15) + noisy(rng, w[k][40 + 10 * k: 190 + 10 * k], every=31) + rand_bases(rng, 15) for k in range(3)]
    reads = [flanked[0], V.rc(flanked[1]), V.rc(flanked[2]), PALINDROME, "N" * 30, with_bad_base(w[0][10:90]), "A", w[1][100:130]]
    res = run_batch_strands(gg, reads, 82, log=True)
    exp = check_x(graph, reads, 82, res)
    assert [e["strand"] for e in exp[:3]] == ["+", "-", "-"] and exp[3]["strand"] in "+ " and exp[7]["strand"] == "+"
    for i in range(3):
        qs, qe = res["query"][i]        # in the coordinates of the strand that won: the flanks are clipped on both sides
        assert 10 <= qs <= 20 and 160 <= qe <= 170, (i, qs, qe)
    assert (res["status"][4], res["texts"][4], exp[4]["picked"]) == (api.READ_UNALIGNED, "", ["+", "-"])
    assert res["status"][5] == api.READ_BAD_BASE and exp[5]["picked"] == []
    inst, st = res["inst"], res["stats"]
    assert inst.get("rg::k_gap_strands_gate") == 1 and "rg::k_strand_gate" not in inst and "rg::k_strand_merge" not in inst, sorted(inst)
    assert st["k_gap_score_local"] == 2 and st["k_gap_pick_local"] == 2 and st["k_gap_dirs_local"] == 1 and st["k_gap_trace_local"] == 1
    assert set(inst) >= {"rg::" + k for k in SMALL} and inst["rg::k_gap_pick_out"] == 2
    again = run_batch_strands(gg, reads, 82, amb=4)
    assert same_bytes(again, res) and again["cells"] == res["cells"]
    assert same_bytes(res, run_batch_strands(gg, reads, 32))
    check_traced_as_mode_50(gg, reads, 82, res, exp)


def test_local_forward_unaligned_and_reverse_aligned():
    from recgraph_amd import api
    graph = graph_tuple(NO_A)
    gg = graph[1]
    reads = ["AAAAAA", "TTTTTT", "AAAA", "NNN"]
    res = run_batch_strands(gg, reads, 82)
    exp = check_x(graph, reads, 82, res)
    assert [(e["status"], e["strand"]) for e in exp] == [(0, "-"), (0, "+"), (0, "-"), (api.READ_UNALIGNED, " ")]
    assert res["score"] == [12, 12, 8, 0] and res["strand"] == ["-", "+", "-", None] and res["status"] == [0, 0, 0, api.READ_UNALIGNED]
    assert res["texts"][0].split("\t")[1:] == V.minus(res["texts"][1]).split("\t")[1:]
    assert same_bytes(res, run_batch_strands(gg, reads, 32))


@pytest.mark.parametrize("mode", [76, 77])
def test_strand_vote(mode):
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(120 + mode - 50)
    w = [g.path_sequence(k) for k in range(3)]
    kmers = V.kmer_set(w)
    short = w[0][5:12]
    good_rev = V.rc(noisy(rng, w[0], every=61)) if mode == 76 else V.rc(w[1][40:190])
    chimera = w[0][100:140] + V.rc(w[1][50:200])                       # its forward piece is the shorter one: the vote sends it reverse first
    hopeless_rev = V.rc(w[2][50:90]) + rand_bases(rng, 200)                  # reverse first, below 0 there: the forward strand is picked too
    reads = [short, good_rev, chimera, hopeless_rev, noisy(rng, w[2]), V.rc(noisy(rng, w[1])), "N" * 40, with_bad_base(w[0][:80]), w[1][10:150]]
    res = run_batch_strands(gg, reads, mode, amb=12)
    exp = check_x(graph, reads, mode, res, kmers=kmers)           # (the counters: every picked strand's score cells, one traceback)
    assert exp[0]["picked"][0] == "+"                                 # votes 0 / 0: forward first
    assert exp[1]["strand"] == "-" and exp[1]["picked"] == ["-"] and exp[1]["score"] >= 0
    assert exp[2]["picked"][0] == "-" and exp[3]["picked"] == ["-", "+"] and exp[7]["picked"] == []
    st = res["stats"]
    assert st["k_strand_vote"] == 1 and st["k_strand_orient"] == 2 and st["k_strand_gate"] == 1 and st["k_gap_trace"] == 1
    assert same_bytes(res, run_batch_strands(gg, reads, mode - 50, amb=12))
    # the exact rule on the same reads picks other strands, and counts them
    exact = run_batch_strands(gg, reads, mode)
    exp0 = check_x(graph, reads, mode, exact)
    assert [e["picked"] for e in exp0] != [e["picked"] for e in exp]


def test_a_reverse_winner_whose_walk_starts_in_a_middle_stripe():
    """Mode 82, five stripes: the piece lies in stripe 2 of the reverse complement, so the higher rounds do nothing for it; a second
    read's piece lies in stripe 0 on the forward strand."""
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(82)
    piece = g.path_sequence(1)[20:280]
    own = rand_bases(rng, 4500) + piece + rand_bases(rng, 9300 - 4500 - len(piece))          # the strand on which it aligns
    reads = [V.rc(own), g.path_sequence(2)[10:200] + rand_bases(rng, 3000)]
    res = run_batch_strands(gg, reads, 82)
    exp = check_x(graph, reads, 82, res)
    assert [e["strand"] for e in exp] == ["-", "+"]
    qs, qe = res["query"][0]
    assert qs // 2048 == qe // 2048 == 2 and 4480 <= qs <= 4520, (qs, qe)
    st = res["stats"]
    assert st["k_gap_score_long"] == 2 and st["k_gap_ckpt_long"] == 1 and st["k_gap_redo_long"] == 5 and st["k_gap_walk_local_long"] == 5
    check_traced_as_mode_50(gg, reads, 82, res, exp)


@pytest.mark.parametrize("mode", XSTRANDS)
def test_beyond_the_old_limit(mode):
    """16384, 40000, 131071 and 5 bases in one batch on the hand graph of five rows, given on either strand: 64 stripes, the walks
    start in different rounds, and every line is mode m + 50's of the strand that won."""
    from recgraph_amd import api
    graph = graph_tuple(TWO_BUBBLES)
    gg, lnz, rows = graph[1:4]
    rng = np.random.default_rng(1000 + mode)
    p0, p1 = ("".join(lnz[r] for r in pr) for pr in rows)
    # one strand of each long read holds a path and no G or C beside it (forward) / no C or G (its complement): the other strand aligns worse
    at = lambda n, left, p: rand_bases(rng, left, "AT") + p + rand_bases(rng, n - left - len(p), "AT")
    reads = [V.rc(at(16384, 9000, p0)), at(131071, 70000, p1), V.rc(at(40000, 39000, p1)), "ATGCT"]
    assert [len(r) for r in reads] == [16384, 131071, 40000, 5]
    res = run_batch_strands(gg, reads, mode)
    exp = check_x(graph, reads, mode, res)
    assert len({e["strand"] for e in exp}) == 2, [e["strand"] for e in exp]
    st = res["stats"]
    assert st["k_gap_ckpt_long"] == 1 and st["k_gap_redo_long"] == 64 and st["k_gap_score_long"] == 2 and "k_gap_dirs_long" not in st
    check_traced_as_mode_50(gg, reads, mode, res, exp)
    with pytest.raises(api._lib.RecGraphError):
        run_batch_strands(gg, reads[:1], mode - 50)          # what modes 26 / 27 / 32 do not take


def test_traced_once():
    """Mode 82 on a striped batch: the score pass twice, the checkpoint pass, the rebuilds and the walks once per chunk / stripe.
    All reads win forward: performed(82) - performed(62) == counted(62), exactly the second score pass.  All reads win on reverse:
    the counters of mode 62 on the reverse complements plus the forward score cells."""
    graph = haplotype(300, 3)
    g, gg, lnz, rows, _ = graph
    rng = np.random.default_rng(8262)
    w = [g.path_sequence(k) for k in range(3)]
    fwd = [rand_bases(rng, 1000 + 700 * k) + noisy(rng, w[k][30:260]) + rand_bases(rng, 3000 - 400 * k) for k in range(3)] + [w[0][50:150]]
    S = (max(len(r) for r in fwd) + 2048) // 2048
    assert S == 3
    res = run_batch_strands(gg, fwd, 82)
    exp = check_x(graph, fwd, 82, res)
    assert [e["strand"] for e in exp] == ["+"] * 4 and all(e["picked"] == ["+", "-"] for e in exp)
    st = res["stats"]
    assert st["k_gap_score_long"] == 2 and st["k_gap_pick_local"] == 2
    assert st["k_gap_ckpt_long"] == 1 and st["k_gap_redo_long"] == S and st["k_gap_walk_local_long"] == S
    base = run_batch_strands(gg, fwd, 62)
    assert same_bytes(res, base)
    assert res["cells"][1] - base["cells"][1] == base["cells"][0] and res["cells"][0] == 2 * base["cells"][0]
    rev = [V.rc(r) for r in fwd]
    res = run_batch_strands(gg, rev, 82)
    exp = check_x(graph, rev, 82, res)
    assert [e["strand"] for e in exp] == ["-"] * 4
    assert res["texts"] == [V.minus(t) for t in base["texts"]]
    assert res["cells"] == (2 * base["cells"][0], base["cells"][1] + base["cells"][0])
    st = res["stats"]
    assert st["k_gap_score_long"] == 2 and st["k_gap_ckpt_long"] == 1 and st["k_gap_redo_long"] == S and st["k_gap_walk_local_long"] == S


def test_65_paths():
    from recgraph_amd import api, synth
    g = synth.random_dag_graph(60, 65, seed=105)
    g.paths[64] = list(g.paths[3])
    used = {i for p in g.paths for i in p}
    g = synth.SynthGraph([(i, s) for i, s in g.segments if i in used], [(a, b) for a, b in g.links if a in used and b in used], g.paths)
    graph = graph_tuple(g)
    gg = graph[1]
    rng = np.random.default_rng(65)
    w = g.path_sequence(64)
    reads = [V.rc(rand_bases(rng, 1000) + w + rand_bases(rng, 2100 - 1000 - len(w))), rand_bases(rng, 2070) + w, V.rc(w[3:40])]
    for mode in XSTRANDS:
        res = run_batch_strands(gg, reads, mode)
        exp = check_x(graph, reads, mode, res)
        assert exp[0]["strand"] == "-" or mode != 82
    seqs = [g.path_sequence(q) for q in range(65)]
    best = int(re.search(r"best path: (\d+)", res["texts"][0]).group(1))
    assert seqs[best] == w and best == seqs.index(w) and best < 64         # the lowest of the identical paths, on the reverse strand too


@pytest.mark.parametrize("mode", [76, 82])
def test_stream_multi_and_the_wrappers_give_the_batch_text(mode):
    from recgraph_amd import api
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(mode)
    reads = list(mixed_reads(26)) + [V.rc(rand_bases(rng, 1500) + noisy(rng, g.path_sequence(1)) + rand_bases(rng, 700))]
    names = ["r%d" % i for i in range(len(reads))]
    res = run_batch_strands(gg, reads, mode)
    check_x(graph, reads, mode, res)
    for kw in ({}, {"both_strands": True}):
        assert api.align_batch(gg, reads, names, mode=mode, **kw) == (res["texts"], res["status"])
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4, **kw)
        assert list(st) == res["texts"] and list(sstatus) == res["status"]
        mt, mstatus = api.align_batch_multi(gg, reads, names, mode=mode, device_ids=[0], **kw)
        assert mt == res["texts"] and mstatus == res["status"]
    st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], tile_reads=3, amb_strand=True)       # (`-s true` stays ignored)
    assert list(st) == res["texts"] and list(sstatus) == res["status"]
    if mode == 82:
        with pytest.raises(api._lib.RecGraphError) as ex:
            api.Stream(gg, api.make_params(82), device_ids=[0], strand_vote=True)
        assert ex.value.code == -1 and "hopeless" in str(ex.value)          # RG_ERR_ARG, and the message says why
        with pytest.raises(api._lib.RecGraphError):
            api.Batch(gg, reads, api.make_params(82, amb=12))
        one = api.pathwise_alignment_gap_local_exec(["$"] + list(reads[3]), gg, very_long_both_strands=True)
        assert one.strand == "-" and one.to_string() == res["texts"][3].replace("r3\t", "Temp\t", 1).rstrip("\n")
    else:
        vote = run_batch_strands(gg, reads, mode, amb=12)
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4, strand_vote=True)
        assert list(st) == vote["texts"] and list(sstatus) == vote["status"]
        assert api.align_batch(gg, reads, names, mode=mode, strand_vote=True) == (vote["texts"], vote["status"])
        one = api.pathwise_alignment_gap_exec(["$"] + list(reads[2]), gg, very_long_both_strands=True)
        assert one.strand == "-" and one.to_string() == res["texts"][2].replace("r2\t", "Temp\t", 1).rstrip("\n")
        one = api.pathwise_alignment_gap_semi_exec(["$"] + list(reads[3]), gg, very_long_both_strands=True)
        assert one.to_string() == api.align_batch(gg, [reads[3]], ["Temp"], mode=77)[0][0].rstrip("\n")


def test_the_cli_runs_the_modes(tmp_path, capsys):
    from recgraph_amd import api, cli
    g, gg = haplotype(300, 3)[:2]
    rng = np.random.default_rng(7682)
    long_rd = rand_bases(rng, 12000) + g.path_sequence(1) + rand_bases(rng, 20000 - 12000 - len(g.path_sequence(1)))
    reads = [g.path_sequence(0)[20:170], "NNNN", V.rc(g.path_sequence(1)[20:170]), V.rc(long_rd)]
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fa").write_text("".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    for m, flags in ((77, []), (77, ["--strand-vote"]), (76, ["--both-strands"]), (82, ["--both-strands"])):
        exp, st = api.align_batch(gg, reads, ["s%d" % i for i in range(4)], mode=m, strand_vote="--strand-vote" in flags)
        assert exp[2].split("\t")[4] == "-" and exp[3].split("\t")[4] == "-"
        cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", str(m), "--devices", "0"] + flags)
        assert capsys.readouterr().out == "".join(exp)
    out = tmp_path / "out.gaf"
    cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", "82", "--devices", "0", "-o", str(out)])
    assert len(out.read_text().splitlines()) == 3
