"""The affine-gap pathwise families on the GPU away from match 2, mismatch -4, o = -4, e = -2 (tests/pathwise_gap_scores.py has the
scorings, the shapes and the searches; tests/test_pathwise_gap_scores_cpu.py checks their preconditions from the rules alone).
Every comparison is exact: bytes and integers against the numpy rules.

A. Both strands (modes 26 / 27 / 32 and 76 / 77 / 82) at six ordinary scorings: "align the other strand iff the first score is < 0,
   keep the reverse record iff strictly greater" depends on the scoring alone — unit costs give scores of exactly 0 on either strand,
   (3, 0, 0, 0) has no negative score at all, (-40, -1) and HOXD70 with (-400, -30) make every inexact read negative.
B. The edge of the admitted score range, (rows + n) * max(|sc|, |o + e|) < 2^28, in every kernel file: every length class of modes
   6 / 7 / 12 and two and three stripes of modes 16 / 17 / 22 and 56 / 57 / 62, on paths of five rows (scores near -2^28, e * j of the
   padding columns beyond it) and on paths of n rows (scores near +2^27), under E1, E2 and E3.  The launch log says which
   instantiation ran; the names are keys of the kernel matrices.
C. Strand scores that differ by less than an f32 ulp (|score| near 2^26 .. 2^27): the reverse record must win by the integers."""
import numpy as np
import pytest

import kernel_matrix_gap as KG
import kernel_matrix_gap_local as KL
import kernel_matrix_gap_long as KLONG
import kernel_matrix_gap_xlong as KX
import pathwise_gap_scores as G
import strand_vote_rule as V
from pathwise_support import (align, check_mode, check_strands, check_x, haplotype, long_read, noisy, run_batch, run_batch_strands)

pytestmark = pytest.mark.gpu
STRANDS, XSTRANDS = (26, 27, 32), (76, 77, 82)
COLUMNS_PER_LANE = {255: 4, 256: 8, 512: 16, 1024: 32, 2047: 32}


def _both(graph, reads, mode, scoring, kmers=None, **kw):
    """One both-strands batch at scoring = (scores, o, e), checked read by read; returns (the batch, [(text, strand, strands aligned)])."""
    scores, o, e = scoring
    reads = list(reads)
    res = run_batch_strands(graph[1], reads, mode, scores=scores, o=o, e=e, **kw)
    if mode in STRANDS:
        exp = check_strands(graph, reads, mode, res, kmers=kmers, scores=scores, o=o, e=e)
        return res, [(x[0], x[2], x[3]) for x in exp]
    exp = check_x(graph, reads, mode, res, kmers=kmers, scores=scores, o=o, e=e)
    return res, [(x["text"], x["strand"], x["picked"]) for x in exp]


def _same_bytes(a, b):
    return (a["texts"], a["status"], a["score"]) == (b["texts"], b["status"], b["score"])


# ---- A. both strands off the defaults ----

@pytest.mark.parametrize("name", sorted(G.ORDINARY))
@pytest.mark.parametrize("mode", STRANDS + XSTRANDS)
def test_both_strands_at_an_ordinary_scoring(mode, name):
    graph = haplotype(300, 3)
    reads = G.strand_reads(mode)
    scoring = G.ordinary(name)
    res, answers = _both(graph, reads, mode, scoring)
    G.assert_conditions(mode, name, answers)
    if name == "non-negative" and mode not in (32, 82):
        # no score below 0: the second strand of no read is looked at, and the bytes are those of the reads as given
        base = run_batch_strands(graph[1], list(reads), mode - 10 if mode in STRANDS else mode - 20, scores=scoring[0], o=scoring[1], e=scoring[2])
        assert _same_bytes(res, base) and base["strand"] == res["strand"]
        assert "k_strand_merge" not in res["stats"] and "k_gap_xstrands_duel" not in res["stats"] and res["stats"]["k_strand_gate"] == 1, res["stats"]
        assert res["stats"]["k_gap_score"] == 1
    if mode in XSTRANDS:
        assert _same_bytes(res, run_batch_strands(graph[1], list(reads), mode - 50, scores=scoring[0], o=scoring[1], e=scoring[2]))


@pytest.mark.parametrize("mode", STRANDS + XSTRANDS)
def test_a_striped_batch_at_steep_gaps(mode):
    """o = -40, e = -1 with the 2100-base read on the reverse strand: both passes (picks) run the striped kernels."""
    graph = haplotype(2200)
    rng = np.random.default_rng(40 + mode)
    w = graph[0].path_sequence(0)
    short = [noisy(rng, w[300 * k + 20: 300 * k + 170], every=37) for k in range(2)]
    reads = [short[0], V.rc(long_read()), V.rc(short[1])]
    res, answers = _both(graph, reads, mode, G.ordinary("steep"), log=True)
    assert [a[1] for a in answers] == ["+", "-", "-"] and answers[1][2] == ["+", "-"], [a[1:] for a in answers]
    kind = {6: 0, 7: 1, 2: 2}[mode % 10]
    assert res["inst"].get("rg::k_gap_score_long<%d>" % kind) == 2, sorted(res["inst"])
    assert not [k for k in res["inst"] if k.startswith("rg::k_gap_score<") or k.startswith("rg::k_gap_score_local<")], sorted(res["inst"])


@pytest.mark.parametrize("mode", [26, 27, 76, 77])
def test_the_vote_at_extend_only_gaps(mode):
    graph = haplotype(300, 3)
    reads = G.strand_reads(mode)
    kmers = V.kmer_set([graph[0].path_sequence(k) for k in range(3)])
    res, answers = _both(graph, reads, mode, G.ordinary("extend-only"), kmers=kmers, amb=12)
    firsts = {a[2][0] for a in answers if a[2]}
    assert firsts == {"+", "-"} and any(a[2] == ["-"] for a in answers) and res["stats"]["k_strand_vote"] == 1, [a[1:] for a in answers]
    _, exact = _both(graph, reads, mode, G.ordinary("extend-only"))
    assert [a[2] for a in exact] != [a[2] for a in answers]


# ---- B. the i32 edge ----

def _edge_batch(graph, reads, mode, scoring):
    """One batch of a mode that aligns the reads as given, with the launch log on, checked against the mode's rule."""
    from recgraph_amd import api
    scores, o, e = scoring
    api.set_option("launch_log", 1)
    try:
        run = run_batch(graph[1], list(reads), mode, score_matrix=scores, o=o, e=e)
    finally:
        api.set_option("launch_log", 0)
    check_mode(graph, list(reads), mode, scores, o, e, texts=run.texts, status=run.status)
    return run


def _launched(run, matrix, names, when_traced=()):
    """Every instantiation of `names` ({name: launches}) is a key of the kernel matrix and was launched that often; those of
    `when_traced` as well, when some read has a record to trace."""
    inst = run.instantiations
    for name, count in list(names.items()) + (list(when_traced.items()) if any(run.texts) else []):
        assert name in matrix, (name, sorted(matrix))
        assert inst.get(name) == count, (name, count, sorted(inst.items()))


@pytest.mark.parametrize("name", ["E1", "E2", "E3"])
@pytest.mark.parametrize("kind,n", G.shapes(G.BASE_LENGTHS), ids=lambda v: str(v))
def test_the_edge_in_every_length_class(kind, n, name):
    """Modes 6 / 7 / 12 with the batch's longest read on a class boundary: 255 (4 columns per lane), 256 (8), 512 (16), 1024 and 2047 (32)."""
    graph, reads = G.edge_shape(kind, n)
    scoring = G.edge_scoring(name, graph, reads)
    C = COLUMNS_PER_LANE[n]
    for mode in (6, 7, 12):
        run = _edge_batch(graph, reads, mode, scoring)
        if mode == 12:
            _launched(run, KL.MATRIX, {KL.score(C): 1, "rg::k_gap_pick_local": 1}, {KL.dirs(C): 1, "rg::k_gap_trace_local": 1})
        else:
            _launched(run, KG.MATRIX, {KG.score(C, mode == 7): 1, "rg::k_gap_pick": 1}, {KG.dirs(C, mode == 7): 1, "rg::k_gap_trace": 1})
            assert run.status == [0] * len(reads)
        assert len([k for k in run.instantiations if k.startswith("rg::k_gap_score")]) == 1, sorted(run.instantiations)


@pytest.mark.parametrize("name", ["E1", "E2", "E3"])
@pytest.mark.parametrize("kind,n", G.shapes(G.LONG_LENGTHS), ids=lambda v: str(v))
def test_the_edge_in_the_striped_kernels(kind, n, name):
    """Modes 16 / 17 / 22: 2048 bases (two stripes, column 2048 alone in the second: the rest is padding) and 4097 (three)."""
    graph, reads = G.edge_shape(kind, n)
    scoring = G.edge_scoring(name, graph, reads)
    for k, mode in enumerate((16, 17, 22)):
        run = _edge_batch(graph, reads, mode, scoring)
        _launched(run, KLONG.MATRIX, {"rg::k_gap_score_long<%d>" % k: 1}, {"rg::k_gap_dirs_long<%d>" % k: 1, KLONG.TRACE[mode]: 1})
        assert run.instantiations.get(KLONG.PICK[mode]) == 1
        assert len([k for k in run.instantiations if k.startswith("rg::k_gap_score")]) == 1, sorted(run.instantiations)


@pytest.mark.parametrize("name", ["E1", "E2", "E3"])
@pytest.mark.parametrize("kind,n", G.shapes(G.LONG_LENGTHS), ids=lambda v: str(v))
def test_the_edge_in_the_checkpointed_traceback(kind, n, name):
    """Modes 56 / 57 / 62 on the same shapes: the checkpoints hold H and Y of every 64th row at the edge values; at 2048 bases the
    bytes are those of modes 16 / 17 / 22."""
    graph, reads = G.edge_shape(kind, n)
    scoring = G.edge_scoring(name, graph, reads)
    stripes = (n + 2048) // 2048
    assert stripes == {2048: 2, 4097: 3}[n]
    for k, mode in enumerate((56, 57, 62)):
        run = _edge_batch(graph, reads, mode, scoring)
        _launched(run, KX.MATRIX, {"rg::k_gap_ckpt_long<%d>" % k: 1}, {"rg::k_gap_redo_long<%d>" % k: stripes, KX.WALK[mode]: stripes})
        assert run.instantiations.get(KX.SCORE[mode]) == 1 and run.instantiations.get(KX.PICK[mode]) == 1, sorted(run.instantiations)
        assert not [k for k in run.instantiations if k.startswith("rg::k_gap_dirs") or k.startswith("rg::k_gap_trace")], sorted(run.instantiations)
        if n == 2048:
            assert (run.texts, run.status) == align(graph[1], list(reads), mode - 40, *scoring), mode


@pytest.mark.parametrize("n", [256, 2048])
@pytest.mark.parametrize("family", [20, 70])
def test_both_strands_at_the_edge(family, n):
    """E1 on the flat graph: every score is near -2^28 on either strand, and the strands are told apart by the integers."""
    graph, reads = G.edge_shape("flat", n)
    scoring = G.edge_scoring("E1", graph, reads)
    for mode in (6 + family, 7 + family, 12 + family):
        res, answers = _both(graph, reads, mode, scoring)
        if mode % 10 != 2:
            assert all(a[2] == ["+", "-"] for a in answers) and min(res["score"]) <= -0.95 * G.LIMIT, (mode, res["score"])


# ---- C. strand scores an f32 cannot tell apart ----

def _tie_piece():
    return G.path_bases(G.tie_graph(), 1)[17:17 + G.TIE_BASES]


@pytest.mark.parametrize("mode", STRANDS)
def test_a_reverse_record_that_wins_by_less_than_an_f32_ulp(mode):
    """Forward and reverse scores that differ and are the same f32 (modes 26 / 27: about -9e7 and -4.7e7 under E1; mode 32: about
    8e7 under E4): the reverse record is strictly better and must be kept — and mode m + 50, which compares integers in its own kernel,
    must give the same bytes."""
    found = G.near_tie_reads(mode)
    reads = [rd for rd, _, _ in found] + [_tie_piece()]
    scoring = G.tie_scoring(mode)
    x, _ = _both(G.tie_graph(), reads, mode + 50, scoring)
    res, answers = _both(G.tie_graph(), reads, mode, scoring)
    assert [a[1] for a in answers[:-1]] == ["-"] * len(found) and res["score"][:-1] == [r for _, _, r in found], (res["strand"], res["score"])
    assert res["stats"]["k_strand_merge"] == 1
    assert _same_bytes(res, x) and res["strand"] == x["strand"]


@pytest.mark.parametrize("mode", [26, 27])
def test_a_reverse_first_record_that_stays_by_less_than_an_f32_ulp(mode):
    """The vote sends these reads reverse first; they score below 0 there, so the forward strand is aligned too, scores lower by less
    than an f32 ulp, and must not replace the reverse-first record."""
    found = G.near_tie_vote_reads(mode)
    reads = [rd for rd, _, _ in found] + [_tie_piece()]
    scoring = G.tie_scoring(mode)
    kmers = G.tie_kmers()
    x, _ = _both(G.tie_graph(), reads, mode + 50, scoring, kmers=kmers, amb=12)
    res, answers = _both(G.tie_graph(), reads, mode, scoring, kmers=kmers, amb=12)
    assert [a[1:] for a in answers[:-1]] == [("-", ["-", "+"])] * len(found) and res["score"][:-1] == [r for _, _, r in found], (res["strand"], res["score"])
    assert _same_bytes(res, x) and res["strand"] == x["strand"]


@pytest.mark.parametrize("mode", [32, 82])
def test_the_local_near_tie_reads_at_e2(mode):
    """The same reads under E2, where every local score is a multiple of maxabs (no near tie is possible): the rule's answer."""
    reads = [rd for rd, _, _ in G.near_tie_reads(32)] + [_tie_piece()]
    res, answers = _both(G.tie_graph(), reads, mode, G.edge_scoring("E2", G.tie_graph(), reads))
    assert all(a[2] == ["+", "-"] for a in answers) and max(res["score"]) == G.TIE_BASES * G.maxabs(G.tie_graph(), reads)
