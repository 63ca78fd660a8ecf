"""CPU: the affine-gap pathwise families off the default scores — what tests/test_gpu_pathwise_gap_scores.py takes for granted, checked
from the rules alone (tests/pathwise_gap_scores.py has the scorings, the shapes and the searches).

  * the edge scorings E1 .. E4 of every shape sit exactly on the plan's bound, and rg_batch_create, which answers before a device is
    needed, admits maxabs and refuses maxabs + 1 with RG_ERR_CAPACITY in every family that takes the read length;
  * the numpy rules, whose "no value" is the sentinel -2^29, stay exact at that edge: their scores equal those of a plain scalar
    Gotoh on Python integers with None for "no value", on shapes of at most 1000 cells per path;
  * the corner scores of the edge shapes: every flat class has a score of at most -0.95 * 2^28, every square class one of at least
    0.49 * 2^28 under E2 and under E3;
  * the seeded searches for strand scores that differ and are the same f32 succeed, and why mode 32 needs E4 for them;
  * the conditions of the both-strands batches at the six ordinary scorings hold in the rule's answers."""
import numpy as np
import pytest

import pathwise_gap_scores as G
import pathwise_gap_strands_rule as S
import strand_vote_rule as V
from pathwise_support import create_rc, expect_strands, haplotype, no_device, noisy, rand_bases

RG_ERR_CAPACITY = -5
FAMILIES = {0: 2047, 10: 16383, 20: 16383, 50: 131071, 70: 131071}        # the offset of a family: its longest read
ALL_SHAPES = G.shapes(G.BASE_LENGTHS + G.LONG_LENGTHS)


def _id(shape):
    return "%s-%d" % shape


@pytest.mark.parametrize("shape", ALL_SHAPES + [("tie", 60)], ids=_id)
def test_the_edge_scorings_sit_on_the_bound(shape):
    graph, reads = (G.tie_graph(), ["A" * G.TIE_BASES]) if shape[0] == "tie" else G.edge_shape(*shape)
    steps = G.longest_path(graph) + max(len(r) for r in reads)
    m = G.maxabs(graph, reads)
    assert steps * m < G.LIMIT <= steps * (m + 1), (steps, m)
    if shape[0] == "tie":
        assert m == 1677721
    for name in G.EDGES:
        match, mismatch, o, e = G.edge_values(name, graph, reads)
        scores, o2, e2 = G.edge_scoring(name, graph, reads)
        assert (o2, e2) == (o, e) and o <= 0 and e <= 0
        assert scores[("A", "A")] == match and scores[("A", "C")] == mismatch == scores[("N", "N")]
        acgtn = [v for (a, b), v in scores.items() if "-" not in (a, b)]
        assert max(max(abs(v) for v in acgtn), abs(o + e)) == m, (name, m)


def _small_shapes():
    """(graph, reads) with rows x bases <= 1000 per path: the flat graph with short and long reads, squares with reads as long as the
    paths and with reads several times as long."""
    out = [("flat-200", G.flat(), [rand_bases(np.random.default_rng(q), 200) for q in range(2)] + ["ATGCT"]),
           ("flat-37", G.flat(), [rand_bases(np.random.default_rng(10 + q), 37) for q in range(2)])]
    for rows, n in ((30, 30), (12, 80)):
        graph = G.square(rows)
        rng = np.random.default_rng(rows)
        w0, w1 = G.path_bases(graph, 0), G.path_bases(graph, 1)
        reads = [(w1 * 8)[:n], noisy(rng, (w0 * 8)[:n], every=7), rand_bases(rng, n), G._with_runs(rng, (w1 * 8)[:n])]
        out.append(("square-%dx%d" % (rows, n), graph, reads))
    return out


@pytest.mark.parametrize("name", sorted(G.EDGES))
@pytest.mark.parametrize("shape", _small_shapes(), ids=lambda s: s[0])
def test_the_rules_stay_exact_at_the_edge(shape, name):
    _, graph, reads = shape
    assert G.longest_path(graph) * max(len(r) for r in reads) <= 1000
    scores, o, e = G.edge_scoring(name, graph, reads)
    table = G.table_of(scores)
    seen = set()
    for mode in (6, 7, 12):
        for rd in reads:
            got, want = G.rule_score(graph, rd, mode, table, o, e), G.unbounded_score(graph, rd, mode, table, o, e)
            assert got == want, (name, mode, rd, got, want)
            seen.add(want)
    assert len(seen) > 1, seen


def test_the_unbounded_gotoh_on_hand_cases():
    """ATGCT on the hand graph (paths ATGAT and ACGCT) at the default scores: one mismatch globally, ATG locally; a read of G alone."""
    from recgraph_amd import api
    table = G.table_of(api.create_score_matrix_i32(2, -4))
    assert [G.unbounded_score(G.flat(), "ATGCT", m, table, -4, -2) for m in (6, 7, 12)] == [4, 4, 6]
    assert [G.unbounded_score(G.flat(), "G", m, table, -4, -2) for m in (6, 7, 12)] == [2 + 2 * (-4 - 2 * 2), 2, 2]      # (a gap of two rows on either side)
    zero = G.table_of(api.create_score_matrix_i32(0, -1))
    assert G.unbounded_score(G.flat(), "ATGCT", 12, zero, 0, -1) is None


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_admission_sits_on_the_edge(shape):
    """maxabs is admitted and maxabs + 1 refused, through the matrix (E2: o + e is maxabs too) and through o + e alone."""
    graph, reads = G.edge_shape(*shape)
    n = max(len(r) for r in reads)
    ok = -3 if no_device() else 0
    m = G.maxabs(graph, reads)
    families = [f for f, longest in FAMILIES.items() if n <= longest]
    assert families and (0 in families) == (n <= 2047)
    for f in families:
        for mode in (6 + f, 7 + f, 12 + f):
            for by_matrix in (True, False):
                at = lambda v: create_rc(graph[0], list(reads), mode, match=v if by_matrix else 1, mismatch=-v if by_matrix else -1,
                                         o=0 if by_matrix else -v, e=-1 if by_matrix else 0)
                rc, msg = at(m)
                assert rc == ok, (mode, by_matrix, m, rc, msg)
                rc, msg = at(m + 1)
                assert rc == RG_ERR_CAPACITY and "2^28" in msg, (mode, by_matrix, m + 1, rc, msg)


@pytest.mark.parametrize("n", G.BASE_LENGTHS + G.LONG_LENGTHS)
def test_every_flat_class_has_a_score_near_minus_2_to_the_28(n):
    graph, reads = G.edge_shape("flat", n)
    assert [len(r) for r in reads] == [n] * 3
    low = {}
    for name in ("E1", "E3"):
        scores, o, e = G.edge_scoring(name, graph, reads)
        low[name] = min(G.rule_score(graph, rd, 6, G.table_of(scores), o, e) for rd in reads)
        assert -G.LIMIT < low[name], (name, low)
    assert low["E1"] <= -0.95 * G.LIMIT, low
    assert n < 512 or low["E3"] <= -0.95 * G.LIMIT, low                # (five matches of +maxabs weigh too much against 250 gap columns)


@pytest.mark.parametrize("n", [n for n in G.BASE_LENGTHS + G.LONG_LENGTHS if n <= G.SQUARE_MAX])
def test_every_square_class_has_a_score_near_half_of_2_to_the_28(n):
    graph, reads = G.edge_shape("square", n)
    assert [len(r) for r in reads] == [n] * 3 and reads[0] == G.path_bases(graph, 1) and len(set(reads)) == 3
    for name in ("E2", "E3"):
        scores, o, e = G.edge_scoring(name, graph, reads)
        top = G.rule_score(graph, reads[0], 6, G.table_of(scores), o, e)
        assert top == n * G.maxabs(graph, reads) and 0.49 * G.LIMIT <= top < G.LIMIT, (name, top)


# ---- strand scores an f32 cannot tell apart ----

@pytest.mark.parametrize("mode", [26, 27, 32])
def test_the_search_for_near_ties_succeeds(mode):
    found = G.near_tie_reads(mode)
    assert len(found) >= 3 and len({rd for rd, _, _ in found}) == len(found)
    scores, o, e = G.tie_scoring(mode)
    exp = expect_strands(G.tie_graph(), [rd for rd, _, _ in found], mode, scores=scores, o=o, e=e)
    for (rd, f, r), x in zip(found, exp):
        assert len(rd) == G.TIE_BASES and r > f and np.float32(f) == np.float32(r) and abs(f) > 1 << 24, (mode, f, r)
        assert mode == 32 or f < 0
        # the composed rule takes the reverse record, whose score is r
        assert x[2:] == ("-", ["+", "-"]) and S.score_of(x[0]) == r, (mode, x[1:], f, r)


@pytest.mark.parametrize("mode", [26, 27])
def test_the_search_for_near_ties_under_the_vote_succeeds(mode):
    found = G.near_tie_vote_reads(mode)
    assert len(found) >= 2
    kmers = G.tie_kmers()
    scores, o, e = G.tie_scoring(mode)
    exp = expect_strands(G.tie_graph(), [rd for rd, _, _ in found], mode, kmers, scores=scores, o=o, e=e)
    for (rd, f, r), x in zip(found, exp):
        assert V.first_reverse(kmers, rd) and f < r < 0 and np.float32(f) == np.float32(r), (mode, f, r)
        # reverse first, below 0 there, so the forward strand is aligned too, and the reverse-first record stays
        assert x[2:] == ("-", ["-", "+"]) and S.score_of(x[0]) == r, (mode, x[1:], f, r)


def test_no_edge_scoring_but_e4_can_give_the_local_rule_a_near_tie():
    """E2 and E3: every local score is a multiple of maxabs, so two that differ are at least 2^20 apart.  E1: every local score is
    the length of a run of exact matches, far below 2^24.  (The reads are random; the arithmetic holds for every read.)"""
    graph = G.tie_graph()
    m = G.maxabs(graph, ["A" * G.TIE_BASES])
    rng = np.random.default_rng(32)
    reads = [rand_bases(rng, G.TIE_BASES) for _ in range(20)]
    for name in ("E1", "E2", "E3"):
        scores, o, e = G.edge_scoring(name, graph, reads)
        got = [G.rule_score(graph, rd, 12, G.table_of(scores), o, e) or 0 for rd in reads]
        assert all(v % m == 0 for v in got) if name != "E1" else all(0 < v <= G.TIE_BASES for v in got), (name, got)


# ---- both strands at ordinary scorings: the conditions of the device batches, from the rule ----

def test_the_conditions_of_the_ordinary_scorings_hold():
    graph = haplotype(300, 3)
    for mode in (26, 27, 32):
        reads = G.strand_reads(mode)
        for name in G.ORDINARY:
            scores, o, e = G.ordinary(name)
            exp = expect_strands(graph, reads, mode, scores=scores, o=o, e=e)
            G.assert_conditions(mode, name, [(x[0], x[2], x[3]) for x in exp])
