"""Scorings at the edge of the admitted score range of the affine-gap pathwise families, the shapes that are run there, and the seeded
searches for strand scores that differ by less than an f32 ulp: what tests/test_pathwise_gap_scores_cpu.py (the preconditions, from the
rules alone) and tests/test_gpu_pathwise_gap_scores.py (the device) share.  A plain module beside the rules; nothing here asks the
product anything.

The plan admits a batch when (R + n) * max(|sc|, |o + e|) < 2^28, R the rows of the longest path and n the longest read, so
maxabs = (2^28 - 1) // (R + n) is the largest admitted magnitude of a shape and maxabs + 1 the first refused one.  The edge scorings:

    E1 "deep gaps"    match 1        mismatch -maxabs   o 0         e -maxabs
    E2 "open-heavy"   match +maxabs  mismatch -maxabs   o -maxabs   e 0
    E3 "tall"         match +maxabs  mismatch -maxabs   o 0         e -maxabs
    E4 "near ties"    match +maxabs  mismatch -1        o 0         e -1

E4 exists for one purpose: two LOCAL scores beyond 2^24 that differ by less than an f32 ulp.  Under E2 and E3 every score is a multiple
of maxabs, under E1 a local alignment is a run of exact matches of at most n points, so none of E1 .. E3 can give mode 32 such a pair
(test_pathwise_gap_scores_cpu.py asserts both facts); under E4 a score is matches * maxabs minus a few units."""
import functools
import os

import numpy as np

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
import strand_vote_rule as V
from pathwise_support import ROOT, TWO_BUBBLES, graph_tuple, haplotype, mixed_reads, noisy, rand_bases

LIMIT = 1 << 28
EDGES = {"E1": lambda m: (1, -m, 0, -m), "E2": lambda m: (m, -m, -m, 0), "E3": lambda m: (m, -m, 0, -m), "E4": lambda m: (m, -1, 0, -1)}
RULES = {6: 0, 7: 1, 12: 2}                   # the base mode of a rule: GAP_GLOBAL, GAP_SEMI, GAP_LOCAL


def longest_path(graph):
    return max(len(r) for r in graph[3])


def maxabs(graph, reads):
    """The largest magnitude the plan admits for this graph_tuple and these reads."""
    return (LIMIT - 1) // (longest_path(graph) + max(len(r) for r in reads))


def edge_values(name, graph, reads):
    """(match, mismatch, o, e) of the edge scoring `name` for this shape."""
    return EDGES[name](maxabs(graph, reads))


def edge_scoring(name, graph, reads):
    """(scores, o, e) of the edge scoring `name` for this shape; scores: the matrix of api.create_score_matrix_i32."""
    from recgraph_amd import api
    match, mismatch, o, e = edge_values(name, graph, reads)
    return api.create_score_matrix_i32(match, mismatch), o, e


def table_of(scores):
    from recgraph_amd import api
    return api._table_from_dict(scores)


def path_bases(graph, k):
    return "".join(graph[2][r] for r in graph[3][k])


# ---- the shapes of the i32 edge ----

BASE_LENGTHS = (255, 256, 512, 1024, 2047)        # C = 4, 8, 16, 32, 32 columns per lane in modes 6 / 7 / 12
LONG_LENGTHS = (2048, 4097)                       # two stripes (the second nearly all padding), three stripes
SQUARE_MAX = 2048


@functools.lru_cache(maxsize=None)
def square(n, seed=7):
    """graph_tuple of two paths of exactly n rows: a random sequence, and the same with six single bases replaced in bubbles."""
    rng = np.random.default_rng(seed + n)
    w = rand_bases(rng, n)
    step = max(3, n // 6)
    spots = [q for q in range(step // 2, n - 1, step) if q >= 1]
    segs, links, p0, p1, prev, nid = [], [], [], [], 0, 0
    tails = []                                    # the segment(s) the next one is linked from

    def seg(s):
        nonlocal nid
        nid += 1
        segs.append("S\t%d\t%s" % (nid, s))
        return nid

    for q in spots + [n]:
        chunk = seg(w[prev:q])
        links.extend((t, chunk) for t in tails)
        p0.append(chunk)
        p1.append(chunk)
        tails = [chunk]
        if q < n:
            a, b = seg(w[q]), seg("ACGT"[("ACGT".index(w[q]) + 2) % 4])
            links.extend([(chunk, a), (chunk, b)])
            p0.append(a)
            p1.append(b)
            tails = [a, b]
        prev = q + 1
    gfa = "\n".join(["H\tVN:Z:1.0"] + segs + ["L\t%d\t+\t%d\t+\t0M" % ab for ab in links] +
                    ["P\tp%d\t%s\t*" % (k, ",".join("%d+" % i for i in p)) for k, p in enumerate((p0, p1))]) + "\n"
    graph = graph_tuple(gfa)
    assert [len(r) for r in graph[3]] == [n, n] and path_bases(graph, 0) == w, [len(r) for r in graph[3]]
    return graph


@functools.lru_cache(maxsize=None)
def flat():
    """graph_tuple of the hand graph of two paths of five rows."""
    return graph_tuple(TWO_BUBBLES)


def _with_runs(rng, s):
    """`s` with a few runs deleted and as many random bases inserted elsewhere (the length is kept)."""
    n = len(s)
    cuts = [(n // 5, 3, 3 * n // 5)] + ([(2 * n // 5, 7, 4 * n // 5)] if n >= 64 else [])
    out, at = [], 0
    for where, run, _ in cuts:
        out.append(s[at:where])
        at = where + run
    out.append(s[at:])
    s = "".join(out)
    for _, run, where in cuts:
        s = s[:where] + rand_bases(rng, run) + s[where:]
    assert len(s) == n
    return s


@functools.lru_cache(maxsize=None)
def edge_shape(kind, n):
    """(graph_tuple, reads) of one class: every read has exactly n bases.  "flat": three random reads on paths of five rows.  "square":
    on paths of n rows, an exact copy of path 1, a copy of path 0 with substitutions, and a copy with a few inserted and deleted runs."""
    rng = np.random.default_rng(1000 * n + len(kind))
    if kind == "flat":
        return flat(), tuple(rand_bases(rng, n) for _ in range(3))
    assert kind == "square" and n <= SQUARE_MAX
    graph = square(n)
    w0, w1 = path_bases(graph, 0), path_bases(graph, 1)
    return graph, (w1, noisy(rng, w0, every=29), _with_runs(rng, noisy(rng, w1, every=53)))


def shapes(lengths):
    return [(kind, n) for n in lengths for kind in ("flat", "square") if kind == "flat" or n <= SQUARE_MAX]


def rule_score(graph, read, mode, table, o, e):
    """The score the rule of base mode 6 / 7 / 12 gives one read; None for a read the local rule leaves unaligned."""
    lnz, rows = graph[2:4]
    if RULES[mode] == 2:
        res = L.align_local(lnz, rows, read, table, o, e)
        return None if res is None or res[0] == 0 else res[0]
    return R.align(lnz, rows, read, table, o, e, RULES[mode] == 1)[0]


# ---- plain scalar Gotoh on Python integers, None for "no value": no sentinel, so nothing to overflow, win or wrap ----

def _max(*vals):
    vals = [v for v in vals if v is not None]
    return max(vals) if vals else None


def _plus(v, d):
    return None if v is None else v + d


def unbounded_score(graph, read, mode, table, o, e):
    """The score of base mode 6 / 7 / 12 by plain Gotoh over every path; None for a read without a local alignment."""
    sc = [[int(table[a * 6 + b]) for b in range(5)] for a in range(5)]
    rule = RULES[mode]
    rc = [R.ALPHA.index(c) for c in R.canonical(read)]
    n, best = len(rc), None
    for k in range(len(graph[3])):
        bases = [R.ALPHA.index(c) for c in path_bases(graph, k)]
        H = [0] + [o + e * j for j in range(1, n + 1)]
        Y = [None] * (n + 1)
        if rule == 2:
            H = [0] * (n + 1)
        for i, b in enumerate(bases, 1):
            Hn, Yn, X = [None] * (n + 1), [None] * (n + 1), None
            if rule == 0:
                Hn[0] = Yn[0] = o + e * i
            else:
                Hn[0] = 0
            for j in range(1, n + 1):
                Yn[j] = _max(_plus(H[j], o + e), _plus(Y[j], e))
                X = _max(_plus(Hn[j - 1], o + e), _plus(X, e))
                Hn[j] = _max(_plus(H[j - 1], sc[b][rc[j - 1]]), Yn[j], X, 0 if rule == 2 else None)
            H, Y = Hn, Yn
            if rule == 1:
                best = _max(best, H[n])
            elif rule == 2:
                best = _max(best, max(H[1:]))
        if rule == 0:
            best = _max(best, H[n])
    return None if rule == 2 and best == 0 else best


# ---- both strands at ordinary scorings ----

ORDINARY = {"extend-only": (2, -4, 0, -2), "open-only": (2, -4, -6, 0), "steep": (2, -4, -40, -1), "hoxd70": (None, None, -400, -30),
            "unit": (0, -1, 0, -1), "non-negative": (3, 0, 0, 0)}


def ordinary(name):
    """(scores, o, e) of an ordinary scoring; scores: the matrix of api.create_score_matrix_i32."""
    from recgraph_amd import api
    match, mismatch, o, e = ORDINARY[name]
    if match is None:
        return api.create_score_matrix_i32(matrix_file_path=os.path.join(ROOT, "tests", "golden", "HOXD70.mtx")), o, e
    return api.create_score_matrix_i32(match, mismatch), o, e


@functools.lru_cache(maxsize=None)
def strand_reads(mode):
    """mixed_reads of the mode's both-strands rule on haplotype(300, 3), then a whole path and the reverse complement of another (what
    scores exactly 0 at unit costs in the global rule too), an exact piece of a path and the reverse complement of one."""
    w = [haplotype(300, 3)[0].path_sequence(k) for k in range(3)]
    return mixed_reads(mode if mode < 50 else mode - 50) + (w[1], V.rc(w[2]), w[0][60:200], V.rc(w[1][50:180]))


def assert_conditions(mode, name, answers):
    """What the batch of strand_reads(mode) at the ordinary scoring `name` is there for, asserted on the rule's answers
    [(text, strand, strands aligned in order), ...]."""
    from pathwise_gap_strands_rule import score_of
    local = mode in (32, 82)
    single_plus = [score_of(t) for t, strand, passes in answers if strand == "+" and passes == ["+"]]
    minus = [score_of(t) for t, strand, passes in answers if strand == "-"]
    ctx = (mode, name, [(strand, passes) for _, strand, passes in answers])
    if local:
        # every read without a bad base is aligned twice; at unit costs a match scores 0 and nothing aligns
        assert all(passes in (["+", "-"], []) for _, _, passes in answers), ctx
        assert all(strand == " " for _, strand, _ in answers) if name == "unit" else {"+", "-"} <= {strand for _, strand, _ in answers}, ctx
    elif name == "unit":
        assert 0 in single_plus and 0 in minus, ctx
    elif name == "non-negative":
        assert all(passes in (["+"], []) for _, _, passes in answers) and single_plus and min(single_plus) >= 0, ctx
    elif name == "open-only" and mode in (27, 77):
        # e = 0: three matches in a row pay for a gap of any length, and every 3-mer occurs in 900 path bases, so no clean read of
        # three bases or more scores below 0 forward in the semiglobal rule.  The batch has no '-' here, and that is the rule's answer.
        assert single_plus and not minus, ctx
    else:
        assert single_plus and minus, ctx


# ---- strand scores an f32 cannot tell apart ----

TIE_ROWS, TIE_BASES = 100, 60
TIE_SCORING = {26: "E1", 27: "E1", 32: "E4"}


def tie_graph():
    return square(TIE_ROWS)


def tie_scoring(mode):
    """(scores, o, e) of the scoring of the mode's near-tie reads: the shape is TIE_ROWS rows by TIE_BASES bases, whatever the reads."""
    return edge_scoring(TIE_SCORING[mode], tie_graph(), ["A" * TIE_BASES])


def _strand_scores(mode, rd):
    scores, o, e = tie_scoring(mode)
    table = table_of(scores)
    return tuple(rule_score(tie_graph(), s, mode - 20, table, o, e) or 0 for s in (rd, V.rc(rd)))


def same_f32(a, b):
    return a != b and np.float32(a) == np.float32(b)


@functools.lru_cache(maxsize=None)
def near_tie_reads(mode, want=3, tries=400):
    """((read, forward score, reverse score), ...): the first `want` of `tries` seeded random reads whose reverse strand scores
    strictly higher than the forward one although both are the same f32; modes 26 / 27: the forward score is below 0, so the exact
    rule aligns the other strand.  The search must succeed."""
    rng = np.random.default_rng(2600 + mode)
    out = []
    for _ in range(tries):
        rd = rand_bases(rng, TIE_BASES)
        f, r = _strand_scores(mode, rd)
        if r > f and same_f32(f, r) and (mode == 32 or f < 0):
            out.append((rd, f, r))
            if len(out) == want:
                return tuple(out)
    raise AssertionError("mode %d: %d of %d reads have strand scores an f32 cannot tell apart: the precondition of the case does not hold"
                         % (mode, len(out), tries))


def tie_kmers():
    return V.kmer_set([path_bases(tie_graph(), k) for k in range(2)])


@functools.lru_cache(maxsize=None)
def near_tie_vote_reads(mode, want=2, tries=600):
    """((read, forward score, reverse score), ...) for the vote of modes 26 / 27: reads built to vote reverse first (the reverse
    complement of 20 bases of a path, then random bases) that score below 0 there, lower still on the forward strand, and the same as
    f32: the reverse-first record must stay.  The search must succeed."""
    rng = np.random.default_rng(2700 + mode)
    kmers = tie_kmers()
    out = []
    for _ in range(tries):
        w = path_bases(tie_graph(), int(rng.integers(0, 2)))
        q = int(rng.integers(0, TIE_ROWS - 20))
        rd = V.rc(w[q:q + 20]) + rand_bases(rng, TIE_BASES - 20)
        if not V.first_reverse(kmers, rd):
            continue
        f, r = _strand_scores(mode, rd)
        if f < r < 0 and same_f32(f, r):
            out.append((rd, f, r))
            if len(out) == want:
                return tuple(out)
    raise AssertionError("mode %d: %d of %d reverse-first reads have strand scores an f32 cannot tell apart: the precondition of the case "
                         "does not hold" % (mode, len(out), tries))
