"""What the tests of the pathwise mode families share: GFA constants, read and graph builders, the batch runners, the per-read checker
of the affine-gap rules and the register bar of their kernels.  A plain module beside the rule modules (tests/pathwise_gap_rule.py and
its kin), imported the same way; every name without a leading underscore is the interface, and no test module imports another.

Plain modules do not get pytest's assertion rewriting, so every assert here carries its own message.

check_reads is the one per-read checker of modes 6 / 7 / 12 and of every family built on them (16 .. 22, 26 .. 32, 44 / 45, 56 .. 62,
76 .. 82), keyed by the rule (GAP_GLOBAL / GAP_SEMI / GAP_LOCAL of recgraph_amd/_lib.py): (a) the whole line equals the line built
from the rule's record, and is empty for a read the local rule leaves unaligned; (b) the printed CIGAR, re-scored against the printed
path bases and the read (local: its slice [query start, query end]) with o, e and the matrix, gives exactly the printed score; (c) the
status is 0, or READ_UNALIGNED where the local rule finds nothing.  It launches nothing.  The rule's four int64 matrices are kept
under rows * (n + 1) <= 1.2e7 per read: a condition on the caller's shapes, asserted here."""
import ctypes as C
import functools
import importlib
import os
import re
import sys
from collections import namedtuple

import numpy as np

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
import pathwise_gap_strands_rule as S
import pathwise_gap_xstrands_rule as X
import strand_vote_rule as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- GFA constants ----

DIAMOND = ("H\tVN:Z:1.0\nS\t1\tA\nS\t2\tT\nS\t3\tC\nS\t4\tG\nL\t1\t+\t2\t+\t0M\nL\t1\t+\t3\t+\t0M\nL\t2\t+\t4\t+\t0M\n"
           "L\t3\t+\t4\t+\t0M\nP\tp0\t1+,2+,4+\t*\nP\tp1\t1+,3+,4+\t*\n")
TWO_BUBBLES = ("S\t1\tA\nS\t2\tT\nS\t3\tC\nS\t4\tG\nS\t5\tA\nS\t6\tC\nS\t7\tT\n" +
               "".join(f"L\t{a}\t+\t{b}\t+\t0M\n" for a, b in [(1, 2), (1, 3), (2, 4), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)]) +
               "P\tp0\t1+,2+,4+,5+,7+\t*\nP\tp1\t1+,3+,4+,6+,7+\t*\n")
NO_G = "S\t1\tA\nS\t2\tC\nS\t3\tT\nS\t4\tA\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t3\t+\t4\t+\t0M\nP\tp0\t1+,2+,3+,4+\t*\n"
# no segment holds an A: AAAAAA finds nothing forward, its reverse complement TTTTTT does
NO_A = ("S\t1\tGCTTTTTTCG\nS\t2\tC\nS\t3\tG\nS\t4\tTTCC\n" + "".join("L\t%d\t+\t%d\t+\t0M\n" % ab for ab in [(1, 2), (1, 3), (2, 4), (3, 4)]) +
        "P\tp0\t1+,2+,4+\t*\nP\tp1\t1+,3+,4+\t*\n")
PALINDROME = "ACGTACGT" * 4

# a GFA the reference accepts beyond the tidy synthetic graphs: several sinks, ids neither contiguous nor in order (the ingestion tests)
ODD_SEGMENTS = {10: "AC", 3: "G", 7: "T", 20: "CA", 15: "TT"}
ODD_LINKS = [(7, 20), (7, 15), (3, 10), (10, 15), (3, 7)]
ODD_PATHS = [("p0", [3, 10, 15]), ("p1", [3, 7, 20]), ("p2", [3, 7, 15])]


def odd_gfa(links=ODD_LINKS, seg_order=(10, 3, 7, 20, 15)):
    out = ["H\tVN:Z:1.0"]
    out += ["S\t%d\t%s" % (i, ODD_SEGMENTS[i]) for i in seg_order]
    out += ["L\t%d\t+\t%d\t+\t0M" % l for l in links]
    out += ["P\t%s\t%s\t*" % (n, ",".join("%d+" % i for i in st)) for n, st in ODD_PATHS]
    return "\n".join(out) + "\n"


def renumbered(sg, rnd):
    """A synthetic graph with ids mapped to a random increasing sequence (gaps, still topological) and shuffled lines."""
    ids = sorted(rnd.sample(range(1, 5 * len(sg.segments)), len(sg.segments)))
    mp = {i: ids[k] for k, (i, _) in enumerate(sg.segments)}
    segs = ["S\t%d\t%s" % (mp[i], s) for i, s in sg.segments]
    links = ["L\t%d\t+\t%d\t+\t0M" % (mp[a], mp[b]) for a, b in sorted(set(sg.links))]
    rnd.shuffle(segs)
    rnd.shuffle(links)
    paths = ["P\tp%d\t%s\t*" % (k, ",".join("%d+" % mp[i] for i in p)) for k, p in enumerate(sg.paths)]
    lines = segs + links
    rnd.shuffle(lines)                     # S and L lines interleaved
    return "\n".join(["H\tVN:Z:1.0"] + lines + paths) + "\n"


# ---- reads and graphs ----

def rand_bases(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n))


def noisy(rng, s, every=97):
    """`s` with a substitution every `every` bases (the length is kept)."""
    s = list(s)
    for k in range(every // 2, len(s), every):
        s[k] = "ACGT"[("ACGT".index(s[k]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def of_length(rng, w, n):
    """A read of exactly n bases from the path bases w: a noisy prefix, or the whole path with random bases inserted in its middle."""
    if n <= len(w):
        return noisy(rng, w[:n])
    return noisy(rng, w[:len(w) // 2]) + rand_bases(rng, n - len(w)) + noisy(rng, w[len(w) // 2:])


def graph_tuple(g):
    """(g, api.Graph, lnz, rows, node ids) of a SynthGraph or of a GFA text: what the checkers take as `graph`."""
    from recgraph_amd import api
    gg = api.Graph.from_gfa_text(g if isinstance(g, str) else g.gfa())
    lnz, rows = R.graph_paths(gg)
    return g, gg, lnz, rows, R.graph_node_ids(gg)


@functools.lru_cache(maxsize=None)
def haplotype(path_len, n_paths=2, seed=71):
    """graph_tuple of a haplotype graph whose paths have about `path_len` rows, built once per process."""
    from recgraph_amd import synth
    return graph_tuple(synth.haplotype_graph(path_len * 13 // 10, n_paths, path_len=path_len, seed=seed))


# ---- batches ----

class Run(namedtuple("Run", "texts status scores counted performed stats")):
    """One batch: the lines, statuses and scores per read, cell_updates, cell_updates_performed and kernel_stats()."""

    @property
    def kernels(self):
        """The coarse kernel names ("inst:" and "mem:" entries left out)."""
        return {k for k in self.stats if k.startswith("k_")}

    @property
    def instantiations(self):
        """Launches per instantiation, from the launch log."""
        return {k[5:]: v[1] for k, v in self.stats.items() if k.startswith("inst:")}


def run_batch(gg, reads, mode, **params):
    from recgraph_amd import api
    b = api.Batch(gg, reads, api.make_params(mode, **params))
    b.run()
    b.fetch()
    n = len(reads)
    return Run([b.gaf_text(i, "r%d" % i, i + 1) for i in range(n)], [b.status(i) for i in range(n)], [b.score(i) for i in range(n)],
               b.cell_updates, b.cell_updates_performed, b.kernel_stats())


def align(gg, reads, mode, scores=None, o=-4, e=-2):
    from recgraph_amd import api
    return api.align_batch(gg, reads, ["r%d" % i for i in range(len(reads))], mode=mode, score_matrix=scores, o=o, e=e)


def create_rc(gfa, reads, mode, o=-4, e=-2, amb=0, match=2, mismatch=None, entries=()):
    """(return code, message) of rg_batch_create, which answers its refusals before a device is needed.  The scores: the default matrix
    with its A / A entry set to `match`, or, given `mismatch`, the match / mismatch matrix; entries ((a, b, value), ...) are written over it."""
    from recgraph_amd import api
    lib = api._lib.load()
    g = api.Graph.from_gfa_text(gfa)
    p = api.make_params(mode, score_matrix=None if mismatch is None else api.create_score_matrix_i32(match, mismatch), o=o, e=e, amb=amb)
    if mismatch is None:
        p.scores[0] = match
    for a, b, v in entries:
        p.scores[a * 6 + b] = v
    blob = "".join(reads).encode()
    off = (C.c_int64 * (len(reads) + 1))(*np.concatenate([[0], np.cumsum([len(r) for r in reads])]).tolist())
    out = C.c_void_p()
    rc = lib.rg_batch_create(g._h, C.byref(p), blob, off, len(reads), C.byref(out))
    if rc == 0:
        lib.rg_batch_destroy(out)
    return rc, lib.rg_last_error().decode()


def no_device():
    from recgraph_amd import api
    return api._lib.load().rg_device_count() == 0


# ---- the per-read checker ----

def _check_record(f, rd, rule, table, o, e, lnz, rows, ctx):
    """(b) for the fields `f` of one record against `rd`, the read on the strand that was aligned."""
    from recgraph_amd import api
    n = len(rd)
    mm = re.fullmatch(r"([0-9MXID]+), best path: (\d+), score: (-?\d+)", f[12])
    assert mm, (ctx, f[12][-80:])
    cigar, k, score, pseq = mm.group(1), int(mm.group(2)), int(mm.group(3)), f[13]
    if rule == api._lib.GAP_LOCAL:
        qs, qe = int(f[2]), int(f[3])
        assert 0 <= qs <= qe <= n - 1 and score > 0, (ctx, qs, qe, n, score)
        got = L.rescore(cigar, pseq, rd, qs, qe, table, o, e)
        assert got == (score, qe - qs + 1, len(pseq)), (ctx, got, score, qs, qe, len(pseq))
    else:
        assert f[2:4] == ["0", str(n - 1)], (ctx, f[:4])
        got = R.rescore(cigar, pseq, rd, table, o, e)
        assert got == (score, n, len(pseq)), (ctx, got, score, n, len(pseq))
    path = "".join(lnz[r] for r in rows[k])
    assert (pseq == path) if rule == api._lib.GAP_GLOBAL else (pseq in path), (ctx, k, len(pseq), len(path))


def check_reads(graph, reads, rule, scores=None, o=-4, e=-2, *, texts, status):
    """Every read of a batch (its lines `texts`, named r0, r1, ..., and its `status`) against the rule; `graph` is a graph_tuple."""
    from recgraph_amd import api
    lnz, rows, node_ids = graph[2:]
    table = None if scores is None else api._table_from_dict(scores)
    for i, rd in enumerate(reads):
        n = len(rd)
        assert rows and max(len(r) for r in rows) * (n + 1) <= 12_000_000, "the rule would need more than ~400 MB"
        if rule == api._lib.GAP_LOCAL:
            exp = L.line_local(lnz, rows, node_ids, "r%d" % i, rd, table, o, e)
        else:
            exp = R.line(lnz, rows, node_ids, "r%d" % i, rd, table, o, e, rule == api._lib.GAP_SEMI)
        assert texts[i] == exp, (rule, i, n, rd[:60], texts[i].split("\t")[:12], exp.split("\t")[:12], texts[i][-200:], exp[-200:])     # (a)
        assert status[i] == (0 if exp else api.READ_UNALIGNED), (rule, i, status[i])                                                 # (c)
        if not exp:
            continue
        assert texts[i].endswith("\n"), (rule, i, texts[i][-100:])
        f = texts[i][:-1].split("\t")
        assert f[:2] == ["r%d" % i, str(n)] and f[4] == "+" and f[9:12] == ["0", "*", "*"], (rule, i, f[:12])
        _check_record(f, rd, rule, table, o, e, lnz, rows, (rule, i))                                                                # (b)


def check_mode(graph, reads, mode, scores=None, o=-4, e=-2, texts=None, status=None):
    """Aligns `reads` in an affine-gap mode (or takes `texts` and `status`) and checks every read against the mode's rule; returns
    (texts, status)."""
    from recgraph_amd import api
    if texts is None:
        texts, status = align(graph[1], reads, mode, scores, o, e)
    check_reads(graph, reads, api._lib.gap_mode(mode).rule, scores, o, e, texts=texts, status=status)
    return texts, status


def check_base(graph, reads, semi, scores=None, o=-4, e=-2, texts=None, status=None):
    """check_mode for -m 6 / -m 7 on a graph_tuple or a GFA text, and beside it: the comments column against the rule's, and, where
    -m 4 / -m 5 walks the same rows (same CIGAR, path and bases), that mode's line with the comments column replaced; returns (texts,
    the number of such reads)."""
    from recgraph_amd import api
    graph = graph if isinstance(graph, tuple) else graph_tuple(graph)
    gg, lnz, rows = graph[1:4]
    texts, status = check_mode(graph, reads, api.MODE_PATHWISE_GAP_SEMI if semi else api.MODE_PATHWISE_GAP, scores, o, e, texts,
                               [0] * len(reads) if texts is not None and status is None else status)
    table = None if scores is None else api._table_from_dict(scores)
    m4, _ = api.align_batch(gg, reads, ["r%d" % i for i in range(len(reads))], mode=api.MODE_PATHWISE_SEMI if semi else api.MODE_PATHWISE, score_matrix=scores)
    whole = 0
    for i, rd in enumerate(reads):
        f = texts[i][:-1].split("\t")
        exp = R.comments(lnz, rows, rd, table, o, e, semi)
        assert "\t".join(f[12:]) == exp, (i, rd[:60], "\t".join(f[12:])[-300:], exp[-300:])
        f4 = m4[i][:-1].split("\t")
        if f4[12].split(", score")[0] == f[12].split(", score")[0] and f4[13] == f[13]:
            assert f[:12] == f4[:12], (i, f[:12], f4[:12])
            whole += 1
    return texts, whole


def check_local(graph, reads, scores=None, o=-4, e=-2, texts=None, status=None):
    """check_mode for -m 12 on a graph_tuple or a GFA text, and beside it: every aligned read scores > 0 and at least what -m 7 gives the
    same read; returns (texts, status)."""
    from recgraph_amd import api
    graph = graph if isinstance(graph, tuple) else graph_tuple(graph)
    texts, status = check_mode(graph, reads, api.MODE_PATHWISE_GAP_LOCAL, scores, o, e, texts, status)
    m7, st7 = align(graph[1], reads, api.MODE_PATHWISE_GAP_SEMI, scores, o, e)
    assert st7 == [0] * len(reads), st7
    for i, text in enumerate(texts):
        if text:
            score, score7 = (int(re.search(r"score: (-?\d+)", t).group(1)) for t in (text, m7[i]))
            assert score > 0 and score >= score7, (i, score, score7)
    return texts, status


# ---- unit costs: modes 44 / 45, which are modes 16 / 17 at match 0, mismatch -1, o = 0, e = -1 ----

EDIT_BASE = {44: 16, 45: 17}
EDIT_KERNELS = {"k_edit_score", "k_gap_pick", "k_edit_dirs", "k_edit_trace"}


def unit_costs():
    from recgraph_amd import api
    return api.create_score_matrix_i32(0, -1)


def run_batch_unit(gg, reads, mode, scores=None):
    """run_batch at unit costs, or with the table `scores` in their place."""
    return run_batch(gg, reads, mode, score_matrix=unit_costs() if scores is None else scores, o=0, e=-1)


def check_edit(graph, reads, mode, scores=None, out=None):
    """Every read of a batch of mode 44 / 45 (run here, or `out`) against the rule of mode 16 / 17 at unit costs; returns the batch."""
    from recgraph_amd import api
    if out is None:
        out = run_batch_unit(graph[1], reads, mode, scores)
    check_reads(graph, reads, api._lib.gap_mode(EDIT_BASE[mode]).rule, unit_costs() if scores is None else scores, 0, -1, texts=out[0], status=out[1])
    return out


# ---- both strands: modes 26 / 27 / 32 and 76 / 77 / 82 ----

def run_batch_strands(gg, reads, mode, amb=None, log=False, scores=None, o=-4, e=-2):
    """One batch through the C accessors: texts, status, scores, strands (None: no record), kernel statistics, cell counters.
    `scores` (a matrix of api.create_score_matrix_i32; None: the default one), `o` and `e` as in `align`."""
    from recgraph_amd import api
    n = len(reads)
    if log:
        api.set_option("launch_log", 1)
    try:
        b = api.Batch(gg, reads, api.make_params(mode, score_matrix=scores, o=o, e=e, amb=amb))
        b.run()
        b.fetch()
        stats = b.kernel_stats()
    finally:
        if log:
            api.set_option("launch_log", 0)
    fields = [b.fields(i) for i in range(n)]
    return dict(texts=[b.gaf_text(i, "r%d" % i, i + 1) for i in range(n)], status=[b.status(i) for i in range(n)],
                score=[b.score(i) for i in range(n)], strand=[f.strand if f else None for f in fields],
                query=[(f.query_start, f.query_end) if f else None for f in fields],
                stats={k: v[1] for k, v in stats.items() if not k.startswith("inst:") and not k.startswith("mem:")},
                inst={k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")}, cells=(b.cell_updates, b.cell_updates_performed))


def _table(scores):
    from recgraph_amd import api
    return None if scores is None else api._table_from_dict(scores)


def expect_strands(graph, reads, mode, kmers=None, scores=None, o=-4, e=-2):
    """The answers of the composed rule of tests/pathwise_gap_strands_rule.py, read by read."""
    g, gg, lnz, rows, node_ids = graph
    table = _table(scores)
    out = []
    for i, rd in enumerate(reads):
        assert max(len(r) for r in rows) * (len(rd) + 1) <= 12_000_000, "the rule would need more than ~400 MB"
        out.append(S.expected(mode, rd, S.line_fn(mode, lnz, rows, node_ids, "r%d" % i, table, o, e), kmers))
    return out


def check_strands(graph, reads, mode, res, kmers=None, exp=None, scores=None, o=-4, e=-2):
    """Checks every read of the batch result `res` (run_batch_strands) against the composed rule of mode 26 / 27 / 32: (a) the whole
    line, (b) the status, (c) the strand, score and query accessors, (d) the CIGAR re-scored on the strand that was chosen, with
    `scores`, `o` and `e` (the ones the batch ran with); returns the rule's answers."""
    from recgraph_amd import api
    g, gg, lnz, rows, node_ids = graph
    rule = api._lib.gap_mode(mode).rule
    exp = exp or expect_strands(graph, reads, mode, kmers, scores, o, e)
    table = _table(scores)
    for i, rd in enumerate(reads):
        text, status, strand, passes = exp[i]
        got = res["texts"][i]
        assert got == text, (mode, i, len(rd), got.split("\t")[:12], text.split("\t")[:12], got[-120:], text[-120:])        # (a)
        assert res["status"][i] == status, (mode, i, res["status"][i], status)                                               # (b)
        if not text:
            assert res["strand"][i] is None, (mode, i)
            if status == S.READ_UNALIGNED:
                assert res["score"][i] == 0, (mode, i, res["score"][i])
            continue
        f = got[:-1].split("\t")
        assert res["strand"][i] == strand == f[4] and res["score"][i] == S.score_of(text), (mode, i, res["strand"][i], strand, res["score"][i])     # (c)
        assert res["query"][i] == (int(f[2]), int(f[3])), (mode, i, res["query"][i], f[2:4])
        chosen = V.rc(S.canonical(rd)) if strand == "-" else S.canonical(rd)
        _check_record(f, chosen, rule, table, o, e, lnz, rows, (mode, i))                                                     # (d)
    return exp


def expect_xstrands(graph, reads, mode, kmers=None, scores=None, o=-4, e=-2):
    """The answers of the composed rule of tests/pathwise_gap_xstrands_rule.py, read by read."""
    g, gg, lnz, rows, node_ids = graph
    table = _table(scores)
    striped = max(len(r) for r in reads) > 2047
    out = []
    for i, rd in enumerate(reads):
        assert max(len(r) for r in rows) * (len(rd) + 1) <= 12_000_000, "the rule would need more than ~400 MB"
        out.append(X.expected(mode, rd, lnz, rows, node_ids, "r%d" % i, kmers, table, o, e, striped=striped))
    return out


def check_x(graph, reads, mode, res, kmers=None, exp=None, scores=None, o=-4, e=-2):
    """Every read of the batch result `res` (run_batch_strands) of mode 76 / 77 / 82 against the composed rule, by check_strands on the
    rule's answer, and the batch's scores and two cell counters against the rule's sums; returns the rule's answers."""
    exp = exp or expect_xstrands(graph, reads, mode, kmers, scores, o, e)
    check_strands(graph, reads, mode - 50, res, exp=[(x["text"], x["status"], x["strand"], x["picked"]) for x in exp], scores=scores, o=o, e=e)
    assert res["score"] == [x["score"] for x in exp], (mode, res["score"], [x["score"] for x in exp])
    want = (sum(x["cells"] for x in exp), sum(x["performed"] for x in exp))
    assert res["cells"] == want, (mode, res["cells"], want)
    return exp


def with_bad_base(rd):
    return rd[:len(rd) // 2] + "?" + rd[len(rd) // 2 + 1:]


@functools.lru_cache(maxsize=None)
def wrong_strand_read_that_scores_above_zero():
    """A 12- to 20-base piece of a path, given on the REVERSE strand, whose forward semiglobal score is >= 0 although its reverse
    complement scores higher: the exact rule never looks at the other strand.  Searched with a fixed seed; the search must succeed."""
    g, gg, lnz, rows, node_ids = haplotype(300, 3)
    rng = np.random.default_rng(2027)
    for _ in range(400):
        k, n = int(rng.integers(0, 3)), int(rng.integers(12, 21))
        w = g.path_sequence(k)
        q = int(rng.integers(0, len(w) - n))
        rd = V.rc(w[q:q + n])
        f, r = R.align(lnz, rows, rd, semi=True)[0], R.align(lnz, rows, V.rc(rd), semi=True)[0]
        if f >= 0 and r > f:
            return rd, f, r
    raise AssertionError("no 12- to 20-base reverse-strand read scores >= 0 forward on this graph: the precondition of the case does not hold")


@functools.lru_cache(maxsize=None)
def mixed_reads(mode):
    """Both strands, a 1-base read, N only, a bad base, a reverse palindrome; mode 27: the wrong-strand read that stays forward."""
    g = haplotype(300, 3)[0]
    rng = np.random.default_rng(260 + mode)
    w = [g.path_sequence(k) for k in range(3)]
    whole, piece = noisy(rng, w[0]), noisy(rng, w[1][40:190], every=41)
    reads = [whole, piece, V.rc(whole), V.rc(piece), "A", "N" * 30, with_bad_base(w[2][20:120]), PALINDROME, noisy(rng, V.rc(w[2])), w[2][100:250]]
    if mode == 27:
        reads.append(wrong_strand_read_that_scores_above_zero()[0])
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def long_read():
    """A noisy 2100-base prefix of a path of about 2200 rows: it scores above 0 in modes 26 and 27 on its own strand."""
    g = haplotype(2200)[0]
    rd = noisy(np.random.default_rng(3), g.path_sequence(1)[:2100], every=53)
    assert len(rd) == 2100, len(rd)
    return rd


# ---- what the compiler made of the kernels ----

def kernel_resources():
    """The module tools/kernel_resources.py (report(): the instantiations of a .hip cross-compiled for gfx950, no GPU)."""
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    return importlib.import_module("kernel_resources")


def assert_rows_in_registers(src, count, vgprs, lds=None):
    """The families' bar for the `count` instantiations of csrc/`src`: no scratch, no spilled VGPR, no AGPR (a kernel without MFMA that
    holds AGPRs has had VGPRs moved there: a spill in all but name), at most `vgprs` VGPRs (a number, or a function of the kernel's
    name) and at most `lds` bytes of LDS (None: not asked).  Returns the report."""
    ks = kernel_resources().report(src)
    assert len(ks) == count, (src, len(ks), count, sorted(k["name"] for k in ks))
    for k in ks:
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0 and k["AGPRs"] == 0, (k["name"], k)
        assert k["VGPRs"] <= (vgprs(k["name"]) if callable(vgprs) else vgprs), (k["name"], k)
        assert lds is None or k["LDS Size [bytes/block]"] <= lds, (k["name"], k)
    return ks
