"""CPU: check_reads of tests/pathwise_support.py, the per-read checker of every affine-gap family, can fail; so can the both-strands
checkers check_strands and check_x, at the default scores and at the scores, o and e they are given.

It has only ever been fed right lines.  Here it gets the rules' own lines for a few short reads on TWO_BUBBLES and NO_G (one of them a
read the local rule leaves unaligned), which it must accept, and then the same lines with one thing wrong at a time, each of which it
must reject.  A wrong line differs from the rule's, so check (a) alone rejects all of them; the last test hands check_reads the wrong
line AS the rule's, so that the re-scoring (b) and the field checks have to object on their own."""
import re

import pytest

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
import pathwise_gap_strands_rule as S
import strand_vote_rule as V
from pathwise_support import NO_G, TWO_BUBBLES, check_reads, check_strands, check_x, expect_strands, expect_xstrands, graph_tuple

GLOBAL, SEMI, LOCAL = 0, 1, 2
READ_UNALIGNED = 16
READS = {TWO_BUBBLES: ["ATGCT", "ATGGGAT", "TGA", "NNN"], NO_G: ["ACTA", "GGGG", "CTA", "ACGTA"]}


def _rule_lines(graph, reads, rule):
    lnz, rows, ids = graph[2:]
    if rule == LOCAL:
        texts = [L.line_local(lnz, rows, ids, "r%d" % i, rd) for i, rd in enumerate(reads)]
    else:
        texts = [R.line(lnz, rows, ids, "r%d" % i, rd, semi=rule == SEMI) for i, rd in enumerate(reads)]
    return texts, [0 if t else READ_UNALIGNED for t in texts]


def _with(line, col, fn):
    f = line[:-1].split("\t")
    f[col] = fn(f[col])
    return "\t".join(f) + "\n"


# one wrong thing in the line of read 0 of TWO_BUBBLES, ATGCT: 3M1X1M on ATGAT (global, semi), 3M on ATG (local), both on path 0
WRONG_LINES = {
    "score": lambda t: _with(t, 12, lambda c: re.sub(r"score: (-?\d+)", lambda m: "score: %d" % (int(m.group(1)) + 1), c)),
    "cigar": lambda t: _with(t, 12, lambda c: c.replace("M", "X", 1)),
    "best path": lambda t: _with(t, 12, lambda c: c.replace("best path: 0", "best path: 1")),
    "newline": lambda t: t[:-1],
    "path bases": lambda t: _with(t, 13, lambda p: p[:-1]),
    "query end": lambda t: _with(t, 3, lambda q: str(int(q) + 1)),
}


def test_the_rules_own_lines_are_accepted():
    from recgraph_amd import api
    assert (api._lib.GAP_GLOBAL, api._lib.GAP_SEMI, api._lib.GAP_LOCAL, api.READ_UNALIGNED) == (GLOBAL, SEMI, LOCAL, READ_UNALIGNED)
    for gfa, reads in READS.items():
        assert all(3 <= len(r) <= 7 for r in reads)
        graph = graph_tuple(gfa)
        for rule in (GLOBAL, SEMI, LOCAL):
            texts, status = _rule_lines(graph, reads, rule)
            assert (READ_UNALIGNED in status) == (rule == LOCAL), (rule, status)
            check_reads(graph, reads, rule, texts=texts, status=status)


def _cases(whats):
    """(rule, what) for every rule to which `what` applies: only the local rule has a query end of its own and an unaligned read."""
    return [(rule, w) for rule in (GLOBAL, SEMI, LOCAL) for w in whats if rule == LOCAL or w not in ("query end", "status 0 on the unaligned read")]


@pytest.mark.parametrize("rule,what", _cases(sorted(WRONG_LINES) + ["status 0 on the unaligned read", "unaligned status on an aligned read"]))
def test_one_wrong_thing_is_rejected(rule, what):
    reads = READS[TWO_BUBBLES]
    graph = graph_tuple(TWO_BUBBLES)
    texts, status = _rule_lines(graph, reads, rule)
    if what == "status 0 on the unaligned read":
        assert status[3] == READ_UNALIGNED
        status[3] = 0
    elif what == "unaligned status on an aligned read":
        status[0] = READ_UNALIGNED
    else:
        texts[0] = WRONG_LINES[what](texts[0])
        assert texts[0] != _rule_lines(graph, reads, rule)[0][0]
    with pytest.raises(AssertionError):
        check_reads(graph, reads, rule, texts=texts, status=status)


@pytest.mark.parametrize("rule,what", _cases(["score", "cigar", "best path", "newline", "query end"]))
def test_the_rescoring_objects_without_the_line_comparison(rule, what, monkeypatch):
    """The wrong line is what the rule itself is made to answer: (a) passes, and the newline, field and re-scoring checks reject it."""
    reads = READS[TWO_BUBBLES][:1]
    graph = graph_tuple(TWO_BUBBLES)
    texts, status = _rule_lines(graph, reads, rule)
    wrong = WRONG_LINES[what](texts[0])
    monkeypatch.setattr(R, "line", lambda *a, **kw: wrong)
    monkeypatch.setattr(L, "line_local", lambda *a, **kw: wrong)
    with pytest.raises(AssertionError):
        check_reads(graph, reads, rule, texts=[wrong], status=status)


# ---- the both-strands checkers off the default scores ----

STRAND_READS = ["ATGCT", "AGCAT", "ATCAT", "NNN", "AT?AT", "G"]       # (AGCAT is the reverse complement of ATGCT; ATCAT that of ATGAT, path 0)
OFF_DEFAULT = [((2, -1), 0, -2), ((3, -1), -1, -1), ((0, -1), 0, -1), ((5, -7), -9, 0)]


def _scores(mm):
    from recgraph_amd import api
    return None if mm is None else api.create_score_matrix_i32(*mm)


def _res_of(exp, cells=None):
    """What run_batch_strands would return for a device that answers as the rule does: exp is [(text, status, strand, passes), ...]."""
    texts = [x[0] for x in exp]
    f = [t[:-1].split("\t") if t else None for t in texts]
    return dict(texts=texts, status=[x[1] for x in exp], score=[S.score_of(t) for t in texts], strand=[x[2] if x[0] else None for x in exp],
                query=[(int(q[2]), int(q[3])) if q else None for q in f], cells=cells)


@pytest.mark.parametrize("mode", [26, 27, 32])
@pytest.mark.parametrize("mm,o,e", OFF_DEFAULT)
def test_the_strand_checkers_take_the_scoring(mode, mm, o, e):
    """expect_strands and check_strands with scores, o, e: the rule's own answers at that scoring are accepted, and they are the rules'
    lines at that scoring; the answers at the default scoring are rejected, by the line comparison and, where the rule is made to
    agree with them, by the re-scoring of the CIGAR with the scoring that was passed."""
    from recgraph_amd import api
    graph = graph_tuple(TWO_BUBBLES)
    lnz, rows, ids = graph[2:]
    scores = _scores(mm)
    table = None if scores is None else api._table_from_dict(scores)
    exp = expect_strands(graph, STRAND_READS, mode, scores=scores, o=o, e=e)
    for i, rd in enumerate(STRAND_READS[:4]):
        one = lambda s: (L.line_local(lnz, rows, ids, "r%d" % i, s, table, o, e) if mode == 32 else
                         R.line(lnz, rows, ids, "r%d" % i, s, table, o, e, mode == 27))
        assert exp[i][0] in ("", one(rd), V.minus(one(V.rc(rd))) if one(V.rc(rd)) else ""), (mode, i, exp[i])
    assert exp[4][1:] == (S.READ_BAD_BASE, " ", [])
    assert check_strands(graph, STRAND_READS, mode, _res_of(exp), scores=scores, o=o, e=e) == exp
    default = expect_strands(graph, STRAND_READS, mode)
    assert default != exp
    with pytest.raises(AssertionError):
        check_strands(graph, STRAND_READS, mode, _res_of(default), scores=scores, o=o, e=e)
    if mm[0] != 2:                  # (another match score: every record of the default scoring re-scores to another number)
        with pytest.raises(AssertionError):
            check_strands(graph, STRAND_READS, mode, _res_of(default), exp=default, scores=scores, o=o, e=e)


@pytest.mark.parametrize("mode", [76, 77, 82])
@pytest.mark.parametrize("mm,o,e", OFF_DEFAULT)
def test_the_xstrand_checkers_take_the_scoring(mode, mm, o, e):
    graph = graph_tuple(TWO_BUBBLES)
    scores = _scores(mm)
    exp = expect_xstrands(graph, STRAND_READS, mode, scores=scores, o=o, e=e)
    same = expect_strands(graph, STRAND_READS, mode - 50, scores=scores, o=o, e=e)
    assert [(x["text"], x["status"], x["strand"], x["picked"]) for x in exp] == same
    res = _res_of(same, cells=(sum(x["cells"] for x in exp), sum(x["performed"] for x in exp)))
    assert check_x(graph, STRAND_READS, mode, res, scores=scores, o=o, e=e) == exp
    default = expect_xstrands(graph, STRAND_READS, mode)
    assert [x["score"] for x in default] != [x["score"] for x in exp]
    with pytest.raises(AssertionError):
        check_x(graph, STRAND_READS, mode, res, scores=scores, o=o, e=e, exp=default)
    with pytest.raises(AssertionError):
        check_x(graph, STRAND_READS, mode, res)                     # (the default scoring: another rule answer)
    res["cells"] = (res["cells"][0], res["cells"][1] + 1)
    with pytest.raises(AssertionError):
        check_x(graph, STRAND_READS, mode, res, scores=scores, o=o, e=e)
