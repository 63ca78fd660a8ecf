"""The rule of the both-strands edit-distance pathwise modes (-m 64 / -m 65; RG_MODE_PATHWISE_EDIT_STRANDS in include/recgraph_hip.h)
stated in Python as the product computes it — "both strands of EVERY read, the reverse strand only when STRICTLY greater" — so that it
can be compared with the rule the header names, the exact rule of modes 26 / 27 (tests/pathwise_gap_strands_rule.py: a `< 0` gate in
front of the reverse strand).  The two agree wherever every score is <= 0, which unit costs guarantee; tests/test_pathwise_edit_strands_cpu.py
checks that on random graphs.  Also the two cell counters of a batch, from the rule's answers.  Nothing here asks the product anything."""
import pathwise_gap_rule as R
import pathwise_gap_strands_rule as S
import strand_vote_rule as V

EDIT_STRANDS = {64: 26, 65: 27}      # mode -> the both-strands affine-gap mode whose answers these are at unit costs
READ_BAD_BASE = S.READ_BAD_BASE


def expected(mode, read, line_of):
    """(text, status, strand, passes) of one read, in the shape of pathwise_gap_strands_rule.expected.  line_of(read text) -> the line
    of one strand in mode 16 / 17 at unit costs."""
    assert mode in EDIT_STRANDS
    s = S.canonical(read)
    if not set(s) <= set("ACGTN"):
        return "", READ_BAD_BASE, " ", []
    fwd, rev = line_of(s), line_of(V.rc(s))
    if S.score_of(rev) > S.score_of(fwd):
        return V.minus(rev), 0, "-", ["+", "-"]
    return fwd, 0, "+", ["+", "-"]


def counters(mode, reads, answers, lnz, rows, table):
    """(rg_batch_cell_updates, rg_batch_cell_updates_performed) of a batch whose reads have the rule's `answers` (text, status, strand,
    ...).  Counted: 2 n (rows summed over the paths) per read without a bad base — both strands are always scored.  Performed: that
    plus the direction pass of the traced strand: the rows of the picked path (mode 65: up to the end row) x n."""
    semi = mode == 65
    total = sum(len(r) for r in rows)
    counted = performed = 0
    for rd, ans in zip(reads, answers):
        if ans[1] == READ_BAD_BASE:
            continue
        s = S.canonical(rd)
        n = len(s)
        counted += 2 * n * total
        _, k, end_row, _, _ = R.align(lnz, rows, V.rc(s) if ans[2] == "-" else s, table, 0, -1, semi)
        performed += (rows[k].index(end_row) + 1 if semi else len(rows[k])) * n
    return counted, counted + performed
