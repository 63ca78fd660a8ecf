"""The rule of the both-strands affine-gap pathwise modes for reads of up to 131071 bases (-m 76 / -m 77 / -m 82;
RG_MODE_PATHWISE_GAP_XSTRANDS in include/recgraph_hip.h) stated in Python: a COMPOSITION of rules that exist, nothing new.

  a PICK on a strand      the score (and path, end row, walk) of tests/pathwise_gap_rule.py (R.align) for modes 76 / 77 and of
                          tests/pathwise_gap_local_rule.py (L.align_local) for mode 82, on the read or on its reverse complement
  which strands are       the exact rule, the vote rule (tests/strand_vote_rule.py: rc, first_reverse, minus) and, for mode 82,
  picked, which one wins  "every read without a bad base" — decided on the picked SCORES (`decide`)
  the report              the line of the winning strand's sequence in mode m + 50 (R.line / L.line_local), strand column '-' for a
                          reverse winner; both counters: every picked strand's score cells, the traced strand's traceback cells

`decide` takes the pick as a function score_of(sequence) -> integer (None: a local pick that is unaligned, which scores 0), so the
composition itself can be checked on hand cases without a graph (tests/test_pathwise_gap_xstrands_cpu.py).  Nothing here asks the
product anything."""
import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
import strand_vote_rule as V

XSTRANDS = {76: 6, 77: 7, 82: 12}
READ_BAD_BASE, READ_UNALIGNED = 8, 16
STRIPE = 2048


def canonical(read):
    return read.upper().replace("-", "N")


def decide(mode, s, score_of, kmers=None):
    """(winning strand, strands picked in order, the winner's score or None) for the canonical read text `s` ('+' the read as given,
    '-' its reverse complement).  `kmers` (strand_vote_rule.kmer_set of the path sequences): the vote rule, modes 76 and 77 only;
    None: the exact rule."""
    assert mode in XSTRANDS and not (kmers is not None and mode == 82)
    first = "-" if kmers is not None and V.first_reverse(kmers, s) else "+"
    other = "+" if first == "-" else "-"
    seq = {"+": s, "-": V.rc(s)}
    got = {first: score_of(seq[first])}
    picked = [first]
    # the second pick: mode 82 always; modes 76 / 77 iff the first score is < 0
    if mode == 82 or got[first] < 0:
        got[other] = score_of(seq[other])
        picked.append(other)
    val = lambda strand: 0 if got[strand] is None else got[strand]          # an unaligned local pick scores 0
    if len(picked) == 1:
        win = first
    else:
        win = "-" if val("-") > val("+") else "+"                            # reverse only when STRICTLY greater, whichever went first
    return win, picked, got[win]


def trace_cells(mode, rows, n, pick, striped):
    """The traceback cells mode m + 50 performs for one read of n bases whose pick is `pick` = (path, end row, end column, ops).
    Not striped (the batch's longest read has at most 2047 bases): the direction pass, rows of the picked path (modes 77 / 82: up to
    the end row) x n.  Striped: the checkpoint pass, the same rows x n, and per stripe the walk looks at — every (i, j) with i > 0 and
    j > 0 on it, the last one included — the largest such i x the stripe's columns that belong to the read."""
    k, end_row, j, ops = pick
    i = rows[k].index(end_row) + 1
    cells = (len(rows[k]) if mode == 76 else i) * n
    if not striped:
        return cells
    top = {}
    for op in [None] + list(ops):
        if op is not None:
            i, j = i - (op in "DU"), j - (op in "DL")
        if i > 0 and j > 0:
            top[j // STRIPE] = max(top.get(j // STRIPE, 0), i)
    for st, r in top.items():
        cells += r * (min(n, st * STRIPE + STRIPE - 1) - max(1, st * STRIPE) + 1)
    return cells


def expected(mode, read, lnz, rows, node_ids, name, kmers=None, table=None, o=-4, e=-2, striped=False):
    """One read as a dict: text, status, score, strand ('+', '-', or ' ' for a read without a record), picked (the strands in
    order), cells (rg_batch_cell_updates) and performed (rg_batch_cell_updates_performed).  `striped`: the longest read of the
    read's batch has more than 2047 bases (the traceback of the whole batch then runs the checkpointed kernels)."""
    s = canonical(read)
    if not set(s) <= set("ACGTN"):
        return dict(text="", status=READ_BAD_BASE, score=0, strand=" ", picked=[], cells=0, performed=0)
    n = len(s)
    found = {}

    def score_of(seq):
        if mode == 82:
            res = L.align_local(lnz, rows, seq, table, o, e)
            if res is None or res[0] == 0:
                found[seq] = None
                return None
            found[seq] = (res[1], res[2], res[3], res[5])
            return res[0]
        res = R.align(lnz, rows, seq, table, o, e, mode == 77)
        found[seq] = (res[1], res[2], n, res[3])
        return res[0]

    win, picked, score = decide(mode, s, score_of, kmers)
    cells = len(picked) * sum(len(r) for r in rows) * n
    if score is None:
        # mode 82, the winner is unaligned: then both strands are (an aligned strand scores above 0 and would have won)
        return dict(text="", status=READ_UNALIGNED, score=0, strand=" ", picked=picked, cells=cells, performed=cells)
    seq = s if win == "+" else V.rc(s)
    if mode == 82:
        text = L.line_local(lnz, rows, node_ids, name, seq, table, o, e)
    else:
        text = R.line(lnz, rows, node_ids, name, seq, table, o, e, mode == 77)
    if win == "-":
        text = V.minus(text)
    return dict(text=text, status=0, score=score, strand=win, picked=picked, cells=cells,
                performed=cells + trace_cells(mode, rows, n, found[seq], striped))
