"""The rule of the both-strands affine-gap pathwise modes (-m 26 / -m 27 / -m 32; RG_MODE_PATHWISE_GAP_STRANDS in
include/recgraph_hip.h) stated in Python: a COMPOSITION of rules that exist, nothing new.

  one pass of "pipeline m"   tests/pathwise_gap_rule.py (R.line) for modes 26 / 27, tests/pathwise_gap_local_rule.py (L.line_local)
                             for mode 32, on the read or on its reverse complement
  which passes run, and      RG_AMB_BOTH_STRANDS (the exact rule), RG_AMB_STRAND_VOTE (tests/strand_vote_rule.py: rc, votes, minus),
  which record is kept       and for mode 32 "every read that has a record"

`expected` takes the pass as a function line_fn(read text) -> line ("" for a read the local rule leaves unaligned), so the
composition itself can be checked on hand cases without a graph (tests/test_pathwise_gap_strands_cpu.py).  Nothing here asks the
product anything."""
import re

import strand_vote_rule as V

STRANDS = {26: 6, 27: 7, 32: 12}
READ_BAD_BASE, READ_UNALIGNED = 8, 16


def canonical(read):
    return read.upper().replace("-", "N")


def score_of(line):
    """The integer a record prints; an unaligned local read has no line and score 0."""
    return int(re.search(r"score: (-?\d+)", line).group(1)) if line else 0


def line_fn(mode, lnz, rows, node_ids, name, table=None, o=-4, e=-2):
    """One pass of pipeline `mode - 10` as a function of the read text."""
    import pathwise_gap_local_rule as L
    import pathwise_gap_rule as R
    if mode == 32:
        return lambda rd: L.line_local(lnz, rows, node_ids, name, rd, table, o, e)
    return lambda rd: R.line(lnz, rows, node_ids, name, rd, table, o, e, mode == 27)


def expected(mode, read, line_of, kmers=None):
    """(text, status, strand, passes) of one read.  `kmers` (strand_vote_rule.kmer_set of the path sequences): the vote rule, modes
    26 and 27 only; None: the exact rule.  strand is '+' or '-', or ' ' for a read without a record; passes lists the strands that
    were aligned, in order ('+' the read as given, '-' its reverse complement)."""
    assert mode in STRANDS and not (kmers is not None and mode == 32)
    s = canonical(read)
    if not set(s) <= set("ACGTN"):
        return "", READ_BAD_BASE, " ", []
    if kmers is not None and V.first_reverse(kmers, s):
        # the vote's pass A is the reverse strand; the forward strand is looked at only when that scored below 0
        rev = line_of(V.rc(s))
        passes = ["-"]
        fwd = None
        if score_of(rev) < 0:
            fwd = line_of(s)
            passes.append("+")
    else:
        fwd = line_of(s)
        passes = ["+"]
        rev = None
        if mode == 32 or score_of(fwd) < 0:
            rev = line_of(V.rc(s))
            passes.append("-")
    # one strand aligned: that record; both: the reverse one only when STRICTLY greater, whichever went first
    take_rev = fwd is None or (rev is not None and score_of(rev) > score_of(fwd))
    if take_rev:
        return V.minus(rev), 0, "-", passes             # (a chosen reverse record has a line: its score is above the forward one's >= 0, or it is the vote's only pass)
    if not fwd:
        return "", READ_UNALIGNED, " ", passes          # (mode 32, neither strand aligns: strand '+', no line and so no record to ask)
    return fwd, 0, "+", passes
