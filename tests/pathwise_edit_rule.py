"""The bit-vector form of the rule of modes 16 / 17 at unit costs (RG_MODE_PATHWISE_EDIT / RG_MODE_PATHWISE_EDIT_SEMI, -m 44 / -m 45;
include/recgraph_hip.h), restated on Python's big integers: the row step of recgraph_amd/csrc/edit/rg_edit_bits.hpp on ONE integer of n
bits (bit t = read column t + 1), the score of the last column followed through its bit, and the walk over the two bits per cell the
direction pass keeps.  tests/test_pathwise_edit_cpu.py holds it equal to tests/pathwise_gap_rule.py at o = 0, e = -1: naive_scores for
the last column of every row, traceback for the ops, ties included.  Nothing here asks the device anything."""
import pathwise_gap_rule as R


def unit_table(scores):
    """scores[a * 6 + b] -> the 5 x 5 block as nested lists; every entry must be 0 or -1 (the modes' admission)."""
    t = [[int(scores[a * 6 + b]) for b in range(5)] for a in range(5)]
    assert all(v in (0, -1) for row in t for v in row)
    return t


def match_vectors(read, table):
    """Peq[b]: bit t is set iff the table scores path base b against read[t] with 0."""
    peq = [0] * 5
    for t, c in enumerate(read):
        for b in range(5):
            if table[b][R.ALPHA.index(c)] == 0:
                peq[b] |= 1 << t
    return peq


def row_step(eq, pv, mv, hin, n):
    """One path row: (Pv, Mv) of the row above -> (Pv, Mv, Ph, Mh, D0) of this one, Ph and Mh UNSHIFTED (bit t: column t + 1 is one
    more / one less than in the row above), D0 bit t: column t + 1 equals its diagonal.  hin: 1 in the global kind (column 0 is i)."""
    mask = (1 << n) - 1
    xv = eq | mv
    xh = ((((eq & pv) + pv) ^ pv) | eq) & mask
    ph = (mv | ~(xh | pv)) & mask
    mh = pv & xh
    d0 = xh | mv
    phs = ((ph << 1) | hin) & mask
    mhs = (mh << 1) & mask
    return (mhs | ~(xv | phs)) & mask, phs & xv, ph, mh, d0


def path_bits(bases, read, scores, semi):
    """(last, bits): last[i] = the score of (row i, column n) for i = 0 .. m, as pathwise_gap_rule.naive_scores returns it; bits[i] =
    (D0, Ph) of row i (bits[0] is None)."""
    read = R.canonical(read)
    n = len(read)
    peq = match_vectors(read, unit_table(scores))
    pv, mv = (1 << n) - 1, 0
    cur = n
    last, bits = [-cur], [None]
    top = 1 << (n - 1)
    for b in bases:
        pv, mv, ph, mh, d0 = row_step(peq[R.ALPHA.index(b)], pv, mv, 0 if semi else 1, n)
        cur += (1 if ph & top else 0) - (1 if mh & top else 0)
        last.append(-cur)
        bits.append((d0, ph))
    return last, bits


def walk(bits, bases, read, scores, m_end, semi):
    """Ops in walk order from (m_end, n), as pathwise_gap_rule.traceback returns them."""
    read = R.canonical(read)
    table = unit_table(scores)
    i, j, ops = m_end, len(read), []
    cap = m_end + len(read) + 2
    while (j > 0 if semi else (i > 0 or j > 0)):
        cap -= 1
        assert cap >= 0
        if i == 0:
            ops.append("L"); j -= 1
            continue
        if j == 0:
            ops.append("U"); i -= 1
            continue
        d0, ph = bits[i]
        match = table[R.ALPHA.index(bases[i - 1])][R.ALPHA.index(read[j - 1])] == 0
        if match or not (d0 >> (j - 1)) & 1:
            ops.append("D"); i -= 1; j -= 1
        elif (ph >> (j - 1)) & 1:
            ops.append("U"); i -= 1
        else:
            ops.append("L"); j -= 1
    return "".join(ops)
