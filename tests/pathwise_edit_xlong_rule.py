"""The striped row step of modes 94 / 95 (RG_MODE_PATHWISE_EDIT_XLONG / RG_MODE_PATHWISE_EDIT_SEMI_XLONG; THE STRIPED ROW STEP in
recgraph_amd/csrc/edit/rg_edit_bits.hpp) restated on Python's integers with the stripe width as a parameter: a row of n bits is cut
into stripes of `width` bits, each a vector of its own, and stripe s > 0 takes hin in {-1, 0, +1} from the top bit of its left
neighbour's unshifted Ph / Mh.  tests/test_pathwise_edit_xlong_cpu.py holds every stripe's bits equal to those of
tests/pathwise_edit_rule.py on the whole vector.  Also the cells the one-stripe traceback rebuilds, from the rule's walk.  Nothing here
asks the device anything."""
import pathwise_edit_rule as E
import pathwise_gap_rule as R

STRIPE = 16384


def stripe_step(eq, pv, mv, hin, width):
    """One path row of one stripe: (Pv, Mv) of the row above -> (Pv, Mv, Ph, Mh, D0, hout); Ph and Mh unshifted, as E.row_step."""
    assert hin in (-1, 0, 1)
    mask = (1 << width) - 1
    xv = eq | mv
    eqh = eq | (1 if hin < 0 else 0)                 # for the Xh term only
    xh = ((((eqh & pv) + pv) ^ pv) | eqh) & mask     # the carry out of the stripe is dropped
    ph = (mv | ~(xh | pv)) & mask
    mh = pv & xh
    d0 = xh | mv
    phs = ((ph << 1) | (1 if hin > 0 else 0)) & mask
    mhs = ((mh << 1) | (1 if hin < 0 else 0)) & mask
    hout = ((ph >> (width - 1)) & 1) - ((mh >> (width - 1)) & 1)
    return (mhs | ~(xv | phs)) & mask, phs & xv, ph, mh, d0, hout


def striped_bits(bases, read, scores, semi, width, hins=None):
    """(last, bits) as E.path_bits returns them, computed stripe by stripe (stripes outermost, as the kernels run) and put together
    again; every hin that a stripe s > 0 took is added to the set `hins`."""
    read = R.canonical(read)
    n, m = len(read), len(bases)
    peq = E.match_vectors(read, E.unit_table(scores))
    S = (n + width - 1) // width
    mask = (1 << width) - 1
    d0s, phs, mhs = [0] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    bnd = [0 if semi else 1] * (m + 1)               # what the stripe takes, per row
    for s in range(S):
        pv, mv = mask, 0
        out = [0] * (m + 1)
        for i, b in enumerate(bases, 1):
            if s > 0 and hins is not None:
                hins.add(bnd[i])
            eq = (peq[R.ALPHA.index(b)] >> (s * width)) & mask
            pv, mv, ph, mh, d0, out[i] = stripe_step(eq, pv, mv, bnd[i], width)
            d0s[i] |= d0 << (s * width)
            phs[i] |= ph << (s * width)
            mhs[i] |= mh << (s * width)
        bnd = out
    top = 1 << (n - 1)
    full = (1 << n) - 1
    cur = n
    last, bits = [-cur], [None]
    for i in range(1, m + 1):
        cur += (1 if phs[i] & top else 0) - (1 if mhs[i] & top else 0)
        last.append(-cur)
        bits.append((d0s[i] & full, phs[i] & full))
    return last, bits


def rebuilt(ops, m_end, n, stripe=STRIPE):
    """(cells, stripes): what the traceback of a walk `ops` (walk order, from (m_end, n)) rebuilds: per stripe in which the walk looks
    at a cell of the matrix proper (i >= 1 and j >= 1; cell (i, j) is of stripe (j - 1) // stripe), rows 1 .. the row it enters with,
    times the stripe's columns that belong to the read."""
    i, j = m_end, n
    cells, seen = 0, []
    for op in ops + "$":
        if i >= 1 and j >= 1:
            s = (j - 1) // stripe
            if s not in seen:
                seen.append(s)
                cells += i * (min(n, (s + 1) * stripe) - s * stripe)
        if op == "D":
            i -= 1; j -= 1
        elif op == "U":
            i -= 1
        elif op == "L":
            j -= 1
    return cells, seen
