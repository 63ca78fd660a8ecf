"""The rule of RG_MODE_PATHWISE_GAP_LOCAL (-m 12; include/recgraph_hip.h) stated in numpy, for tests/test_pathwise_gap_local_cpu.py,
the kernel matrix of the local gap kernels and the GPU tests: Smith-Waterman-Gotoh of the read against every path on its own, one row
at a time with X through np.maximum.accumulate, the choice among (path, row, column) and the tie-broken traceback that stops on the
first cell with H == 0.  Shares the helpers of tests/pathwise_gap_rule.py (-m 6 / -m 7); nothing here asks the device anything."""
import numpy as np

import pathwise_gap_rule as R
from pathwise_gap_rule import ALPHA, NEG, canonical, default_scores, graph_node_ids, graph_paths  # noqa: F401  (re-exported)


def _row(Hp, Yp, srow, o, e, ej):
    """Row i from row i - 1: (H, X, Y, D) along the last axis.  H' = max(0, D, Y) and column 0 is H = 0, X = Y = NEG; the scan
    over the clamped H' is exact because o <= 0."""
    Y = np.maximum(Hp + o + e, Yp + e)
    D = np.full_like(Hp, NEG)
    D[..., 1:] = Hp[..., :-1] + srow[..., 1:]
    Hq = np.maximum(np.maximum(D, Y), 0)
    Hq[..., 0] = 0
    Y[..., 0] = NEG
    z = Hq - ej
    run = np.empty_like(z)
    run[..., 0] = NEG
    run[..., 1:] = np.maximum.accumulate(z, axis=-1)[..., :-1]
    X = run + o + ej
    X[..., 0] = NEG
    return np.maximum(Hq, X), X, Y, D


def path_rows(bases, read, scores, o, e):
    """(H, X, Y, D) of every row 0 .. m for one path, each n + 1 wide."""
    sc = R._table(scores)
    rc = R._codes(read)
    n = len(read)
    ej = e * np.arange(n + 1, dtype=np.int64)
    H = np.zeros(n + 1, dtype=np.int64)
    Y = np.full(n + 1, NEG, dtype=np.int64)
    full = [(H, Y.copy(), Y.copy(), Y.copy())]
    srow = np.zeros(n + 1, dtype=np.int64)
    for b in bases:
        srow[1:] = sc[ALPHA.index(b)][rc]
        H, X, Y, D = _row(H, Y, srow, o, e, ej)
        full.append((H, X, Y, D))
    return full


def all_paths_best(lnz, rows, read, scores, o, e):
    """(best[k], first[k]): the largest H_k[i][j] over i >= 1, 1 <= j <= n and the first row index i (1-based) that attains it; every
    path advanced by the same row step at once."""
    sc = R._table(scores)
    rc = R._codes(read)
    n, P = len(read), len(rows)
    lens = np.array([len(r) for r in rows])
    M = int(lens.max())
    bc = np.full((P, M), 4, dtype=np.int64)
    for k, pr in enumerate(rows):
        bc[k, :len(pr)] = [ALPHA.index(lnz[r]) for r in pr]
    ej = e * np.arange(n + 1, dtype=np.int64)
    H = np.zeros((P, n + 1), dtype=np.int64)
    Y = np.full((P, n + 1), NEG, dtype=np.int64)
    best = np.zeros(P, dtype=np.int64)
    first = np.zeros(P, dtype=np.int64)
    srow = np.zeros((P, n + 1), dtype=np.int64)
    for t in range(M):
        act = lens > t
        srow[:, 1:] = sc[bc[:, t]][:, rc]
        Hn, _, Yn, _ = _row(H, Y, srow, o, e, ej)
        H = np.where(act[:, None], Hn, H)
        Y = np.where(act[:, None], Yn, Y)
        v = Hn[:, 1:].max(axis=1)
        up = act & (v > best)                       # strictly better: the first row that attains the maximum
        best[up] = v[up]
        first[up] = t + 1
    return best, first


def traceback(full, m_end, j_end, o, e):
    """(ops in walk order, stop row index, stop column) from state H at (m_end, j_end)."""
    H = [f[0] for f in full]
    X = [f[1] for f in full]
    Y = [f[2] for f in full]
    D = [f[3] for f in full]
    i, j, state, ops = m_end, j_end, "H", []
    while True:
        if state == "H":
            if H[i][j] == 0:                        # checked first; every border cell is one
                break
            if H[i][j] == D[i][j]:
                ops.append("D"); i -= 1; j -= 1
            elif H[i][j] == Y[i][j]:
                state = "Y"
            else:
                assert H[i][j] == X[i][j]
                state = "X"
        elif state == "Y":
            ops.append("U")
            state = "H" if H[i - 1][j] + o + e >= Y[i - 1][j] + e else "Y"
            i -= 1
        else:
            ops.append("L")
            state = "H" if H[i][j - 1] + o + e >= X[i][j - 1] + e else "X"
            j -= 1
    return "".join(ops), i, j


def align_local(lnz, rows, read, scores=None, o=-4, e=-2):
    """None when the read has no local alignment (best value 0); otherwise (score, path, end_row, end_col, stop_col, ops in walk
    order, path bases consumed in path order)."""
    read = canonical(read)
    assert set(read) <= set(ALPHA) and o <= 0 and e <= 0
    scores = default_scores() if scores is None else scores
    best, first = all_paths_best(lnz, rows, read, scores, o, e)
    pick = None                                     # (score, -row, -path) maximised
    for k, pr in enumerate(rows):
        if best[k] <= 0:
            continue
        cand = (int(best[k]), -pr[int(first[k]) - 1], -k, int(first[k]))
        if pick is None or cand[:3] > pick[:3]:
            pick = cand
    if pick is None:
        return None
    score, _, negk, m_end = pick
    k = -negk
    pr = rows[k]
    bases = [lnz[r] for r in pr[:m_end]]
    full = path_rows(bases, read, scores, o, e)
    hits = np.nonzero(full[m_end][0][1:] == score)[0]
    assert len(hits) >= 1
    end_col = int(hits[0]) + 1                      # the smallest column
    ops, i_stop, stop_col = traceback(full, m_end, end_col, o, e)
    used = sum(1 for c in ops if c in "DU")
    assert i_stop == m_end - used
    return score, k, pr[m_end - 1], end_col, stop_col, ops, "".join(bases[m_end - used:])


def line_local(lnz, rows, node_ids, name, read, scores=None, o=-4, e=-2):
    """The whole expected GAF line ("" for a read without a local alignment).  Query start is stop_col, query end is end_col - 1;
    path string and path coordinates as in pathwise_gap_rule.line for -m 7."""
    res = align_local(lnz, rows, read, scores, o, e)
    if res is None:
        return ""
    score, k, end_row, end_col, stop_col, ops, pseq = res
    pr, L = rows[k], len(lnz)
    m_end = pr.index(end_row) + 1
    used = len(pseq)
    ids = [node_ids[r] for r in pr[m_end - used:m_end]]
    ids = [x for q, x in enumerate(ids) if q == 0 or x != ids[q - 1]]
    stop = pr[m_end - used - 1] if m_end - used - 1 >= 0 else 0
    start = 0 if stop == 0 else stop + 1
    head = 0
    if start > 0:
        c = start - 1
        while c > 0 and node_ids[c] == node_ids[start]:
            c -= 1; head += 1
    tail, c = 0, end_row + 1
    while c < L - 1 and node_ids[c] == node_ids[end_row]:
        c += 1; tail += 1
    pend = head + used - 1 if used > 0 else 0
    cigar = R.cigar_of(ops, pseq, canonical(read)[stop_col:end_col])
    return "%s\t%d\t%d\t%d\t+\t>%s\t%d\t%d\t%d\t0\t*\t*\t%s, best path: %d, score: %d\t%s\n" % (
        name, len(read), stop_col, end_col - 1, ">".join(str(x) for x in ids), pend + tail + 1, head, pend, cigar, k, score, pseq)


def rescore(cigar, pseq, read, qstart, qend, scores=None, o=-4, e=-2):
    """Score of a printed CIGAR against the printed path bases and the read slice [qstart, qend] (inclusive), independently of any
    tie rule: (score, read bases consumed, path bases consumed)."""
    return R.rescore(cigar, pseq, canonical(read)[qstart:qend + 1], scores, o, e)


def naive_local(bases, read, scores, o, e):
    """Plain scalar Smith-Waterman-Gotoh (no scan, no numpy): H as (m + 1) lists of n + 1 values."""
    sc = R._table(scores)
    read = canonical(read)
    n, m = len(read), len(bases)
    H = [[0] * (n + 1) for _ in range(m + 1)]
    X = [[NEG] * (n + 1) for _ in range(m + 1)]
    Y = [[NEG] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            Y[i][j] = max(H[i - 1][j] + o + e, Y[i - 1][j] + e)
            X[i][j] = max(H[i][j - 1] + o + e, X[i][j - 1] + e)
            H[i][j] = max(0, H[i - 1][j - 1] + int(sc[ALPHA.index(bases[i - 1])][ALPHA.index(read[j - 1])]), Y[i][j], X[i][j])
    return H
