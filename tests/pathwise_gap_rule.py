"""The rule of RG_MODE_PATHWISE_GAP / RG_MODE_PATHWISE_GAP_SEMI (-m 6 / -m 7; include/recgraph_hip.h) stated in numpy, for
tests/test_pathwise_gap_cpu.py, the gap kernel matrix and the GPU tests: exact Gotoh of the read against every path on its own, one
row at a time with X through np.maximum.accumulate, the choice among the paths and the tie-broken traceback.  Nothing here asks
the device anything; the graph comes in as (lnz, rows of every path) — graph_paths() reads both from the host-side graph handle."""
import numpy as np

NEG = -(1 << 29)
ALPHA = "ACGTN"


def graph_node_ids(graph):
    """Segment id of every graph row (0 for row 0 and for 'F'), from the host-side graph handle (dump 3)."""
    ids = [int(x) for x in graph.dump(3).split(",")]
    ids[0] = 0
    return ids + [0]


def graph_paths(graph):
    """(lnz, [graph rows of path k in path order]) of an api.Graph (host data only: dump 0 and dump 30)."""
    lnz = graph.dump(0)
    body = graph.dump(30).split(";")
    rows = [[int(x) for x in part.split(",")] for part in body[1:] if part]
    assert len(rows) == graph.paths_number
    return lnz, rows


def canonical(read):
    return read.upper().replace("-", "N")


def default_scores(m=2, x=-4):
    """scores[a * 6 + b] of score_matrix.rs:35-51 (the '-' entries are not read by the rule)."""
    t = [m if i == j else (2 * x if 5 in (i, j) else x) for i in range(6) for j in range(6)]
    t[4 * 6 + 4] = x
    return t


def _codes(s):
    return np.array([ALPHA.index(c) for c in s], dtype=np.int64)


def _row(Hp, Yp, srow, o, e, ej, semi):
    """Row i from row i - 1: (H, X, Y, D), along the last axis (one path, or one path per leading index).  srow[..., j]:
    sc(b_i, s_j) for j >= 1 (srow[..., 0] unused)."""
    Y = np.maximum(Hp + o + e, Yp + e)
    D = np.full_like(Hp, NEG)
    D[..., 1:] = Hp[..., :-1] + srow[..., 1:]
    Hq = np.maximum(D, Y)
    if semi:
        Hq[..., 0] = 0
        Y[..., 0] = NEG
    # X[j] = max_{k < j} (H'[k] + o + e (j - k)): exact because o <= 0 (a gap opened out of a gap never beats extending it)
    z = Hq - ej
    run = np.empty_like(z)
    run[..., 0] = NEG
    run[..., 1:] = np.maximum.accumulate(z, axis=-1)[..., :-1]
    X = run + o + ej
    X[..., 0] = NEG
    return np.maximum(Hq, X), X, Y, D


def _table(scores):
    t = np.array(scores, dtype=np.int64).reshape(6, 6)
    return t[:5, :5]


def path_rows(bases, read, scores, o, e, semi, keep):
    """H of every row for one path: keep=False -> the last column only (m + 1 values); keep=True -> (H, X, Y, D) as (m + 1) x (n + 1)."""
    sc = _table(scores)
    rc = _codes(read)
    n = len(read)
    ej = e * np.arange(n + 1, dtype=np.int64)
    H = o + ej
    H[0] = 0
    Y = np.full(n + 1, NEG, dtype=np.int64)
    last = [int(H[n])]
    full = [(H.copy(), H.copy(), Y.copy(), Y.copy())] if keep else None
    if keep:
        full[0][1][0] = NEG
    srow = np.zeros(n + 1, dtype=np.int64)
    for b in bases:
        srow[1:] = sc[ALPHA.index(b)][rc]
        H, X, Y, D = _row(H, Y, srow, o, e, ej, semi)
        last.append(int(H[n]))
        if keep:
            full.append((H, X, Y, D))
    return full if keep else last


def all_paths_last(lnz, rows, read, scores, o, e, semi):
    """(last, lens): last[k][i] = H_k[i][n] for i = 0 .. lens[k], every path advanced by the same row step at once (one path per
    leading index; a path that has ended keeps its values)."""
    sc = _table(scores)
    rc = _codes(read)
    n, P = len(read), len(rows)
    lens = np.array([len(r) for r in rows])
    M = int(lens.max())
    bc = np.full((P, M), 4, dtype=np.int64)
    for k, pr in enumerate(rows):
        bc[k, :len(pr)] = [ALPHA.index(lnz[r]) for r in pr]
    ej = e * np.arange(n + 1, dtype=np.int64)
    H = np.tile(o + ej, (P, 1))
    H[:, 0] = 0
    Y = np.full((P, n + 1), NEG, dtype=np.int64)
    last = np.full((P, M + 1), NEG, dtype=np.int64)
    last[:, 0] = H[:, n]
    srow = np.zeros((P, n + 1), dtype=np.int64)
    for t in range(M):
        act = lens > t
        srow[:, 1:] = sc[bc[:, t]][:, rc]
        Hn, _, Yn, _ = _row(H, Y, srow, o, e, ej, semi)
        H = np.where(act[:, None], Hn, H)
        Y = np.where(act[:, None], Yn, Y)
        last[act, t + 1] = Hn[act, n]
    return last, lens


def traceback(full, m_end, n, o, e, semi):
    """Ops in walk order (from the chosen cell back) as a string of D / U / L, by the tie rules of the header."""
    H = [f[0] for f in full]
    X = [f[1] for f in full]
    Y = [f[2] for f in full]
    D = [f[3] for f in full]
    i, j, state, ops = m_end, n, "H", []
    while True:
        if semi and j == 0:
            break
        if i == 0 and j == 0:
            break
        if i == 0:                       # row 0: only X is finite
            ops.append("L"); j -= 1; continue
        if j == 0:                       # column 0 of -m 6: only Y is finite
            ops.append("U"); i -= 1; continue
        if state == "H":
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
    return "".join(ops)


def align(lnz, rows, read, scores=None, o=-4, e=-2, semi=False):
    """(score, path, end_row, ops in walk order, path bases consumed in path order) of one read (text; canonicalised here)."""
    read = canonical(read)
    assert set(read) <= set(ALPHA) and o <= 0 and e <= 0
    scores = default_scores() if scores is None else scores
    n = len(read)
    last, lens = all_paths_last(lnz, rows, read, scores, o, e, semi)
    best = None                          # (score, -row, -path) maximised
    for k, pr in enumerate(rows):
        col = [int(v) for v in last[k, :lens[k] + 1]]
        if not semi:
            cand = (col[-1], 0, -k, len(pr))
        else:
            v = max(col[1:])
            i = 1 + col[1:].index(v)    # the first row that attains it
            cand = (v, -pr[i - 1], -k, i)
        if best is None or cand[:3] > best[:3]:
            best = cand
    score, _, negk, m_end = best
    k = -negk
    pr = rows[k]
    bases = [lnz[r] for r in pr[:m_end]]
    full = path_rows(bases, read, scores, o, e, semi, keep=True)
    assert int(full[m_end][0][n]) == score
    ops = traceback(full, m_end, n, o, e, semi)
    used = sum(1 for c in ops if c in "DU")
    return score, k, pr[m_end - 1], ops, "".join(bases[m_end - used:])


def cigar_of(ops, pseq, read):
    """The CIGAR the formatter prints for walk-order ops: D -> M (X on a mismatch), U -> I, L -> D, run-length coded."""
    read = canonical(read)
    out, pi, ri = [], 0, 0
    fwd = ops[::-1]
    # a semiglobal walk consumes the whole read but only `pseq` of the path
    for c in fwd:
        if c == "D":
            out.append("M" if pseq[pi] == read[ri] else "X"); pi += 1; ri += 1
        elif c == "U":
            out.append("I"); pi += 1
        else:
            out.append("D"); ri += 1
    assert pi == len(pseq) and ri == len(read)
    s, i = "", 0
    while i < len(out):
        j = i
        while j < len(out) and out[j] == out[i]:
            j += 1
        s += "%d%s" % (j - i, out[i])
        i = j
    return s


def comments(lnz, rows, read, scores=None, o=-4, e=-2, semi=False):
    """The comments column of the expected line: "<cigar>, best path: k, score: S\\t<path bases>"."""
    score, k, _, ops, pseq = align(lnz, rows, read, scores, o, e, semi)
    return "%s, best path: %d, score: %d\t%s" % (cigar_of(ops, pseq, read), k, score, pseq)


def line(lnz, rows, node_ids, name, read, scores=None, o=-4, e=-2, semi=False):
    """The whole expected GAF line.  Path string and coordinates as the walkers derive them from (best path, end row, ops): the walk
    consumes the rows of the path that end at end_row; the row it stops on, i, gives start = i + 1 (0 when it reaches row 0);
    path_start is the offset of `start` inside its segment, path_end = path_start + consumed - 1, path_length = path_end + what
    is left of end_row's segment + 1."""
    score, k, end_row, ops, pseq = align(lnz, rows, read, scores, o, e, semi)
    pr, L = rows[k], len(lnz)
    m_end = pr.index(end_row) + 1
    used = len(pseq)
    consumed = pr[m_end - used:m_end]
    ids = [node_ids[r] for r in consumed]
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
    n = len(read)
    return "%s\t%d\t0\t%d\t+\t>%s\t%d\t%d\t%d\t0\t*\t*\t%s, best path: %d, score: %d\t%s\n" % (
        name, n, n - 1, ">".join(str(x) for x in ids), pend + tail + 1, head, pend, cigar_of(ops, pseq, read), k, score, pseq)


def rescore(cigar, pseq, read, scores=None, o=-4, e=-2):
    """Score of a printed CIGAR against the printed path bases, independently of any tie rule: (score, read bases consumed, path
    bases consumed).  I and D runs cost o + e * length each."""
    import re
    read = canonical(read)
    sc = _table(default_scores() if scores is None else scores)
    total, pi, ri = 0, 0, 0
    for cnt, op in re.findall(r"(\d+)([MXID])", cigar):
        cnt = int(cnt)
        if op in "MX":
            for _ in range(cnt):
                assert (pseq[pi] == read[ri]) == (op == "M"), (cigar, pi, ri)
                total += int(sc[ALPHA.index(pseq[pi])][ALPHA.index(read[ri])])
                pi += 1; ri += 1
        elif op == "I":
            total += o + e * cnt; pi += cnt
        else:
            total += o + e * cnt; ri += cnt
    return total, ri, pi


def naive_scores(bases, read, scores, o, e, semi):
    """Plain scalar Gotoh (no scan, no numpy): H of the last column per row — the check of the rule's own row step."""
    sc = _table(scores)
    read = canonical(read)
    n, m = len(read), len(bases)
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    X = [[NEG] * (n + 1) for _ in range(m + 1)]
    Y = [[NEG] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, n + 1):
        X[0][j] = o + e * j
        H[0][j] = X[0][j]
    for i in range(1, m + 1):
        if semi:
            H[i][0] = 0
        else:
            Y[i][0] = o + e * i
            H[i][0] = Y[i][0]
        for j in range(1, n + 1):
            Y[i][j] = max(H[i - 1][j] + o + e, Y[i - 1][j] + e)
            X[i][j] = max(H[i][j - 1] + o + e, X[i][j - 1] + e)
            H[i][j] = max(H[i - 1][j - 1] + int(sc[ALPHA.index(bases[i - 1])][ALPHA.index(read[j - 1])]), Y[i][j], X[i][j])
    return [H[i][n] for i in range(m + 1)]
