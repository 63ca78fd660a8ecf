"""What the windowed layer rebuild (recgraph_amd/csrc/layer_window/: k_layer_win<C, CW>, walked by k_trace of rg_pathwise.hip) owes,
stated in numpy for tests/test_layer_window_rule_cpu.py and tests/test_gpu_layer_window_walks.py.  Nothing of the rule asks the device
or the library anything; the three names at the end are what the two GPU test modules of the window share to run a batch.

The contract is the one of the kernel's header comment and of rg_layer_window.hpp, restated for the one case where the walked path
is the alpha of every row it visits: a graph with exactly ONE path.  There the rebuilt values are plain linear-gap Needleman-Wunsch
of the read against the path, g = scores[5]:

  source of a cell (RowOps16::alpha)   d = A[t-1][c-1] + s, u = A[t-1][c] + g: D on d >= u; L only where A[t][c-1] + g is strictly
                                       larger than max(d, u).  Column 0 takes U and holds t g (0 when semi); row 0 holds c g.
  window of layer row t                [left(t), left(t) + W), left = layer_window_left(start_col, t_start, t, W, wpad), wpad = 64 C,
                                       C in {4, 8, 16} from the longest read of the batch.  The start cell is (rows of the path, n);
                                       semi: (the first row that attains the maximum of the last column, n).
  known                                row 0 at every window column <= n.  A cell of row t inside window(t) is known iff the source
                                       the sweep names is known AS ROW t SEES IT: a value of row t - 1 at column c' counts only if c'
                                       lies in window(t - 1) and in window(t) (an entering block starts unknown, the lane at the left
                                       edge reads unknown to its left); an L cell needs c - 1 >= left(t) and (t, c - 1) known.
  decision of (t, c), c >= 1           stored iff (t-1, c-1), (t-1, c) and (t, c-1) are all known in that sense, else 0; the stored
                                       value is 1 if d attains max(d, u, l), else 2 if u does, else 3 — which is the sweep's source.
  verdict                              fall back if the start cell is unknown; else walk from it while t > 0 and j > 0 and fall back
                                       on a column outside window(t) or on a code 0."""
import re

import numpy as np

ALPHA = "ACGTN"
D, U, L = 1, 2, 3


def columns_per_lane(n):
    """C of a batch whose longest read has n bases (plan_pathwise; the windowed kernels exist for C <= 16, n <= 1023)."""
    C = 4
    while C * 64 < n + 1:
        C *= 2
    assert C <= 16, n
    return C


def layer_window_left(start_col, t_start, t, W, wpad):
    """rg_layer_window.hpp, restated."""
    e = start_col - (t_start - t) - W // 2
    e = min(e, wpad - W)
    e = max(e, 0)
    return e & ~3


def window_clamped(start_col, t_start, t, W, wpad):
    e = start_col - (t_start - t) - W // 2
    return e < 0 or e > wpad - W


def _codes(s):
    return np.array([ALPHA.index(c) for c in s.upper().replace("-", "N")], dtype=np.int64)


def sources(path_bases, read, scores, semi):
    """-> (src, last): src[t][c] in {D, U, L} the source the sweep names for every cell of rows 1 .. m (row 0 and column 0 filled
    with L and U, what the walk's tail does there), last[t] = A[t][n]."""
    sc = np.array(scores, dtype=np.int64).reshape(6, 6)
    g = int(scores[5])
    rc, pc = _codes(read), _codes(path_bases)
    n, m = len(rc), len(pc)
    S = sc[:, rc]                                                      # S[b][j - 1] = s(b, read[j])
    cg = g * np.arange(n + 1, dtype=np.int64)
    A = np.empty((m + 1, n + 1), dtype=np.int64)
    A[0] = cg
    du = np.empty(n + 1, dtype=np.int64)
    for t in range(1, m + 1):
        np.maximum(A[t - 1, :-1] + S[pc[t - 1]], A[t - 1, 1:] + g, out=du[1:])
        du[0] = 0 if semi else t * g
        # A[t][c] = max_k<=c (du[k] + (c - k) g): a prefix maximum of du - c g
        du -= cg
        np.maximum.accumulate(du, out=A[t])
        A[t] += cg
    d = A[:-1, :-1] + S[pc]
    u = A[:-1, 1:] + g
    src = np.empty((m + 1, n + 1), dtype=np.uint8)
    src[0] = L
    src[1:, 0] = U
    src[1:, 1:] = np.where(d >= u, D, U)
    src[1:, 1:][A[1:, 1:] > np.maximum(d, u)] = L
    return src, A[:, n].copy()


class Model:
    """The windowed layers of one read against one path: which cells are known, which decisions are stored, and the walk."""

    def __init__(self, path_bases, read, scores, W, semi, wpad=None, edge_known=False):
        self.n, self.m, self.W, self.semi = len(read), len(path_bases), W, semi
        self.wpad = 64 * columns_per_lane(self.n) if wpad is None else wpad
        assert self.wpad >= self.n + 1 and W % 64 == 0
        self.src, self.last = sources(path_bases, read, scores, semi)
        n = self.n
        if semi:
            assert self.m >= 1
            self.t_start = 1 + int(np.argmax(self.last[1:]))          # the first row that attains the maximum
        else:
            self.t_start = self.m
        self.score = int(self.last[self.t_start])
        ts = self.t_start
        self.left = [layer_window_left(n, ts, t, W, self.wpad) for t in range(ts + 1)]
        # `edge_known` is NOT the contract: it lets the column left of the window count as known, the mistake the tests must notice
        self.edge_known = edge_known
        K = np.zeros((ts + 1, n + 2), dtype=bool)                     # (column n + 1: a spare so that slices need no clipping)
        lo = self.left[0]
        K[0, lo:min(lo + W, n + 1)] = True
        cols = np.arange(n + 2)
        for t in range(1, ts + 1):
            lo = self.left[t]
            hi = min(lo + W, n + 1)                                   # columns beyond the read feed nothing the walk reads
            if hi <= lo:
                continue
            prev = self._prev(K, t)
            s = self.src[t, lo:hi]
            c = cols[lo:hi]
            base = np.where(s == U, prev[c], prev[c - 1])             # (column 0 takes U; prev[-1] is the spare: never known)
            # an L cell takes the nearest non-L column to its left INSIDE the window; none: unknown
            nonl = s != L
            idx = np.maximum.accumulate(np.where(nonl, np.arange(hi - lo), -1))
            known = np.where(idx >= 0, base[np.maximum(idx, 0)], False)
            if self.edge_known and lo > 0:
                known = np.where(idx >= 0, known, True)
            K[t, lo:hi] = known
        self.K = K

    def _prev(self, K, t):
        """Row t - 1 as row t sees it: its known cells inside window(t) (K[t - 1] is empty outside window(t - 1))."""
        lo = self.left[t]
        prev = K[t - 1].copy()
        prev[:lo] = False
        prev[lo + self.W:] = False
        if self.edge_known and lo > 0:
            prev[lo - 1] = True
        return prev

    def in_window(self, t, c):
        return self.left[t] <= c < self.left[t] + self.W

    def decision(self, t, c):
        """The stored code of (t, c), t >= 1, c >= 1: 0 unless all three inputs are known."""
        if not self.in_window(t, c):
            return 0
        lo = self.left[t]
        pk = lambda x: bool(self.K[t - 1][x]) and lo <= x < lo + self.W
        if self.edge_known and c - 1 == lo - 1:
            return int(self.src[t][c]) if pk(c) else 0
        if c - 1 < lo:
            return 0
        return int(self.src[t][c]) if pk(c - 1) and pk(c) and self.K[t][c - 1] else 0

    def tail(self, t, j):
        return "L" * j + ("" if self.semi else "U" * t)

    def true_walk(self):
        """Ops in walk order (from the start cell back) by the sweep's sources alone, and the largest |j - centre(t)| over the cells
        of the walk whose row's window is not clamped."""
        t, j, ops, exc = self.t_start, self.n, [], 0
        while t > 0 and j > 0:
            if not window_clamped(self.n, self.t_start, t, self.W, self.wpad):
                exc = max(exc, abs(j - (self.n - (self.t_start - t))))
            s = int(self.src[t][j])
            ops.append("DUL"[s - 1])
            if s != L:
                t -= 1
            if s != U:
                j -= 1
        return "".join(ops) + self.tail(t, j), exc

    def verdict(self):
        """-> (falls_back, why, excursion, ops of the windowed walk or None)"""
        ops_true, exc = self.true_walk()
        if not self.K[self.t_start][self.n]:
            return True, "start cell unknown", exc, None
        t, j, ops = self.t_start, self.n, []
        while t > 0 and j > 0:
            if not self.in_window(t, j):
                return True, "column %d outside the window of row %d" % (j, t), exc, None
            s = self.decision(t, j)
            if s == 0:
                return True, "code 0 at (%d, %d)" % (t, j), exc, None
            ops.append("DUL"[s - 1])
            if s != L:
                t -= 1
            if s != U:
                j -= 1
        ops = "".join(ops) + self.tail(t, j)
        assert ops == ops_true
        return False, "", exc, ops


_SEEN = {}


def analyse(path_bases, read, scores, W, semi, wpad=None):
    """-> dict(falls_back, why, excursion, ops: the windowed walk or None, true_ops: the walk by the sources alone, score, t_start).
    wpad: 64 x the columns per lane of the BATCH (its longest read decides); default: of this read.  Kept per argument tuple: the tests
    of one session ask for the same reads more than once."""
    key = (path_bases, read, tuple(scores), W, semi, wpad)
    if key not in _SEEN:
        m = Model(path_bases, read, scores, W, semi, wpad)
        fb, why, exc, ops = m.verdict()
        _SEEN[key] = dict(falls_back=fb, why=why, excursion=exc, ops=ops, true_ops=m.true_walk()[0], score=m.score, t_start=m.t_start)
    return _SEEN[key]


def window_verdict(path_bases, read, scores, W, semi, wpad=None):
    """-> (falls_back, why, excursion)"""
    r = analyse(path_bases, read, scores, W, semi, wpad)
    return r["falls_back"], r["why"], r["excursion"]


def walk_leaves_window(ops, t_start, n, W, wpad=None):
    """Does a walk (ops in walk order: D, U, L from the start cell (t_start, n) back) visit a cell (t, j), t > 0 and j > 0, outside
    window(t)?  k_trace reads code 0 there: a necessary condition for falling back, on any graph."""
    wpad = 64 * columns_per_lane(n) if wpad is None else wpad
    t, j = t_start, n
    for op in ops:
        if t <= 0 or j <= 0:
            break
        lo = layer_window_left(n, t_start, t, W, wpad)
        if not lo <= j < lo + W:
            return True
        if op != "L":
            t -= 1
        if op != "U":
            j -= 1
    return False


def walk_excursion(ops, t_start, n, W, wpad=None):
    """Largest |j - centre(t)| over the cells (t > 0, j > 0) of a walk whose row's window is not clamped."""
    wpad = 64 * columns_per_lane(n) if wpad is None else wpad
    t, j, exc = t_start, n, 0
    for op in ops:
        if t <= 0 or j <= 0:
            break
        if not window_clamped(n, t_start, t, W, wpad):
            exc = max(exc, abs(j - (n - (t_start - t))))
        if op != "L":
            t -= 1
        if op != "U":
            j -= 1
    return exc


def cigar_ops(text):
    """Walk-order ops of a printed record: its CIGAR (M / X -> D, I -> U, D -> L) read backwards."""
    cigar = text.split("\t")[12].split(",")[0]
    fwd = "".join({"M": "D", "X": "D", "I": "U", "D": "L"}[op] * int(cnt) for cnt, op in re.findall(r"(\d+)([MXID])", cigar))
    return fwd[::-1]


def record_score(text):
    return int(re.search(r"score: (-?\d+)", text).group(1))


def one_path_gfa(path_bases, seg=1):
    """A graph with exactly one path: segments of `seg` bases (the last one takes the rest)."""
    segs = [path_bases[i:i + seg] for i in range(0, len(path_bases), seg)]
    out = ["H\tVN:Z:1.0"] + ["S\t%d\t%s" % (i + 1, s) for i, s in enumerate(segs)]
    out += ["L\t%d\t+\t%d\t+\t0M" % (i, i + 1) for i in range(1, len(segs))]
    out.append("P\tpath0\t" + ",".join("%d+" % (i + 1) for i in range(len(segs))) + "\t*")
    return "\n".join(out) + "\n"


# ---------------------------------------------------------------------------------------------------------------------------------
# Read families: walks that wander inside the window and graze its edge.  A read is a path with EVENTS applied: (position in the
# path, +k: k random bases inserted there | -k: the k path bases from there deleted), positions ascending.
SHAPES = ((200, 128), (300, 128), (300, 256), (1000, 128), (1000, 256))      # (n, W): the smallest at which a window exists
FAMILIES = ("drift_del", "drift_ins", "excursion", "staircase", "lane_wrap", "clamp_start", "clamp_end")


def rand_bases(rng, k):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=k))


def apply_events(p, events, rng):
    out, at = [], 0
    for pos, k in events:
        assert at <= pos <= len(p), (events, len(p))
        out.append(p[at:pos])
        at = pos
        if k > 0:
            out.append(rand_bases(rng, k))
        else:
            at = pos - k
            assert at <= len(p), (events, len(p))
    out.append(p[at:])
    return "".join(out)


def drifts(W):
    h = W // 2
    return (1, 8, 30, h - 16, h - 8, h - 4, h - 2, h, h + 2, h + 4, h + 8, h + 36)


def path_lengths(n, W):
    """(long, short): reads that lose bases against their path sit on the long one, reads that gain bases on the short one, so that
    every read of a batch keeps the columns per lane of n and the longest one comes near the last column of the last lane."""
    cap = 64 * columns_per_lane(n) - 1
    dmax = W // 2 + 36
    long_ = min(n + dmax, n + 150, cap)
    return long_, long_ - dmax


def family_events(family, n, W):
    """-> [(which path: "long" | "short", events)], at most 12 reads."""
    Ll, Ls = path_lengths(n, W)
    h = W // 2
    out = []
    if family == "drift_del":
        out = [("long", [(Ll // 2, -d)]) for d in drifts(W)]
    elif family == "drift_ins":
        out = [("short", [(Ls // 2, d)]) for d in drifts(W)]
    elif family == "excursion":
        # deletion of d, 4 d + 60 path bases, insertion of d (and the mirror order): the separation keeps the optimal alignment
        # from going diagonally through mismatches instead.  Centred on the path; events that do not fit it are left out.
        for d in (24, 40, h - 8, h, h + 8):
            span = 5 * d + 60
            a = max(20, (Ll - span) // 2)
            if a + span + 20 > Ll:
                continue
            out.append(("long", [(a, -d), (a + span, d)]))
            out.append(("long", [(a, d), (a + 4 * d + 60, -d)]))
    elif family == "staircase":
        # k indels of 8 bases, one every 50 bases, all in the same direction
        for k in (1, 4, W // 16 - 1, W // 16, W // 16 + 1, (h + 36) // 8):
            for which, LL, sign in (("long", Ll, -1), ("short", Ls, 1)):
                a = max(30, (LL - 50 * k) // 2)
                if a + 50 * k + 10 <= LL:
                    out.append((which, [(a + 50 * i, 8 * sign) for i in range(k)]))
    elif family == "lane_wrap":
        # the L run of an insertion covers a read column that is a multiple of W (where block -> lane wraps from lane 63 to lane 0), the
        # same run W / 4 to either side (other phases of the window), and each with a deletion of 20 some 100 bases later (the run is
        # met off-centre)
        k = max(1, int(round(Ls / 2.0 / W)))
        for d in (30, 70):
            for shift in (0, W // 4, -(W // 4)):
                a = k * W - d // 2 + shift
                if a + 10 > Ls:                      # (the shortest shape has no room to the right of its only multiple of W)
                    continue
                out.append(("short", [(a, d)]))
                if a + 120 <= Ls:
                    out.append(("short", [(a, d), (a + 100, -20)]))
    elif family == "clamp_start":
        for k in (40, 100):
            for at in (20, 70):
                out.append(("long", [(at, -k)]))
                out.append(("short", [(at, k)]))
    elif family == "clamp_end":
        for k in (40, 100):
            for at in (20, 70):
                out.append(("long", [(Ll - at - k, -k)]))
                out.append(("short", [(Ls - at, k)]))
    else:
        raise ValueError(family)
    assert 0 < len(out) <= 12, (family, n, W, len(out))
    return out


def semi_events(n, W):
    h = W // 2
    Ll, Ls = path_lengths(n, W)
    out = [("long", [(Ll // 2, -d)]) for d in (8, h - 8, h, h + 36)] + [("short", [(Ls // 2, d)]) for d in (8, h - 8, h, h + 36)]
    k = max(1, int(round(Ls / 2.0 / W)))
    out += [("short", [(k * W - d // 2 + shift, d)]) for d in (30, 70) for shift in (0, W // 4) if k * W - d // 2 + shift + 10 <= Ls]
    return out


def family_reads(family, n, W, seed=0):
    """-> [(path bases, [reads], semi)]: one batch per entry, every batch on a graph of its one path.  "semi": -m 5 pieces of a path
    with 60 more bases at either end, carrying the drift and lane-wrap events."""
    rng = np.random.default_rng(1000 * n + W + seed)
    Ll, Ls = path_lengths(n, W)
    base = rand_bases(rng, Ll)
    if family == "semi":
        path = rand_bases(rng, 60) + base + rand_bases(rng, 60)
        return [(path, [apply_events(base[:Ll if which == "long" else Ls], ev, rng) for which, ev in semi_events(n, W)], True)]
    groups = {"long": [], "short": []}
    for which, ev in family_events(family, n, W):
        groups[which].append(apply_events(base[:Ll if which == "long" else Ls], ev, rng))
    return [(base[:Ll if which == "long" else Ls], reads, False) for which, reads in groups.items() if reads]


def batch_wpad(reads):
    return 64 * columns_per_lane(max(len(r) for r in reads))


def shape_census(scores, n, W):
    """(reads that fall back, reads that do not, of those: with an excursion >= W / 4) over the global families of one (n, W)."""
    fb = ok = wide = 0
    for family in FAMILIES:
        for path, reads, semi in family_reads(family, n, W):
            wpad = batch_wpad(reads)
            for rd in reads:
                r = analyse(path, rd, scores, W, semi, wpad)
                fb += r["falls_back"]
                ok += not r["falls_back"]
                wide += (not r["falls_back"]) and r["excursion"] >= W // 4
    return fb, ok, wide


# ---- shared by tests/test_gpu_layer_window.py and tests/test_gpu_layer_window_walks.py ----

LOG = "mem:layer_window:"      # the pseudo-statistic that names the windowed kernel ("inst:" belongs to tests/kernel_matrix.py)


def oracle_mode(oracle, mode):
    return {4: oracle.M4_ABS, 5: oracle.M5_ABS, 8: oracle.M8_ABS, 9: oracle.M9_ABS}[mode]


def align_windowed(gg, reads, mode, window):
    """(texts, kernel statistics) of one batch under layer_window = `window` (0: the full-width kernels); the default is put back."""
    from recgraph_amd import api
    try:
        api.set_option("layer_window", window)
        b = api.Batch(gg, reads, api.make_params(mode))
        b.run()
        b.fetch()
        texts = [b.gaf_text(i, "r", 1) for i in range(len(reads))]
        stats = b.kernel_stats()
    finally:
        api.set_option("layer_window", 256)
    return texts, stats
