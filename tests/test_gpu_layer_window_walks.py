"""GPU: the windowed traceback layers (recgraph_amd/csrc/layer_window/) under walks that WANDER inside the window and graze its edge.

tests/test_gpu_layer_window.py drives k_layer_win with reads that walk the centre diagonal (nothing unknown is ever near) and with
reads that leave the window at once (the full-width fallback gives their bytes).  Here the walk drifts 8 to W / 2 + 36 columns, goes
off and comes back, climbs in steps of 8, runs left across the column where block -> lane wraps from lane 63 to lane 0, and carries
its indels inside the zones where the window is clamped.  Every case aligns its reads three ways — window on, layer_window = 0, the CPU
oracle — and all three texts must be equal, read by read.

  (a) graphs with ONE path, -m 4 and -m 5 (family "semi"): there tests/layer_window_rule.py states which reads the window owes and
      which it may hand to the full-width kernels, and `mem:layer_full_reads` must EQUAL the rule's count — with the speculative
      bound off (no_spec) and on, which agree because on one path every read reaches its bound.  A kernel that calls too much
      unknown (right bytes through the fallback) or too little (wrong bytes, or a walk on stale codes) shows here.
  (b) graphs with several paths, -m 4 / 8 / 9 and -m 5 on pieces: bytes, and for -m 4 the provable lower bound — a read whose walk (the
      oracle's) leaves the window must fall back.  No upper bound: a member path follows its alpha's direction words, which the rule
      does not state.  The count is printed.
  (c) a stream of three 40-read tiles in chunks of 24: order kept, the batch's bytes, the rule's count over all 120 reads."""
import numpy as np
import pytest

import layer_window_rule as R
from layer_window_rule import LOG, align_windowed as _gpu, oracle_mode as _omode

pytestmark = pytest.mark.gpu
FULL = "mem:layer_full_reads"


def _scores(oracle):
    return oracle.scores_match_mis(2, -4)


def _three_ways(oracle, gfa, reads, mode, window, options=()):
    """-> (reads that fell back, oracle texts).  Window on (under `options`), window off, oracle: equal texts."""
    from recgraph_amd import api
    gg = api.Graph.from_gfa_text(gfa)
    og = oracle.Graph.from_gfa_text(gfa)
    exp = [og.align(_omode(oracle, mode), rd, name="r", idx=1)[0] for rd in reads]
    try:
        for name, value in options:
            api.set_option(name, value)
        on, stats = _gpu(gg, reads, mode, window)
    finally:
        for name, _ in options:
            api.set_option(name, 0)
    off, stats0 = _gpu(gg, reads, mode, 0)
    for i in range(len(reads)):
        assert on[i] == off[i], (mode, window, i, on[i][-300:], off[i][-300:])
        assert on[i] == exp[i], (mode, window, i, on[i][-300:], exp[i][-300:])
    assert any(k.startswith(LOG) for k in stats) and FULL in stats, sorted(stats)
    assert not any(k.startswith(LOG) or k == FULL for k in stats0), sorted(stats0)
    return int(stats[FULL][0]), exp


def _alone(oracle, gfa, reads, mode, window, options):
    """Which reads fall back: every read in a batch of its own (to locate a difference of counts)."""
    return [_three_ways(oracle, gfa, [rd], mode, window, options)[0] for rd in reads]


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) one path: exact counts
@pytest.mark.parametrize("n,W", R.SHAPES)
def test_every_shape_holds_both_kinds_of_read(oracle, n, W):
    """The cases below cannot degenerate: per (n, W) the rule sends at least two reads to the fallback and keeps at least four, two of
    them with a walk a quarter of the window off its diagonal."""
    fb, ok, wide = R.shape_census(_scores(oracle), n, W)
    print("n %d, W %d: the rule sends %d reads to the full-width kernels and keeps %d, %d of those wander >= W / 4" % (n, W, fb, ok, wide))
    assert fb >= 2 and ok >= 4 and wide >= 2, (n, W, fb, ok, wide)


@pytest.mark.parametrize("family", R.FAMILIES + ("semi",))
@pytest.mark.parametrize("n,W", R.SHAPES)
def test_one_path_exact_fallback_counts(oracle, n, W, family):
    scores = _scores(oracle)
    want_total = got_total = 0
    for path, reads, semi in R.family_reads(family, n, W):
        wpad = R.batch_wpad(reads)
        assert wpad == 64 * R.columns_per_lane(n) and len(reads) <= 12, (family, n, W, sorted(map(len, reads)))
        mode = 5 if semi else 4
        gfa = R.one_path_gfa(path, 9)
        want = [R.window_verdict(path, rd, scores, W, semi, wpad) for rd in reads]
        for options in ((("no_spec", 1),), ()):
            got, _ = _three_ways(oracle, gfa, reads, mode, W, options)
            print("%s, n %d, W %d, -m %d%s, %d reads of %d-%d bases on a path of %d: the rule sends %d to the full-width kernels, the device %d"
                  % (family, n, W, mode, ", no_spec" if options else "", len(reads), min(map(len, reads)), max(map(len, reads)), len(path),
                     sum(v[0] for v in want), got))
            if got != sum(v[0] for v in want):
                alone = _alone(oracle, gfa, reads, mode, W, options)
                diff = [(i, len(rd), want[i], alone[i]) for i, rd in enumerate(reads) if alone[i] != int(want[i][0])]
                assert False, (family, n, W, options, got, sum(v[0] for v in want), diff)
        want_total += sum(v[0] for v in want)
        got_total += got
    assert got_total == want_total


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) several paths: bytes, and the lower bound a walk that leaves the window gives
def _dag():
    from recgraph_amd import synth
    g = synth.random_dag_graph(DAG[0], 12, seed=DAG[1])
    shortest = min(len(g.path_sequence(k)) for k in range(12))
    assert 250 <= shortest <= 350, shortest
    return g


DAG = (150, 3)
MULTI = {"hap1000": lambda: _hap(1500, 4, 1000, 7), "hap400": lambda: _hap(500, 4, 400, 9), "dag300": _dag}
MULTI_CASES = (("hap1000", 128), ("hap1000", 256), ("hap400", 128), ("dag300", 128))
_GRAPHS = {}


def _hap(rows, paths, plen, seed):
    from recgraph_amd import synth
    return synth.haplotype_graph(rows, paths, path_len=plen, seed=seed)


def _graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = MULTI[name]()
    return _GRAPHS[name]


def _centred(s, e):
    """The event e (+k: insertion, -k: deletion, of at most all but 30 bases) in the middle of s."""
    if e > 0:
        return len(s) // 2, e
    e = max(e, -(len(s) - 30))
    return (len(s) + e) // 2, e


def multi_reads(g, W, seed, piece=False):
    """At most 12 reads of at most 1023 bases on paths other than path 0: single events (deletions of 8, 30, W / 2 - 8, W / 2 + 36;
    insertions of 8 and 30; an insertion whose L run covers a column that is a multiple of W) and mosaics — the head of one path, the
    tail of another, one event in the head and one in the tail, so that -m 8 wanders in its forward and in its reverse walk.  piece:
    the paths without their first 60 and last 40 bases (-m 5 / -m 9: the alignment starts and ends inside the graph)."""
    rng = np.random.default_rng(seed)
    h = W // 2
    P = len(g.paths)
    seq = lambda k: g.path_sequence(k)[60:-40] if piece else g.path_sequence(k)
    out = []
    for i, d in enumerate((8, 30, h - 8, h + 36)):
        q = seq(1 + i % (P - 1))
        out.append(R.apply_events(q, [(len(q) // 2, -d)], rng))
    for i, d in enumerate((8, 30)):
        q = seq(1 + (i + 1) % (P - 1))
        out.append(R.apply_events(q, [(len(q) // 2, d)], rng))
    q = seq(P - 1)
    k = max(1, int(round(len(q) / 2.0 / W)))
    out.append(R.apply_events(q, [(min(k * W, len(q) - 60) - 15, 30)], rng))
    for i, (e1, e2) in enumerate(((-30, 30), (-(h - 8), 8), (8, -(h - 8)), (-(h + 36), 30), (30, -(h + 36)))):
        a, b = seq(1 + i % (P - 1)), seq((2 + i) % P)
        f = 0.4 + 0.05 * i
        head, tail = a[:int(f * len(a))], b[int(f * len(b)):]
        out.append(R.apply_events(head, [_centred(head, e1)], rng) + R.apply_events(tail, [_centred(tail, e2)], rng))
    return [rd[:1023] for rd in out]


@pytest.mark.parametrize("mode", [4, 8, 9, 5])
@pytest.mark.parametrize("gname,W", MULTI_CASES)
def test_several_paths_same_bytes_and_the_lower_bound(oracle, gname, W, mode):
    g = _graph(gname)
    reads = multi_reads(g, W, 17, piece=mode in (5, 9))
    wpad = R.batch_wpad(reads)
    options = (("no_spec", 1),) if mode == 4 else ()
    got, exp = _three_ways(oracle, g.gfa(), reads, mode, W, options)
    print("%s, W %d, -m %d, %d reads of %d-%d bases: %d took the full-width kernels" % (gname, W, mode, len(reads), min(map(len, reads)), max(map(len, reads)), got))
    if mode != 4:
        return
    # the walk of -m 4 starts at (the last row of the best path, n): t_start = the rows the walk consumes
    leaves, wide = [], []
    for rd, text in zip(reads, exp):
        ops = R.cigar_ops(text)
        t_start = ops.count("D") + ops.count("U")
        leaves.append(R.walk_leaves_window(ops, t_start, len(rd), W, wpad))
        wide.append(R.walk_excursion(ops, t_start, len(rd), W, wpad) >= W // 4)
    print("    walks that leave the window: %d, walks >= W / 4 off the diagonal that stay inside: %d" % (sum(leaves), sum(w and not l for w, l in zip(wide, leaves))))
    assert got >= sum(leaves), (got, leaves)
    assert any(leaves) and any(w and not l for w, l in zip(wide, leaves)), (leaves, wide)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) a stream
def test_a_stream_of_drifting_reads_keeps_order_bytes_and_count(oracle):
    from recgraph_amd import api
    n, W = 300, 128
    rng = np.random.default_rng(33)
    path = R.rand_bases(rng, 400)
    a = 200
    distinct = [x for d in R.drifts(W) for x in (path[:a] + path[a + d:], path[:a] + R.rand_bases(rng, d) + path[a:])]
    assert 256 <= min(map(len, distinct)) and max(map(len, distinct)) <= 511            # 8 columns per lane whatever a chunk holds
    reads = [distinct[(7 * i) % len(distinct)] for i in range(120)]
    scores = _scores(oracle)
    verdict = {rd: R.window_verdict(path, rd, scores, W, False, 512)[0] for rd in distinct}
    want = sum(verdict[rd] for rd in reads)
    assert 0 < want < 120
    gfa = R.one_path_gfa(path, 9)
    got1, exp = _three_ways(oracle, gfa, distinct, 4, W)
    assert got1 == sum(verdict.values()), (got1, sum(verdict.values()))
    exp1 = dict(zip(distinct, exp))
    gg = api.Graph.from_gfa_text(gfa)
    try:
        api.set_option("chunk_reads", 24)
        api.set_option("layer_window", W)
        st = api.Stream(gg, api.make_params(api.MODE_PATHWISE), device_ids=[0], handles_per_device=2, tile_reads=40)
        st.push(reads, ["r"] * len(reads))
        st.finish()
        out = [t.text_of(i).decode() for t in st for i in range(t.n)]
        stats = st.kernel_stats()
        st.close()
    finally:
        api.set_option("chunk_reads", 0)
        api.set_option("layer_window", 256)
    got = int(stats.get(FULL, (0, 0))[0])
    print("stream of 120 drifting reads, W %d: the rule sends %d to the full-width kernels, the device %d" % (W, want, got))
    assert len(out) == 120
    for i, rd in enumerate(reads):
        assert out[i] == exp1[rd], (i, out[i][-200:], exp1[rd][-200:])
    assert got == want, (got, want)
