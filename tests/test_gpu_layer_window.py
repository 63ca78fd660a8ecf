"""GPU: the traceback layers rebuilt inside a column window (recgraph_amd/csrc/layer_window/) give the bytes of the full-width
kernels and of the oracle.

Every case aligns its reads three ways — window on (option layer_window = 128 | 256), window off (0: the kernels of before), and
the CPU oracle — and all three texts must be equal, read by read.  `mem:layer_window:<instantiation>` says which k_layer_win ran
(tests/kernel_matrix_layer_window.py), `mem:layer_full_reads` how many reads the window could not serve and were rebuilt at full
width (k_layer_full / k_trace_full).

  short      reads of 100-255 bases, 6 paths, -m 8 and -m 4, window 256: the window covers the row, nothing falls back
  config5    1000-base reads, 1 % substitutions, half of them mosaics of two paths, window 256: nothing falls back
  indels     300-base reads with ONE 100-base deletion / insertion against their path, window 128: the walk leaves the window,
             the reads fall back, the bytes stay
  edges-*    -m 9 / -m 5 (the alignment starts inside the graph), a 1023-base read, recombinations in the last 20 columns,
             300-base reads; window 128 and 256
  stream     three 40-read tiles, chunk_reads 24, reads of the config5 and the indel kind mixed; input order kept"""
import numpy as np
import pytest

import kernel_matrix_layer_window as KW
from layer_window_rule import LOG, align_windowed as _gpu, oracle_mode as _omode

pytestmark = pytest.mark.gpu
_ORACLE = {}      # (graph key, oracle mode, read) -> text with name "r", index 1
_RESULTS = {}


def _graph(key):
    from recgraph_amd import synth
    rows, paths, plen, seed = key
    return synth.haplotype_graph(rows, paths, path_len=plen, seed=seed)


def _subst(rng, s, rate=0.01):
    s = list(s)
    for i in range(len(s)):
        if rng.random() < rate:
            s[i] = "ACGT"[("ACGT".index(s[i]) + int(rng.integers(1, 4))) % 4]
    return "".join(s)


def _rand(rng, k):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=k))


def _fit(rng, s, length):
    return s[:length] if len(s) >= length else s + _rand(rng, length - len(s))


def mosaic_reads(g, count, length, seed):
    """Reads of the config-5 kind without indels: a path, or (every other read) the head of one path and the tail of another."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        a = g.path_sequence(int(rng.integers(0, len(g.paths))))
        if i % 2:
            b = g.path_sequence(int(rng.integers(0, len(g.paths))))
            f = 0.2 + 0.6 * rng.random()
            a = a[:int(f * len(a))] + b[int(f * len(b)):]
        out.append(_subst(rng, _fit(rng, a, length)))
    return out


def indel_reads(g, count, length, seed, indel=100):
    """Reads of `length` bases that carry one `indel`-base deletion (even reads) or insertion (odd reads) against their path."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        p = g.path_sequence(int(rng.integers(0, len(g.paths))))
        cut = len(p) // 4 + int(rng.integers(0, len(p) // 4))
        s = p[:cut] + (p[cut + indel:] if i % 2 == 0 else _rand(rng, indel) + p[cut:])
        out.append(_subst(rng, _fit(rng, s, length), 0.005))
    return out


def _check(oracle, gkey, reads, mode, window, want_full=None):
    """-> (instantiations of k_layer_win launched, reads that fell back)"""
    from recgraph_amd import api
    g = _graph(gkey)
    gg = api.Graph.from_gfa_text(g.gfa())
    if ("og", gkey) not in _ORACLE:
        _ORACLE[("og", gkey)] = oracle.Graph.from_gfa_text(g.gfa())
    og = _ORACLE[("og", gkey)]
    exp = []
    for rd in reads:
        k = (gkey, mode, rd)
        if k not in _ORACLE:
            _ORACLE[k] = og.align(_omode(oracle, mode), rd, name="r", idx=1)[0]
        exp.append(_ORACLE[k])
    on, stats = _gpu(gg, reads, mode, window)
    off, stats0 = _gpu(gg, reads, mode, 0)
    full = int(stats.get("mem:layer_full_reads", (0, 0))[0])
    insts = {k[len(LOG):] for k in stats if k.startswith(LOG)}
    assert not any(k.startswith("inst:") and "k_layer_win" in k for k in stats)
    print("layer window %d, -m %d, %d reads of %d-%d bases: %s, full-width reads %d" % (window, mode, len(reads), min(map(len, reads)), max(map(len, reads)),
                                                                                      sorted(insts), full))
    for i in range(len(reads)):
        assert on[i] == off[i], (mode, window, i, on[i][-300:], off[i][-300:])
        assert on[i] == exp[i], (mode, window, i, on[i][-300:], exp[i][-300:])
    # the window ran (and with it the fallback launches), the old route did not see it
    assert insts and {"k_layer_full", "k_trace_full", "mem:layer_full_reads"} <= set(stats), sorted(stats)
    assert not any("k_layer_win" in k or k in ("k_layer_full", "k_trace_full", "mem:layer_full_reads") for k in stats0), sorted(stats0)
    if want_full == 0:
        assert full == 0, full
    elif want_full:
        assert full >= want_full, full
    return insts, full


def _case_short(oracle):
    gkey = (600, 6, 255, 5)
    whole = mosaic_reads(_graph(gkey), 6, 255, 100)
    reads = [rd[:n] for rd, n in zip(whole, (100, 137, 200, 254, 255, 255))]
    insts = set()
    for mode in (8, 4):
        insts |= _check(oracle, gkey, reads, mode, 256, want_full=0)[0]
    return insts


def _case_config5(oracle):
    gkey = (1500, 4, 1000, 7)
    reads = mosaic_reads(_graph(gkey), 8, 1000, 77)
    return _check(oracle, gkey, reads, 8, 256, want_full=0)[0]


def _case_indels(oracle):
    insts = set()
    # deletions against 400-base paths and insertions against 200-base paths: 300 bases either way
    gdel, gins = (500, 4, 400, 9), (260, 4, 200, 10)
    dels = indel_reads(_graph(gdel), 8, 300, 90)[0::2]
    inss = indel_reads(_graph(gins), 8, 300, 91)[1::2]
    # -m 8 owes no fallback for either kind: a recombination bridges a deletion (forward displacement) and an insertion (the
    # inserted bases go diagonally against the next 100 rows, a recombination steps 100 rows back), two walks that each stay on
    # their diagonal.  -m 4 has one walk on one path.  Insertion: 300 bases against 200 rows need 100 L steps, the walk ends 100
    # columns LEFT of its diagonal, 36 beyond the window's edge at columns >= 50: every read falls back.  Deletion: 100 U steps, 100
    # columns RIGHT of the diagonal, which leaves the window only where the deletion lies beyond column 128 — the window never
    # starts left of column 0, and a cut at columns 100 .. 199 can lie inside [0, 128): at least one read (what the case is
    # specified to assert), not all.
    for gkey, reads, modes in ((gdel, dels, ((8, None), (4, 1))), (gins, inss, ((8, None), (4, len(inss))))):
        for mode, want in modes:
            i, full = _check(oracle, gkey, reads, mode, 128, want_full=want)
            insts |= i
    return insts


def _edge_reads():
    g1023, g300, gshort = (1300, 3, 1023, 11), (400, 4, 300, 12), (300, 4, 200, 13)
    rng = np.random.default_rng(5)
    sets = []
    # a read of 1023 bases (the last column of the last lane), whole paths and a recombination in the last 20 columns
    g = _graph(g1023)
    a, b = g.path_sequence(0), g.path_sequence(2)
    sets.append((g1023, [_fit(rng, a, 1023), _subst(rng, _fit(rng, a[:len(a) - 12] + b[len(b) - 12:], 1023)), _subst(rng, _fit(rng, b[:len(b) - 18] + a[len(a) - 18:], 1023))], (8, 9)))
    g = _graph(g300)
    a, b = g.path_sequence(1), g.path_sequence(3)
    sets.append((g300, [_fit(rng, a, 300), _fit(rng, a[:len(a) - 15] + b[len(b) - 15:], 300), _subst(rng, _fit(rng, b[:150] + a[150:], 300)), a[40:340][:300]], (8, 9, 5)))
    # semiglobal: pieces from inside a path (the alignment starts inside the graph)
    g = _graph(gshort)
    a = g.path_sequence(2)
    sets.append((gshort, [a[60:160], _subst(rng, a[30:180]), a[100:], a[:120]], (9, 5)))
    return sets


def _case_edges(oracle, window):
    """None of these reads carries an indel of more than the 40 leading bases one of them skips, so no walk drifts 64 columns from
    its diagonal: no read may fall back at either width — a windowed kernel that stored code 0 everywhere would still give the
    right bytes through the fallback, and only this count shows it."""
    insts = set()
    for gkey, reads, modes in _edge_reads():
        for mode in modes:
            insts |= _check(oracle, gkey, reads, mode, window, want_full=0)[0]
    # reads of at most 127 bases: the 128-column window covers the row
    gkey = (300, 4, 120, 14)
    g = _graph(gkey)
    tiny = [g.path_sequence(k)[:n] for k, n in ((0, 127), (1, 100), (2, 64), (3, 1))]
    for mode in (8, 4):
        insts |= _check(oracle, gkey, tiny, mode, window, want_full=0)[0]
    return insts


_CASES = {"short": _case_short, "config5": _case_config5, "indels": _case_indels,
          "edges-128": lambda o: _case_edges(o, 128), "edges-256": lambda o: _case_edges(o, 256)}


@pytest.mark.parametrize("cid", KW.CASES)
def test_windowed_layers_give_the_same_bytes(oracle, cid):
    _RESULTS[cid] = _CASES[cid](oracle)
    for name, case in KW.MATRIX.items():
        if case == cid:
            assert name in _RESULTS[cid], (name, cid, sorted(_RESULTS[cid]))


def test_a_stream_of_mixed_reads_keeps_its_order(oracle):
    from recgraph_amd import api
    gkey = (1300, 3, 1000, 21)
    g = _graph(gkey)
    a = mosaic_reads(g, 8, 1000, 31)
    b = indel_reads(g, 8, 1000, 32)
    distinct = [x for pair in zip(a, b) for x in pair]
    reads = [distinct[(7 * i) % len(distinct)] for i in range(120)]
    og = oracle.Graph.from_gfa_text(g.gfa())
    exp1 = {rd: og.align(oracle.M4_ABS, rd, name="r", idx=1)[0] for rd in distinct}
    gg = api.Graph.from_gfa_text(g.gfa())
    names = ["r"] * len(reads)
    out, full = {}, {}
    try:
        api.set_option("chunk_reads", 24)
        # (-m 4, window 128.  An insertion read is path[:cut] + 100 random bases + path[cut:900] against ~1000 rows: the last ~100
        # rows have no bases left, the walk opens with ~100 U steps at the last column and stands ~100 columns right of its diagonal,
        # 36 beyond the window: it falls back, inside the stream's chunks)
        for window in (128, 0):
            api.set_option("layer_window", window)
            st = api.Stream(gg, api.make_params(api.MODE_PATHWISE), device_ids=[0], handles_per_device=2, tile_reads=40)
            st.push(reads, names)
            st.finish()
            out[window] = [t.text_of(i).decode() for t in st for i in range(t.n)]
            stats = st.kernel_stats()
            st.close()
            full[window] = stats.get("mem:layer_full_reads", (0, 0))[0]
    finally:
        api.set_option("chunk_reads", 0)
        api.set_option("layer_window", 256)
    print("stream, window 128: full-width reads %d of 120" % full[128])
    assert len(out[128]) == 120
    # 16 distinct reads, each 7 or 8 times: the 4 insertion reads must fall back
    assert full[128] >= 28 and full[0] == 0, full
    for i, rd in enumerate(reads):
        assert out[128][i] == out[0][i], i
        assert out[128][i] == exp1[rd], (i, out[128][i][-200:], exp1[rd][-200:])
