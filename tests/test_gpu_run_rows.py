"""The counted row loop of k_sweep16's register runs (run_rows: an inner loop over the rows that are known to continue the run inside
the current 64-record block, an outer one per block switch, capped run field, tail or run end) changes no byte.

A counted loop can go wrong only at its bounds, so the inputs put a bound everywhere it can fall.  `bounds_graph` is hand-built:
6 paths, allele segments of 1, 2, 3, 62, 63, 64, 65, 127 and 140 rows (the run field is capped at 63: the long ones hit the cap once
and twice) in groups of 1, 2, 3 and 4 paths (every member count the run loops have a body for: by construction of the graph — the
statistics count run rows and silent rows, not the body that ran them), shared segments of 3 rows between them, every
fifth base of the 140- and the 127-row allele an N (the profile pseudo-row inside a counted stretch).  Blocks, paths -> rows:

    Q1  {1,5}: q[0]   {0}: 1   {2}: 2   {3}: 1   {4}: 2          Q2  {2,5}: q[1]   {0}: 2   {1}: 1   {3}: 2   {4}: 1
    B1  {0}: 140      {1,2}: 127        {3,4,5}: 63
    B2  {0,1,2,3}: 62 {4}: 65           {5}: 64
    B3  {0}: 1        {1}: 2   {2}: 3   {3,4,5}: 64
    P1  {1,5}: q[2]   ...as Q1          P2  {2,5}: q[3]   ...as Q2

The reads follow path 5, half of them mosaics of path 5 and another path: paths 0 - 4 go hopeless, and they still lead path 5 further
down the table in either direction (path 0 in every shared segment, 1 and 2 in the Q / P blocks, 3 and 4 in B1 / B3), so they are
computed on: their runs take the lean form, path 5's the full one.  The lengths src, q and snk were moved until the split step tables
of BOTH directions hold the five bounds `test_inputs_put_a_bound_everywhere` asserts — on the CPU, before any GPU case relies on them.

Every GPU case aligns at most 64 reads with -m 8, default scores, retire_shift 4 and the launch log on, three ways — retirement on,
`no_retire` 1, the CPU oracle (M8_ABS): equal texts read by read, mem:run_rows > 0, and the instantiation of the case's packed width ran
in both sweeps.  `wide70` (70 paths: kWide steps over continuation entries) and `len1200` (32 columns per lane) keep the variants that
are closest to the register limit under test with the rebuilt source around them: bytes against the oracle."""
import numpy as np
import pytest

OPTS = ("retire_shift", "no_retire", "launch_log")


def bounds_graph(reps=1, src=4, q=(2, 2, 2, 2), snk=4, seed=77):
    """-> SynthGraph: the block series of the module docstring `reps` times between a source of `src` and a sink of `snk` rows."""
    from recgraph_amd import synth
    rng = np.random.default_rng(seed)
    segments, links, paths = [], [], [[] for _ in range(6)]

    def seg(n, with_n=False):
        s = synth._rand_seq(rng, n)
        if with_n:
            s = "".join("N" if k % 5 == 2 else c for k, c in enumerate(s))
        segments.append((len(segments) + 1, s))
        return len(segments)

    prev = seg(src)
    for p in paths:
        p.append(prev)
    pair1 = lambda n: [((1, 5), n), ((0,), 1), ((2,), 2), ((3,), 1), ((4,), 2)]
    pair2 = lambda n: [((2, 5), n), ((0,), 2), ((1,), 1), ((3,), 2), ((4,), 1)]
    series = [pair1(q[0]), pair2(q[1]),
              [((0,), -140), ((1, 2), -127), ((3, 4, 5), 63)],
              [((0, 1, 2, 3), 62), ((4,), 65), ((5,), 64)],
              [((0,), 1), ((1,), 2), ((2,), 3), ((3, 4, 5), 64)],
              pair1(q[2]), pair2(q[3])]
    for _ in range(reps):
        for groups in series:
            ids = {}
            for members, n in groups:
                s = seg(abs(n), with_n=n < 0)
                for k in members:
                    ids[k] = s
            sh = seg(3)
            for k in range(6):
                links += [(prev, ids[k]), (ids[k], sh)]
                paths[k] += [ids[k], sh]
            prev = sh
    last = seg(snk)
    for p in paths:
        links.append((prev, last))
        p.append(last)
    return synth.SynthGraph(segments, links, paths)


def _subst(rng, s, rate=0.01):
    s = list(s)
    for i in range(len(s)):
        if s[i] == "N" or rng.random() < rate:
            s[i] = "ACGT"[int(rng.integers(0, 4))]
    return "".join(s)


def bounds_reads(g, n, seed):
    """Path 5 with 1 % substitutions; every second read a mosaic: path 5 up to a uniform point, another path from there on."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n):
        a = g.path_sequence(5)
        if i % 2:
            b, frac = g.path_sequence(int(rng.integers(0, 5))), rng.random()
            a = a[:int(frac * len(a))] + b[int(frac * len(b)):]
        reads.append(_subst(rng, a))
    return reads


def _fields(text):
    recs = text.split(";")[2]
    out = []
    for r in recs.split(","):
        x = int(r.split(":")[0], 16)
        out.append(((x >> 23) & 7, (x >> 26) & 63))
    return out


def table_bounds(f):
    """Which of the five bounds a split step table [(flags, run field)] holds."""
    n = len(f)
    run = lambda t: (f[t][0] & 4) and f[t][1] > 0
    return {
        # a record with a capped field whose counted stretch of 63 rows is followed by another inner row of the run
        "cap": any(run(t) and f[t][1] == 63 and t + 63 < n and f[t + 63][0] == 7 and f[t + 63][1] > 0 and
                   all(f[u][0] == 7 for u in range(t + 1, t + 63)) for t in range(n)),
        "rows on both sides of a block boundary": any(t % 64 == 63 and run(t) and f[t][1] > 1 for t in range(n)),
        "last row is record 63 of a block": any(t % 64 == 63 and run(t) and f[t][1] == 1 for t in range(n)),
        "tail is record 0 of a block": any(t % 64 == 0 and (f[t][0] & 4) and f[t][1] == 0 for t in range(n)),
        "run ends on the last record": bool(run(n - 1) and f[n - 1][1] == 1),
    }


def _tables(g):
    from recgraph_amd import api
    gg = api.Graph.from_gfa_text(g.gfa())
    return [_fields(gg.dump(which)) for which in (32, 34)]


# (src, q, snk) of the two graphs: the first lengths, tried in ascending order, at which the split tables of both directions hold all
# five bounds (672 records a direction at one series of blocks, 2660 at four)
C4_LENGTHS = dict(src=4, q=(1, 1, 1, 2), snk=4)
C16_LENGTHS = dict(src=4, q=(1, 1, 1, 1), snk=4)

# name -> (graph, reads, packed width, kWide)
CASES = {
    "c4": (lambda: bounds_graph(1, **C4_LENGTHS), lambda g: bounds_reads(g, 48, 771), 4, False),
    "c16": (lambda: bounds_graph(4, **C16_LENGTHS), lambda g: bounds_reads(g, 12, 772), 16, False),
}


def _keep_cases():
    from recgraph_amd import synth
    return {
        "wide70": (lambda: synth.random_dag_graph(80, 70, seed=16),
                   lambda g: [_subst(np.random.default_rng(160 + i), g.path_sequence((7 * i) % 70)) for i in range(16)], None, True),
        "len1200": (lambda: synth.haplotype_graph(2600, 8, path_len=1200, seed=1208),
                    lambda g: synth.haplotype_reads(g, 8, length=1200, seed=12080, mosaic_frac=0.5), 32, False),
    }


@pytest.mark.parametrize("name", ["c4", "c16"])
def test_inputs_put_a_bound_everywhere(name):
    g = CASES[name][0]()
    lens = sorted({len(s) for _, s in g.segments})
    assert set((1, 2, 3, 62, 63, 64, 65, 127, 140)) <= set(lens), lens
    assert sum("N" in s for _, s in g.segments) == 2 * (1 if name == "c4" else 4)
    reads = CASES[name][1](g)
    lo, hi = (200, 250) if name == "c4" else (800, 1000)
    assert all(lo <= len(r) <= hi for r in reads), sorted(len(r) for r in reads)
    for direction, f in zip(("forward", "reverse"), _tables(g)):
        missing = [k for k, v in table_bounds(f).items() if not v]
        assert not missing, (name, direction, missing)


def _gpu(gfa, reads, options):
    """(texts, silent rows, run rows, {instantiation: launches}) of one batch under `options` and the launch log (restored afterwards)."""
    from recgraph_amd import api
    lib = api._lib.load()
    before = {k: lib.rg_get_option(k.encode()) for k in OPTS}
    try:
        for k, v in dict(options, launch_log=1).items():
            api.set_option(k, v)
        gg = api.Graph.from_gfa_text(gfa)
        b = api.Batch(gg, reads, api.make_params(api.MODE_RECOMBINATION))
        b.run()
        b.fetch()
        texts = [b.gaf_text(i, "r%d" % i, i + 1) for i in range(len(reads))]
        stats = b.kernel_stats()
    finally:
        for k, v in before.items():
            api.set_option(k, v)
    insts = {k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")}
    return texts, int(stats["mem:silent_rows"][0]), int(stats["mem:run_rows"][0]), insts


def _oracle_texts(oracle, g, reads, threads=8):
    from concurrent.futures import ThreadPoolExecutor
    og = oracle.Graph.from_gfa_text(g.gfa())
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(lambda i: og.align(oracle.M8_ABS, reads[i], name="r%d" % i, idx=i + 1)[0], range(len(reads))))


def _ran_in_both_sweeps(insts, C, wide):
    names = [k for k, v in insts.items() if k.startswith("rg::k_sweep16<") and k.endswith(", 0, true, %s, false>" % ("true" if wide else "false"))
             and (C is None or k.startswith("rg::k_sweep16<%d," % C)) and v >= 2]
    return bool(names)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c4", "c16"])
def test_counted_run_rows_change_no_byte(oracle, name):
    mk_graph, mk_reads, C, wide = CASES[name]
    g = mk_graph()
    reads = mk_reads(g)
    assert len(reads) <= 64
    exp = _oracle_texts(oracle, g, reads)
    on, silent, runs, insts = _gpu(g.gfa(), reads, {"retire_shift": 4})
    off, silent0, runs0, insts0 = _gpu(g.gfa(), reads, {"retire_shift": 4, "no_retire": 1})
    print("%s: %d reads, silent rows %d of %d run rows with retirement, %d of %d without" % (name, len(reads), silent, runs, silent0, runs0))
    assert _ran_in_both_sweeps(insts, C, wide) and _ran_in_both_sweeps(insts0, C, wide), (name, sorted(insts), sorted(insts0))
    for i in range(len(reads)):
        assert on[i] == exp[i], (name, i, on[i][-300:], exp[i][-300:])
        assert off[i] == exp[i], (name, i, off[i][-300:], exp[i][-300:])
    assert runs > 0 and runs0 > 0, (name, runs, runs0)
    assert 0 < silent <= runs and silent0 == 0, (name, silent, runs, silent0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wide70", "len1200"])
def test_variants_next_to_the_counted_loop_against_the_oracle(oracle, name):
    mk_graph, mk_reads, C, wide = _keep_cases()[name]
    g = mk_graph()
    reads = mk_reads(g)
    assert len(reads) <= 64
    exp = _oracle_texts(oracle, g, reads)
    on, _, runs, insts = _gpu(g.gfa(), reads, {"retire_shift": 4})
    print("%s: %d reads, %d run rows" % (name, len(reads), runs))
    assert _ran_in_both_sweeps(insts, C, wide), (name, sorted(insts))
    for i in range(len(reads)):
        assert on[i] == exp[i], (name, i, on[i][-300:], exp[i][-300:])
