"""GPU: the lean row loop of k_sweep16 for SILENT register runs (runs whose computed members are all proven hopeless,
with no direction word asked for) changes no byte, and the counters "mem:silent_rows" / "mem:run_rows" say that it ran.

Every case aligns at most 64 reads with -m 8, default scores, at retire_shift 4 (path retirement evaluates every 16 step records, so
it is live on graphs of a few hundred rows) three ways: retirement on, `no_retire` 1, and the CPU oracle (M8_ABS).  All three texts
are equal read by read; silent_rows > 0 with retirement, == 0 without it, and never above run_rows.

  c4 / c8 / c16   one haplotype graph per packed width of the variant: reads of 200 / 450 / 900 bases, half of them mosaics of two
                  paths (two picks, both sweeps live); 8 - 16 paths, 600 - 2000 rows: step tables of many 64-record blocks, allele
                  segments of up to 16 rows (runs cross block boundaries)
  nbases          the c4 graph with every fifth base of its allele segments an N: the 'N' profile row inside silent runs
  second-pass     the c4 batch at spec_margin -10^6: every read fails its bound and is aligned again.  The later passes store every
                  direction word, so they count no silent row: the same batch with `no_dsel` 1 — the first pass then stores every
                  word too, the later passes are the same launches — counts none at all.  (Both passes add into one statistic, so the
                  second pass's own count cannot be read apart.  "silent_rows > 0 with retirement" is deliberately NOT asserted for
                  this batch: on a bound no path can reach the first pass retires every path at its first evaluation and has next
                  to no run rows left, silent or not — measured 0.)
  members         a hand-built graph of five paths whose reads follow path 4.  In its A blocks paths 0 - 3 share one allele; in the
                  blocks between them path 1, 2 or 3 shares an allele with path 4 and the others have short alleles of their own.
                  Paths 1 - 3 are hopeless but lead path 4 further down, path 0 leads them: the A alleles run silent with up to
                  four members.  A one-member silent row can only be a row of a private allele, so more silent rows than
                  2 sweeps x reads x private-allele rows proves runs with several members among them.  Why only there: shared
                  segments are rows every path visits and the alleles with path 4 hold the picked path (never silent); an A allele
                  cannot run with ONE computed member, because that member would be its alpha, path 0, and path 0 leads nothing
                  but the A alleles — once hopeless it is kept only while one of paths 1 - 3 is still needed, and that path is
                  then a computed member of this A allele too (the closure of DESIGN 4.7; either sweep: the groups are the same).

The launch log is on in every run: each case asserts that the instantiation of its packed width, k_sweep16<C, 0, true, false, false>,
ran in both sweeps.

Seeds: chosen on the CPU so that the oracle gives a real alignment (a path of segments and a CIGAR, not an empty record) for every read of every
case; the test asserts it for at least 90 % of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = ("retire_shift", "no_retire", "spec_margin", "no_dsel", "no_pick2", "launch_log")
WIDTH = {"c4": 4, "c8": 8, "c16": 16, "nbases": 4, "second-pass": 4, "members": 8}      # columns per lane: 64 C >= read length + 1
_CACHE = {}


def _with_n(g, every=5):
    """The same graph with every `every`-th base of its allele segments (the segments not every path walks) an N."""
    from recgraph_amd import synth
    on_all = set(g.paths[0])
    for p in g.paths[1:]:
        on_all &= set(p)
    segs = [(i, s if i in on_all else "".join("N" if k % every == 2 else c for k, c in enumerate(s))) for i, s in g.segments]
    return synth.SynthGraph(segs, g.links, g.paths)


def members_graph(seed, blocks=24, along=12, short=2):
    """-> (SynthGraph, rows of the private alleles).  Block 2t is an A block — alleles {0, 1, 2, 3} and {4}, `along` rows each —,
    block 2t + 1 pairs path 1 + t % 3 with path 4 in one allele of `along` rows and gives the other three paths private alleles of
    `short` rows; a shared segment of three rows behind every block."""
    from recgraph_amd import synth
    rng = np.random.default_rng(seed)
    segments, links, paths = [], [], [[] for _ in range(5)]
    private_rows = 0

    def seg(n):
        segments.append((len(segments) + 1, synth._rand_seq(rng, n)))
        return len(segments)

    prev = seg(8)
    for p in paths:
        p.append(prev)
    for b in range(blocks):
        if b % 2 == 0:
            groups = [((0, 1, 2, 3), along), ((4,), along)]
        else:
            m = 1 + (b // 2) % 3
            groups = [((k,), short) for k in (0, 1, 2, 3) if k != m] + [((m, 4), along)]
            private_rows += 3 * short
        ids = {}
        for members, n in groups:
            s = seg(n)
            for k in members:
                ids[k] = s
        sh = seg(3)
        for k in range(5):
            links += [(prev, ids[k]), (ids[k], sh)]
            paths[k] += [ids[k], sh]
        prev = sh
    snk = seg(8)
    for p in paths:
        links.append((prev, snk))
        p.append(snk)
    return synth.SynthGraph(segments, links, paths), private_rows


def _subst(rng, s, rate=0.01):
    s = list(s)
    for i in range(len(s)):
        if rng.random() < rate:
            s[i] = "ACGT"[("ACGT".index(s[i]) + int(rng.integers(1, 4))) % 4]
    return "".join(s)


# name -> (graph recipe, reads, read length, read seed, option switches of the run with retirement)
CASES = {
    "c4": (("haplotype", dict(target_rows=620, n_paths=8, path_len=200, seed=411)), 32, 200, 4110, {}),
    "c8": (("haplotype", dict(target_rows=1100, n_paths=12, path_len=450, seed=812)), 24, 450, 8120, {}),
    "c16": (("haplotype", dict(target_rows=2000, n_paths=16, path_len=900, seed=1616)), 12, 900, 16160, {}),
    "nbases": (("haplotype_n", dict(target_rows=620, n_paths=8, path_len=200, seed=411)), 32, 200, 4111, {}),
    "second-pass": (("haplotype", dict(target_rows=620, n_paths=8, path_len=200, seed=411)), 32, 200, 4110, {"spec_margin": -1000000}),
    "members": (("members", dict(seed=57)), 16, 0, 570, {"no_pick2": 1}),
}


def build(name):
    """(SynthGraph, reads, private-allele rows or None) of a case."""
    from recgraph_amd import synth
    (kind, args), nreads, length, rseed, _ = CASES[name]
    private = None
    if kind == "members":
        g, private = members_graph(**args)
        rng = np.random.default_rng(rseed)
        reads = [_subst(rng, g.path_sequence(4)) for _ in range(nreads)]
    else:
        g = synth.haplotype_graph(**args)
        if kind == "haplotype_n":
            g = _with_n(g)
        reads = synth.haplotype_reads(g, nreads, length=length, seed=rseed, mosaic_frac=0.5)
    return g, reads, private


def is_real_alignment(text):
    """The GAF line names a path of segments and carries a CIGAR (an empty record has neither)."""
    line = [ln for ln in text.splitlines() if "\t" in ln]
    if not line:
        return False
    f = line[-1].split("\t")
    return len(f) > 12 and f[5].startswith(">") and f[12][:1].isdigit() and int(f[3]) > int(f[2])


def oracle_texts(oracle, name, threads=8):
    """Computed once per graph and read set (c4 and second-pass share theirs), never changed."""
    from concurrent.futures import ThreadPoolExecutor
    key = ("oracle",) + tuple(str(x) for x in CASES[name][:4])
    if key not in _CACHE:
        g, reads, _ = build(name)
        og = oracle.Graph.from_gfa_text(g.gfa())
        with ThreadPoolExecutor(threads) as ex:
            _CACHE[key] = list(ex.map(lambda i: og.align(oracle.M8_ABS, reads[i], name="r%d" % i, idx=i + 1)[0], range(len(reads))))
    return _CACHE[key]


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
    assert "mem:silent_rows" in stats and "mem:run_rows" in stats, sorted(stats)
    insts = {k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")}
    return texts, int(stats["mem:silent_rows"][0]), int(stats["mem:run_rows"][0]), insts


def _run(oracle, name, want_silent=True):
    if name in _CACHE:
        return _CACHE[name]
    g, reads, private = build(name)
    assert len(reads) <= 64
    exp = oracle_texts(oracle, name)
    assert sum(is_real_alignment(t) for t in exp) * 10 >= 9 * len(exp), name
    gfa = g.gfa()
    opts = dict(CASES[name][4], retire_shift=4)
    on, silent, runs, insts = _gpu(gfa, reads, opts)
    off, silent0, runs0, insts0 = _gpu(gfa, reads, dict(opts, no_retire=1))
    variant = "rg::k_sweep16<%d, 0, true, false, false>" % WIDTH[name]
    assert insts.get(variant, 0) >= 2 and insts0.get(variant, 0) >= 2, (name, variant, sorted(insts))
    print("%s: %d reads, silent rows %d of %d run rows with retirement, %d of %d without" % (name, len(reads), silent, runs, silent0, runs0))
    for i in range(len(reads)):
        assert on[i] == exp[i], (name, i, on[i][-300:], exp[i][-300:])
        assert on[i] == off[i], (name, i, on[i][-300:], off[i][-300:])
    assert silent <= runs and (silent > 0 or not want_silent), (name, silent, runs)
    assert silent0 == 0 and runs0 > 0, (name, silent0, runs0)
    _CACHE[name] = (g, reads, private, silent, runs)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["c4", "c8", "c16", "nbases"])
def test_silent_runs_change_no_byte(oracle, name):
    g, reads, _, silent, runs = _run(oracle, name)
    if name == "nbases":
        assert any("N" in s for _, s in g.segments)


def test_second_pass_counts_no_silent_row(oracle):
    # (the first pass, on a bound no path can reach, retires every path at its first evaluation: it has next to no runs, silent or not)
    g, reads, _, silent, runs = _run(oracle, "second-pass", want_silent=False)
    # every word stored in every pass: no run is silent, and the bytes stay
    texts, silent_all, runs_all, _ = _gpu(g.gfa(), reads, dict(CASES["second-pass"][4], retire_shift=4, no_dsel=1))
    assert texts == oracle_texts(oracle, "second-pass")
    assert silent_all == 0 and runs_all > 0, (silent_all, runs_all)


def test_silent_runs_with_several_members(oracle):
    g, reads, private, silent, runs = _run(oracle, "members")
    assert silent > 2 * len(reads) * private, (silent, len(reads), private)
