"""GPU: silent members left out of the key work of k_sweep16's narrow record variants (rg_sweep16.hip, KEY WORK THAT NO RECORD
USES: pass (1) of a gather run, the folds of general-path records, the tails of silent runs) change no byte, and the counters
"mem:key_folds" / "mem:key_rows" / "mem:key_rows_hit" / "mem:key_folds_saved" say what ran.

Every case aligns a few reads with -m 8, default scores, at retire_shift 4 (path retirement evaluates every 16 step records, so it
is live on graphs of a few hundred rows) three ways: under the case's switches, the same with `no_retire` 1 (no path is ever proven
hopeless: the silent set stays empty), and the CPU oracle (M8_ABS).  All three texts are equal read by read.

Graphs: random walks through segments in id order (synth.random_dag_graph: segments that several segments lead into, so rows have
several groups — tails in the split tables, general-path records with `no_split`), 9 - 12 paths, and one 32-path haplotype graph of
~1200 rows whose 700-base reads are mosaics (gather runs on the rows every path visits; the 16-column variant needs reads past 511 bases).  Packed widths 4, 8 and 16 by read length.

  gather   a hand-built graph of six paths whose reads are exact copies of path 5.  Blocks of private alleles (every other path
           diverges from the read by a whole allele per block) alternate with shared segments of eight rows, which all six paths run
           through as one group: more members than a register run takes, so the inner rows of every shared segment are a gather run.
           Paths 0 - 4 are hopeless after a few blocks but stay needed (path 0 leads the shared groups, and each of 1 - 4 shares an
           allele with path 5 in every fourth block): the gather runs then have only silent needed members besides the read's own path.
           (Pass (1) then iterates one member, path 5, over the alpha's base.  It cannot be left with NO member here or anywhere a
           group holds every path: a hopeless path stays needed only while it leads a path that is not hopeless, and that path is a
           member of the same group.  An empty iterator is the loop's ordinary exit — `kn = -1`, the table holds the alpha alone —
           which every pass (1) reaches behind its last member.)

  tails    a hand-built graph of six paths whose reads follow path 4 (1 % substitutions).  In its A blocks path 4 has an allele of its
           own, paths 0 - 3 share the next one and path 5 has the last; in the blocks between them path 1, 2 or 3 shares an allele
           with path 4 (so paths 1 - 3 stay needed once hopeless, and path 0 leads them) and the others have short private ones.  The
           first row of the shared segment behind an A block has three groups, in table order {4}, {0, 1, 2, 3}, {5}: the register
           run of {0 - 3} through its allele is silent, and its tail finds the keys of {4} parked and the group of {5} still to
           come — the tail that folds nothing.

Counters, not timings.  With retirement: members are left out (`key_folds_saved` > 0, fewer folds than without retirement), rows
close, some of them write a record and not all of them.  Without retirement the silent set is empty and nothing
is left out.  `no_spec` (the provable bound, on the mosaic reads of the 32-path graph: the best single path lies far below a mosaic's
optimum, so the bound lets nearly every row emit): more than half of the closing rows write a record.  Each of the three places has cases
that assert its own counter: gather pass (1) (`gather`, `c8`, `c16`), the general path (`no_split`, `c8`, `c16`), the tails of
silent runs (`tails`).
(`key_folds + key_folds_saved` of a run with retirement is NOT the `key_folds` of the run without: records all of whose members are
retired are skipped whole, and the pass-(1) members of a gather run are counted as left out but never as folds.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = ("retire_shift", "no_retire", "spec_margin", "no_spec", "no_split", "no_pick2", "launch_log")
KEYS = ("mem:key_folds", "mem:key_rows", "mem:key_rows_hit", "mem:key_folds_saved", "mem:key_saved_gather", "mem:key_saved_general",
        "mem:key_saved_tail")
# name -> (graph recipe, reads, read length cap, packed width, switches)
GRAPHS = {
    "dag4": (("dag", dict(nseg=120, P=9, seed=202, max_jump=3)), 16, 250, 4),
    "dag8": (("dag", dict(nseg=200, P=12, seed=207, max_jump=3, max_seg=6)), 12, 500, 8),
    "hap16": (("hap", dict(seed=3216)), 12, 0, 16),
    "dag4n": (("dagn", dict(nseg=120, P=9, seed=202, max_jump=3)), 16, 250, 4),
    "gather": (("gather", dict(seed=66)), 12, 0, 4),
    "tails": (("tails", dict(seed=57)), 16, 0, 8),
}
CASES = {
    "c4": ("dag4", {}), "c8": ("dag8", {}), "c16": ("hap16", {}),
    "no_split": ("dag4", {"no_split": 1}), "no_spec": ("hap16", {"no_spec": 1}), "spec_margin0": ("dag4", {"spec_margin": 0}),
    "no_retire2": ("dag4", {"no_retire": 2}), "no_retire3": ("dag4", {"no_retire": 3}), "nbases": ("dag4n", {}),
    "gather": ("gather", {}),
    "tails": ("tails", {"no_pick2": 1}),
}
# the place whose own counter the case asserts
PLACE = {"gather": ("mem:key_saved_gather",), "no_split": ("mem:key_saved_general",), "c8": ("mem:key_saved_gather", "mem:key_saved_general"),
         "c16": ("mem:key_saved_gather", "mem:key_saved_general"), "tails": ("mem:key_saved_tail",)}
_CACHE = {}


def gather_graph(seed, blocks=12, shared=8, along=10):
    """Six paths; block b: paths 0 - 4 have private alleles of `along` rows, except that path m = 1 + b % 4 shares its allele with path 5
    and that path 0 and path k = 1 + (b + 1) % 4 merge into one segment for the second half of theirs (a row with two groups that the
    read's path does not visit); a shared segment of `shared` rows behind every block."""
    from recgraph_amd import synth
    rng = np.random.default_rng(seed)
    segments, links, paths = [], [], [[] for _ in range(6)]

    def seg(n):
        segments.append((len(segments) + 1, synth._rand_seq(rng, n)))
        return len(segments)

    prev = seg(shared)
    for p in paths:
        p.append(prev)
    for b in range(blocks):
        m = 1 + b % 4
        k2 = 1 + (b + 1) % 4
        walk = {k: [seg(along)] for k in range(1, 5) if k not in (m, k2)}
        walk[m] = walk[5] = [seg(along)]
        walk[0], walk[k2] = [seg(along // 2)], [seg(along // 2)]
        half = seg(along - along // 2)
        walk[0].append(half)
        walk[k2].append(half)
        sh = seg(shared)
        for k in range(6):
            chain = [prev] + walk[k] + [sh]
            links += list(zip(chain, chain[1:]))
            paths[k] += walk[k] + [sh]
        prev = sh
    return synth.SynthGraph(segments, sorted(set(links)), paths)


def tails_graph(seed, blocks=24, along=12, short=2):
    """Six paths.  Block 2t is an A block — alleles {4}, {0, 1, 2, 3}, {5} in that id order, `along` rows each —, block 2t + 1 pairs
    path 1 + t % 3 with path 4 in one allele of `along` rows and gives the other four paths private alleles of `short` rows (paths 0
    and 5 then share `short` more rows: closing rows no read comes near); a shared
    segment of three rows behind every block."""
    from recgraph_amd import synth
    rng = np.random.default_rng(seed)
    segments, links, paths = [], [], [[] for _ in range(6)]

    def seg(n):
        segments.append((len(segments) + 1, synth._rand_seq(rng, n)))
        return len(segments)

    prev = seg(8)
    for p in paths:
        p.append(prev)
    for b in range(blocks):
        if b % 2 == 0:
            groups = [((4,), along), ((0, 1, 2, 3), along), ((5,), along)]
        else:
            m = 1 + (b // 2) % 3
            groups = [((k,), short) for k in (0, 1, 2, 3, 5) if k != m] + [((m, 4), along)]
        walk = {}
        for members, n in groups:
            s = seg(n)
            for k in members:
                walk[k] = [s]
        if b % 2 == 1:
            # (paths 0 and 5 merge behind their private alleles: a row with two groups that the reads' path does not visit)
            x = seg(short)
            walk[0].append(x)
            walk[5].append(x)
        sh = seg(3)
        for k in range(6):
            chain = [prev] + walk[k] + [sh]
            links += list(zip(chain, chain[1:]))
            paths[k] += walk[k] + [sh]
        prev = sh
    snk = seg(8)
    for p in paths:
        p.append(snk)
    links += [(prev, snk)]
    return synth.SynthGraph(segments, sorted(set(links)), paths)


def build(gname):
    from recgraph_amd import synth
    if gname in _CACHE:
        return _CACHE[gname]
    (kind, args), nreads, cap, width = GRAPHS[gname]
    if kind == "tails":
        g = tails_graph(**args)
        rng = np.random.default_rng(args["seed"] * 10)
        src = g.path_sequence(4)
        reads = ["".join("ACGT"[("ACGT".index(c) + int(rng.integers(1, 4))) % 4] if rng.random() < 0.01 else c for c in src) for _ in range(nreads)]
    elif kind == "gather":
        g = gather_graph(**args)
        reads = [g.path_sequence(5)] * nreads
    elif kind == "hap":
        g = synth.haplotype_graph(1000, 32, path_len=700, seed=args["seed"])
        reads = synth.haplotype_reads(g, nreads, length=700, seed=args["seed"] + 1, mosaic_frac=0.75)
    else:
        kw = {k: v for k, v in args.items() if k not in ("nseg", "P")}
        g = synth.random_dag_graph(args["nseg"], args["P"], **kw)
        if kind == "dagn":
            segs = [(i, "".join("N" if k % 5 == 2 else c for k, c in enumerate(s))) for i, s in g.segments]
            g = synth.SynthGraph(segs, g.links, g.paths)
        plen = min(len(g.path_sequence(k)) for k in range(args["P"]))
        length = min(plen, cap)
        assert length > (64 * width) // 2, (gname, plen)      # the reads select the packed width of the case
        # the last read is an exact copy of one path: beside it the other paths diverge, and a gather run of its rows has only silent
        # needed members besides the read's own path once retirement has looked at them
        reads = synth.haplotype_reads(g, nreads - 1, length=length, seed=args["seed"] + 1, mosaic_frac=0.6) + [g.path_sequence(args["P"] - 1)[:length]]
    _CACHE[gname] = (g, reads)
    return _CACHE[gname]


def oracle_texts(oracle, gname):
    """Computed once per graph and read set, never changed."""
    key = ("oracle", gname)
    if key not in _CACHE:
        g, reads = build(gname)
        og = oracle.Graph.from_gfa_text(g.gfa())
        _CACHE[key] = [og.align(oracle.M8_ABS, rd, name="r%d" % i, idx=i + 1)[0] for i, rd in enumerate(reads)]
    return _CACHE[key]


def _gpu(gfa, reads, options):
    """(texts, {counter: value}, {instantiation: launches}) of one batch under `options` and the launch log (restored afterwards)."""
    from recgraph_amd import api
    lib = api._lib.load()
    before = {k: lib.rg_get_option(k.encode()) for k in OPTS}
    try:
        for k, v in dict(options, launch_log=1).items():
            api.set_option(k, v)
        b = api.Batch(api.Graph.from_gfa_text(gfa), reads, api.make_params(api.MODE_RECOMBINATION))
        b.run()
        b.fetch()
        texts = [b.gaf_text(i, "r%d" % i, i + 1) for i in range(len(reads))]
        stats = b.kernel_stats()
    finally:
        for k, v in before.items():
            api.set_option(k, v)
    assert all(k in stats for k in KEYS), sorted(stats)
    return texts, {k: int(stats[k][0]) for k in KEYS}, {k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_silent_members_left_out_change_no_byte(oracle, name):
    gname, switches = CASES[name]
    g, reads = build(gname)
    exp = oracle_texts(oracle, gname)
    opts = dict(switches, retire_shift=4)
    on, cnt, insts = _gpu(g.gfa(), reads, opts)
    off, cnt0, insts0 = _gpu(g.gfa(), reads, dict(opts, no_retire=1))
    print(name, "with retirement", cnt, "without", cnt0)
    variant = "rg::k_sweep16<%d, 0, true, false, false>" % GRAPHS[gname][3]
    assert insts.get(variant, 0) >= 2 and insts0.get(variant, 0) >= 2, (name, variant, sorted(insts))
    for i in range(len(reads)):
        assert on[i] == exp[i], (name, i, on[i][-300:], exp[i][-300:])
        assert on[i] == off[i], (name, i, on[i][-300:], off[i][-300:])
    for c in (cnt, cnt0):
        assert c["mem:key_rows"] > 0 and c["mem:key_folds"] > 0, (name, c)
        assert c["mem:key_rows_hit"] <= c["mem:key_rows"], (name, c)
    # with retirement: rows write records, not every closing row does, and members are left out
    assert 0 < cnt["mem:key_rows_hit"] < cnt["mem:key_rows"], (name, cnt)
    assert cnt["mem:key_folds_saved"] > 0 and cnt["mem:key_folds"] < cnt0["mem:key_folds"], (name, cnt, cnt0)
    for place in PLACE.get(name, ()):
        assert cnt[place] > 0, (name, place, cnt)
    if name == "no_spec":
        assert 2 * cnt["mem:key_rows_hit"] > cnt["mem:key_rows"], (name, cnt)
    # a fold is left out only for a member of the silent set, and without retirement the set is empty
    assert cnt0["mem:key_folds_saved"] == 0, (name, cnt0)
