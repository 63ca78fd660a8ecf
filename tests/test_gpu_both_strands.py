"""GPU: RG_AMB_BOTH_STRANDS — both strands inside a pathwise batch (modes 4, 5, 8, 9; include/recgraph_hip.h).

The reference has no such mode (its `-s true` stops at modes 0-3), so the expected text is BUILT from the oracle by the
rule the header states: fwd = oracle(read); if its printed score is < 0, rev = oracle(reverse complement); if rev's
printed score is strictly greater, the expected record is rev's with the strand column '-', else fwd's."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def _rc(s):
    return "".join(COMP[c] for c in reversed(s))


def _threads(cap=32):
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(cap, n))


def _printed_score(text):
    return float(re.search(r"score: (-?[0-9.]+)", text).group(1))


def _minus(text):
    f = text.split("\t")
    assert f[4] == "+"
    f[4] = "-"
    return "\t".join(f)


def _omode(oracle, m):
    return {4: oracle.M4_ABS, 5: oracle.M5_ABS, 8: oracle.M8_ABS, 9: oracle.M9_ABS}[m]


def _amode(m):
    from recgraph_amd import api
    return {4: api.MODE_PATHWISE, 5: api.MODE_PATHWISE_SEMI, 8: api.MODE_RECOMBINATION, 9: api.MODE_RECOMBINATION_SEMI}[m]


def expected_both_strands(oracle, og, m, reads, prefix="q"):
    """Per read: (expected text, branch, reverse record has a recombination), from the oracle alone.  branch: 'plain' (not
    retried), 'kept' (retried, forward kept), 'rev' (reverse wins).  Read i is called prefix + str(i)."""
    om = _omode(oracle, m)
    _, _, fwd = og.bench_text(om, reads, nthreads=_threads(), name_prefix=prefix)
    retry = [i for i, t in enumerate(fwd) if _printed_score(t.decode()) < 0]
    out = [(t.decode(), "plain", False) for t in fwd]
    if retry:
        # (bench_text names by position: the reverse complements keep their reads' places, the others are one base long)
        sub = [_rc(reads[i]) if i in set(retry) else "A" for i in range(len(reads))]
        _, _, rev = og.bench_text(om, sub, nthreads=_threads(), name_prefix=prefix)
        for i in retry:
            f, r = fwd[i].decode(), rev[i].decode()
            if _printed_score(r) > _printed_score(f):
                out[i] = (_minus(r), "rev", "recombination path" in r)
            else:
                out[i] = (f, "kept", False)
    return out


def _mutate(rng, s, rate):
    s = list(s)
    for k in range(len(s)):
        if rng.random() < rate:
            s[k] = "ACGT"[int(rng.integers(0, 4))]
    return "".join(s)


def _mixed_reads(path_seqs, n_each, seed, semi):
    """Reads cut from a path, reverse complements of such reads, mosaics of two paths on both strands, heavily mutated
    reads and random reads."""
    rng = np.random.default_rng(seed)
    P = len(path_seqs)

    def cut(s):
        if not semi:
            return s
        a = int(rng.integers(0, len(s) // 4))
        return s[a:a + len(s) * 3 // 4]

    def walk():
        return cut(_mutate(rng, path_seqs[int(rng.integers(0, P))], 0.01))

    def mosaic():
        a, b = path_seqs[int(rng.integers(0, P))], path_seqs[int(rng.integers(0, P))]
        fr = 0.25 + 0.5 * rng.random()
        return cut(_mutate(rng, a[:int(fr * len(a))] + b[int(fr * len(b)):], 0.01))
    n = len(path_seqs[0])
    rd = [walk() for _ in range(n_each)] + [_rc(walk()) for _ in range(n_each)]
    rd += [mosaic() for _ in range(n_each)] + [_rc(mosaic()) for _ in range(n_each)]
    rd += [_mutate(rng, walk(), 0.75) for _ in range(n_each)]
    rd += ["".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=int(rng.integers(n // 2, n)))) for _ in range(n_each + 4)]
    order = rng.permutation(len(rd))
    return [rd[int(k)] for k in order]


def _example_paths(gfa):
    seg, paths = {}, []
    for ln in gfa.splitlines():
        f = ln.split("\t")
        if f[0] == "S":
            seg[f[1]] = f[2]
        elif f[0] == "P":
            paths.append("".join(seg[s[:-1]] for s in f[2].split(",")))
    return paths


CASES = {
    # name: (graph, reads per kind, seed)
    "example": (None, 7, 101),
    "wide_70_paths": ((1500, 70, 300, 77), 7, 202),            # P > 64: several 64-path pages
    "striped_2150": ((5400, 4, 2150, 78), 6, 303),             # reads of 2 100+ bases: the column-striped kernels
}


def _case(name, m, example_gfa):
    from recgraph_amd import synth
    spec, n_each, seed = CASES[name]
    semi = m in (5, 9)
    if spec is None:
        gfa = example_gfa
        paths = _example_paths(gfa)
    else:
        sg = synth.haplotype_graph(spec[0], spec[1], path_len=spec[2], seed=spec[3])
        gfa = sg.gfa()
        paths = [sg.path_sequence(k) for k in range(spec[1])]
    return gfa, _mixed_reads(paths, n_each, seed + m, semi)


def check_not_vacuous(m, exp):
    """>= 5 reads in each of the three branches, and for -m 8 / 9 a reverse winner of either GAF shape."""
    n = {b: sum(1 for e in exp if e[1] == b) for b in ("plain", "kept", "rev")}
    assert min(n.values()) >= 5, (m, n)
    if m in (8, 9):
        shapes = {e[2] for e in exp if e[1] == "rev"}
        assert shapes == {True, False}, (m, shapes)
    return n


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("m", [4, 5, 8, 9])
def test_parity_by_construction(oracle, example_gfa, m, name):
    from recgraph_amd import api
    gfa, reads = _case(name, m, example_gfa)
    og = oracle.Graph.from_gfa_text(gfa)
    exp = expected_both_strands(oracle, og, m, reads)
    counts = check_not_vacuous(m, exp)          # from the oracle alone, before the GPU is touched
    print("both strands -m %d %s: %s" % (m, name, counts))
    want = [e[0] for e in exp]
    names = ["q%d" % i for i in range(len(reads))]
    g = api.Graph.from_gfa_text(gfa)
    mode = _amode(m)
    texts, status = api.align_batch(g, reads, names, mode=mode, both_strands=True)
    assert not any(status)
    bad = [(i, exp[i][1], texts[i][-200:], want[i][-200:]) for i in range(len(reads)) if texts[i] != want[i]]
    assert not bad, (len(bad), bad[:2])
    # the stream, with tiles that split the set (rg_stream_opts.amb_strand = 2), and every visible device behind one call
    stexts, sstatus = api.align_stream(g, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=11,
                                       both_strands=True)
    assert stexts == want and sstatus == status
    if name == "example":
        mtexts, _ = api.align_batch_multi(g, reads, names, mode=mode, device_ids=[0], both_strands=True)
        assert mtexts == want
    # the structured record and the accessors describe the chosen record
    b = api.Batch(g, reads, api.make_params(mode, amb=api.AMB_BOTH_STRANDS))
    b.run()
    b.fetch()
    assert b.format_all(names).decode() == "".join(want)
    for i in range(len(reads)):
        e = api.GAFStruct.from_line(want[i].rstrip("\n"))
        f = b.fields(i, names[i])
        assert (f.strand, f.path, f.path_length, f.path_start, f.path_end, f.query_length, f.query_end, f.comments) == \
               (e.strand, e.path, e.path_length, e.path_start, e.path_end, e.query_length, e.query_end, e.comments), i
        assert f.strand == ("-" if exp[i][1] == "rev" else "+")
        if "recombination path" not in want[i]:
            assert b.score(i) == int(_printed_score(want[i]))
    # nothing else moved: the bit clear gives the forward text, and amb_strand = 1 on a pathwise stream is still ignored
    _, _, fwd = og.bench_text(_omode(oracle, m), reads, nthreads=_threads(), name_prefix="q")
    plain, _ = api.align_batch(g, reads, names, mode=mode)
    assert plain == [t.decode() for t in fwd]
    ign, _ = api.align_stream(g, reads, names, mode=mode, device_ids=[0], tile_reads=11, amb_strand=True)
    assert ign == plain


def _sweeps(stats):
    return sum(v[1] for k, v in stats.items() if k.startswith("k_sweep"))


def test_edges_none_all_bad_base_and_tie(oracle):
    """A tile where no read qualifies (the second pass is skipped: one set of sweep launches), one where all do, reads the
    reference panics on, and an exact tie.

    In modes 4, 5, 8, 9 the only panic of the reference that depends on the READ is the score lookup of a character
    outside ACGTN (HashMap unwrap) — RG_READ_BAD_BASE here, `would_panic` in the oracle; every other panic of these modes
    comes from the graph or the parameters and refuses the whole batch.  So the reads "with a bad base" and "the reference
    would panic on" are the same reads in these modes; k_strand_gate tests both status bits with one mask."""
    from recgraph_amd import api, synth
    sg = synth.haplotype_graph(600, 6, path_len=200, seed=31)
    g = api.Graph.from_gfa_text(sg.gfa())
    og = oracle.Graph.from_gfa_text(sg.gfa())
    good = synth.haplotype_reads(sg, 24, 200, seed=5, mosaic_frac=0.5)
    for m in (4, 8):
        mode, om = _amode(m), _omode(oracle, m)
        assert all(_printed_score(og.align(om, r)[0]) >= 0 for r in good)
        runs = {}
        for key, reads, both in (("none_off", good, 0), ("none_on", good, 1), ("all_on", [_rc(r) for r in good], 1)):
            b = api.Batch(g, reads, api.make_params(mode, amb=api.AMB_BOTH_STRANDS if both else 0))
            b.run()
            b.fetch()
            runs[key] = (b.kernel_stats(), b.cell_updates, [b.gaf_text(i, "q%d" % i) for i in range(len(reads))])
        st_off, st_on, st_all = runs["none_off"][0], runs["none_on"][0], runs["all_on"][0]
        assert "k_strand_gate" not in st_off and st_on["k_strand_gate"][1] == 1 and st_on["k_revcomp"][1] == 1
        assert "k_strand_merge" not in st_on and _sweeps(st_on) == _sweeps(st_off)         # one sweep launch set, not two
        assert runs["none_on"][1] == runs["none_off"][1] and runs["none_on"][2] == runs["none_off"][2]
        assert st_all["k_strand_merge"][1] == 1 and _sweeps(st_all) >= 2 * _sweeps(st_off)
        exp = expected_both_strands(oracle, og, m, [_rc(r) for r in good])
        assert all(e[1] == "rev" for e in exp) and runs["all_on"][2] == [e[0] for e in exp]
        assert runs["all_on"][1] > runs["none_on"][1]            # the cell updates include the second pass
        # reads the reference panics on: not retried, status kept, no text; their neighbours are untouched
        reads = [good[0], good[1][:80] + "X" + good[1][81:], _rc(good[2]), "ACGT*" + good[3][5:], _rc(good[4])]
        for r in (reads[1], reads[3]):
            assert og.align(om, r)[2]
        texts, status = api.align_batch(g, reads, None, mode=mode, both_strands=True)
        assert [bool(s & api.READ_BAD_BASE) for s in status] == [False, True, False, True, False]
        assert texts[1] == "" and texts[3] == ""
        e = expected_both_strands(oracle, og, m, [reads[0], reads[2], reads[4]], prefix="x")
        for k, i in enumerate((0, 2, 4)):
            assert texts[i] == e[k][0].replace("x%d\t" % k, "read%d\t" % i, 1)
    # an exact tie keeps '+': a palindromic read (its reverse complement is itself) scores the same on both strands
    tie = "ACGT" * 30
    assert _rc(tie) == tie
    for m in (4, 5, 8, 9):
        om = _omode(oracle, m)
        f, r = og.align(om, tie, name="t")[0], og.align(om, _rc(tie), name="t")[0]
        assert _printed_score(f) < 0 and _printed_score(f) == _printed_score(r)          # it IS retried, and it ties
        texts, _ = api.align_batch(g, [tie, _rc(good[0])], ["t", "u"], mode=_amode(m), both_strands=True)
        assert texts[0] == f and "\t+\t" in texts[0] and "\t-\t" in texts[1]


def test_refusals():
    from recgraph_amd import api, synth
    sg = synth.haplotype_graph(300, 4, path_len=100, seed=3)
    g = api.Graph.from_gfa_text(sg.gfa())
    rd = synth.haplotype_reads(sg, 4, 100, seed=4)
    for mode, amb in ((api.MODE_GLOBAL_POA, 4), (api.MODE_GAP_POA, 4), (api.MODE_LOCAL_POA, 6), (api.MODE_RECOMBINATION, 5),
                      (api.MODE_PATHWISE, 6), (api.MODE_PATHWISE_SEMI, 1), (api.MODE_RECOMBINATION, 8)):
        with pytest.raises(api._lib.RecGraphError) as ex:
            api.Batch(g, rd, api.make_params(mode, amb=amb))
        assert ex.value.code == -1
        if mode in (api.MODE_GLOBAL_POA, api.MODE_GAP_POA):
            assert "amb_strand" in str(ex.value) and "-s true" in str(ex.value)
    # the handle is usable afterwards, and set_reads keeps the mode of the handle
    b = api.Batch(g, rd, api.make_params(api.MODE_RECOMBINATION, amb=api.AMB_BOTH_STRANDS))
    b.run()
    b.fetch()
    first = [b.gaf_text(i, "r%d" % i) for i in range(4)]
    b.set_reads([api.rev_and_compl(r) for r in rd])
    b.run()
    b.fetch()
    again = [b.gaf_text(i, "r%d" % i) for i in range(4)]
    assert [t.replace("\t-\t", "\t+\t", 1) for t in again] == first and all("\t-\t" in t for t in again)
    # a POA stream takes amb_strand = 2 as 1; a pathwise stream with it may keep its records (they are the chosen ones)
    st = api.Stream(g, api.make_params(api.MODE_RECOMBINATION), device_ids=[0], both_strands=True, keep_records=True)
    st.push([api.rev_and_compl(r) for r in rd])
    st.finish()
    t = st.next()
    assert t.records and all(b"\t-\t" in t.text_of(i) for i in range(4))
    st.close()
    with pytest.raises(api._lib.RecGraphError):
        api.Stream(g, api.make_params(api.MODE_GLOBAL_POA), device_ids=[0], both_strands=True, keep_records=True)


def test_one_full_size_launch(oracle):
    """Config-5 shape, ONE 4 096-read tile with every second read reverse-complemented: the second pass is a 2 048-read launch
    on the work buffers the 4 096-read pass just used (the gfx950 store hazard of round 5 only showed at full launches).  A
    384-read sample against the oracle run on the expected strand of each read."""
    from recgraph_amd import api, synth
    sg, _, _ = synth.make_config("C5", n_reads=1)
    g = api.Graph.from_gfa_text(sg.gfa())
    og = oracle.Graph.from_gfa_text(sg.gfa())
    base = synth.haplotype_reads(sg, 4096, 1000, seed=9431, mosaic_frac=0.5)
    reads = [_rc(r) if i % 2 else r for i, r in enumerate(base)]
    names = ["read%d" % i for i in range(4096)]
    check = sorted({k * 4095 // 383 for k in range(384)})           # 384 reads spread over the whole index range, 0 and 4095 included
    assert len(check) == 384 and sum(i % 2 for i in check) > 150
    _, _, exp = og.bench_text(oracle.M8_ABS, [base[i] for i in check], nthreads=_threads(96), name_prefix="x")
    assert all(_printed_score(t.decode()) >= 0 for t in exp)      # the expected strand aligns well: the other one cannot win
    texts, status = api.align_batch(g, reads, names, mode=api.MODE_RECOMBINATION, both_strands=True)
    assert not any(status)
    bad = []
    for k, i in enumerate(check):
        e = exp[k].decode().replace("x%d\t" % k, "read%d\t" % i, 1)
        if i % 2:
            e = _minus(e)
        if texts[i] != e:
            bad.append(i)
    assert not bad, (len(bad), bad[:12])
    assert sum("\t-\t" in t for t in texts) == 2048
