"""GPU: RG_AMB_STRAND_VOTE — RG_AMB_BOTH_STRANDS with the first strand of every read picked by a 12-mer vote (modes 4, 5,
8, 9; amb_mode = 12; include/recgraph_hip.h).

The vote is a pure function of (graph, read), so the expected text is BUILT from the oracle plus the Python statement of
the vote in tests/strand_vote_rule.py: the 12-mer set of the path sequences of the GFA, k_pick's sampling, first strand
'-' iff V_r > V_f; pass A on the first strand, pass B on the other one iff pass A scores < 0; with both aligned the reverse
record only if strictly greater."""
import numpy as np
import pytest

from strand_vote_rule import expected_strand_vote, gfa_paths, kmer_set, minus, oracle_texts, printed_score, rc, threads, votes

pytestmark = pytest.mark.gpu


def _omode(oracle, m):
    return {4: oracle.M4_ABS, 5: oracle.M5_ABS, 8: oracle.M8_ABS, 9: oracle.M9_ABS}[m]


def _amode(m):
    from recgraph_amd import api
    return {4: api.MODE_PATHWISE, 5: api.MODE_PATHWISE_SEMI, 8: api.MODE_RECOMBINATION, 9: api.MODE_RECOMBINATION_SEMI}[m]


def _vote_amb():
    from recgraph_amd import api
    return api.AMB_BOTH_STRANDS | api.AMB_STRAND_VOTE


def expected_both_strands(og, omode, reads, prefix="q"):
    """The exact rule of RG_AMB_BOTH_STRANDS, re-stated: forward; if its printed score is < 0 the reverse complement; the
    reverse record, strand '-', only when strictly greater."""
    out = oracle_texts(og, omode, reads, prefix)
    retry = {i for i, t in enumerate(out) if printed_score(t) < 0}
    if retry:
        sub = [rc(reads[i]) if i in retry else "A" for i in range(len(reads))]
        rev = oracle_texts(og, omode, sub, prefix)
        for i in retry:
            r = rev[i]
            if printed_score(r) > printed_score(out[i]):
                out[i] = minus(r)
    return out


def _mutate(rng, s, rate):
    s = list(s)
    for k in range(len(s)):
        if rng.random() < rate:
            s[k] = "ACGT"[int(rng.integers(0, 4))]
    return "".join(s)


def _random(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def _mixed_reads(path_seqs, n_each, seed, semi):
    """Walks, reverse-complemented walks, mosaics of two paths on both strands, 75 %-mutated reads, random reads, and
    reverse-complemented walks whose last ~85 % is random: a few of their 12-mers survive, so they go reverse first, score
    below 0 there and reach pass B."""
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

    def rc_head():
        s = rc(walk())
        keep = max(len(s) * 15 // 100, 16)
        return s[:keep] + _random(rng, len(s) - keep)
    n = len(path_seqs[0])
    rd = [walk() for _ in range(n_each)] + [rc(walk()) for _ in range(n_each)]
    rd += [mosaic() for _ in range(n_each)] + [rc(mosaic()) for _ in range(n_each)]
    rd += [_mutate(rng, walk(), 0.75) for _ in range(n_each)]
    rd += [_random(rng, int(rng.integers(n // 2, n))) for _ in range(n_each + 4)]
    rd += [rc_head() for _ in range(n_each + 3)]
    order = rng.permutation(len(rd))
    return [rd[int(k)] for k in order]


CASES = {
    # name: (graph, reads per kind, seed): the shapes of tests/test_gpu_both_strands.py
    "example": (None, 7, 101),
    "wide_70_paths": ((1500, 70, 300, 77), 7, 202),            # P > 64: several 64-path pages
    "striped_2150": ((5400, 4, 2150, 78), 6, 303),             # reads of 2 100+ bases: the column-striped kernels
}


def _case(name, m, example_gfa):
    from recgraph_amd import synth
    spec, n_each, seed = CASES[name]
    if spec is None:
        gfa = example_gfa
    else:
        gfa = synth.haplotype_graph(spec[0], spec[1], path_len=spec[2], seed=spec[3]).gfa()
    paths = gfa_paths(gfa)
    return gfa, kmer_set(paths), _mixed_reads(paths, n_each, seed + m, m in (5, 9))


def check_not_vacuous(m, exp):
    """Conditions on the INPUTS, from the oracle and the Python vote alone: >= 5 reads in each of (first strand) x (accepted |
    both aligned), both outcomes among the reads with both strands aligned, and for -m 8 / 9 a reverse winner of either GAF
    shape."""
    n = {(fr, both): sum(1 for e in exp if (e[1], e[2]) == (fr, both)) for fr in (False, True) for both in (False, True)}
    assert min(n.values()) >= 5, (m, n)
    assert {e[3] for e in exp if e[2]} == {True, False}, m
    if m in (8, 9):
        assert {e[4] for e in exp if e[3]} == {True, False}, m
    return n


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("m", [4, 5, 8, 9])
def test_parity_by_construction(oracle, example_gfa, m, name):
    from recgraph_amd import api
    gfa, kmers, reads = _case(name, m, example_gfa)
    og = oracle.Graph.from_gfa_text(gfa)
    om = _omode(oracle, m)
    exp = expected_strand_vote(og, om, kmers, reads)
    counts = check_not_vacuous(m, exp)          # before the GPU is touched
    print("strand vote -m %d %s: (first '-', both aligned) -> reads %s" % (m, name, counts))
    want = [e[0] for e in exp]
    names = ["q%d" % i for i in range(len(reads))]
    g = api.Graph.from_gfa_text(gfa)
    mode = _amode(m)
    texts, status = api.align_batch(g, reads, names, mode=mode, strand_vote=True)
    assert not any(status)
    bad = [(i, exp[i][1:], texts[i][-200:], want[i][-200:]) for i in range(len(reads)) if texts[i] != want[i]]
    assert not bad, (len(bad), bad[:2])
    # the stream, with tiles that split the set (rg_stream_opts.amb_strand = 3) on two handles, and the multi-device call
    stexts, sstatus = api.align_stream(g, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=11,
                                       strand_vote=True)
    assert stexts == want and sstatus == status
    if name == "example":
        mtexts, _ = api.align_batch_multi(g, reads, names, mode=mode, device_ids=[0], strand_vote=True)
        assert mtexts == want
    # the structured record and the accessors describe the chosen record
    b = api.Batch(g, reads, api.make_params(mode, amb=_vote_amb()))
    b.run()
    b.fetch()
    assert b.format_all(names).decode() == "".join(want)
    for i in range(len(reads)):
        e = api.GAFStruct.from_line(want[i].rstrip("\n"))
        f = b.fields(i, names[i])
        assert (f.strand, f.path, f.path_length, f.path_start, f.path_end, f.query_length, f.query_end, f.comments) == \
               (e.strand, e.path, e.path_length, e.path_start, e.path_end, e.query_length, e.query_end, e.comments), i
        assert f.strand == ("-" if exp[i][3] else "+")
        if "recombination path" not in want[i]:
            assert b.score(i) == int(printed_score(want[i]))
    # nothing else moved: bit 2 alone still follows the exact rule, and no bit gives the forward text
    both, _ = api.align_batch(g, reads, names, mode=mode, both_strands=True)
    assert both == expected_both_strands(og, om, reads)
    plain, _ = api.align_batch(g, reads, names, mode=mode)
    assert plain == oracle_texts(og, om, reads)


def _sweeps(stats):
    return sum(v[1] for k, v in stats.items() if k.startswith("k_sweep"))


def _run(g, reads, mode, amb):
    from recgraph_amd import api
    b = api.Batch(g, reads, api.make_params(mode, amb=amb))
    b.run()
    b.fetch()
    return b.kernel_stats(), b.cell_updates, [b.gaf_text(i, "q%d" % i) for i in range(len(reads))]


def _six_path_graph(oracle):
    from recgraph_amd import api, synth
    sg = synth.haplotype_graph(600, 6, path_len=200, seed=31)
    good = synth.haplotype_reads(sg, 24, 200, seed=5, mosaic_frac=0.5)
    return api.Graph.from_gfa_text(sg.gfa()), oracle.Graph.from_gfa_text(sg.gfa()), kmer_set(gfa_paths(sg.gfa())), good


def test_the_saving_is_real_without_a_clock(oracle):
    """Reverse-strand reads cost one launch set, not two: the kernel statistics say so."""
    from recgraph_amd import api
    g, og, kmers, good = _six_path_graph(oracle)
    back = [rc(r) for r in good]
    assert all(votes(kmers, r)[1] > votes(kmers, r)[0] for r in back) and not any(votes(kmers, r)[1] > votes(kmers, r)[0] for r in good)
    for m in (4, 8):
        mode, om = _amode(m), _omode(oracle, m)
        fwd = oracle_texts(og, om, good)
        assert all(printed_score(t) >= 0 for t in fwd)
        st_plain, cells_plain, t_plain = _run(g, good, mode, 0)
        assert t_plain == fwd
        st_vote, _, t_vote = _run(g, back, mode, _vote_amb())
        assert _sweeps(st_vote) == _sweeps(st_plain)
        assert st_vote["k_strand_vote"][1] == 1 and st_vote["k_strand_orient"][1] == 1 and "k_strand_merge" not in st_vote
        assert t_vote == [minus(t) for t in fwd]            # the oracle's record of the reverse complement, strand swapped
        st_exact, _, t_exact = _run(g, back, mode, api.AMB_BOTH_STRANDS)
        assert _sweeps(st_exact) >= 2 * _sweeps(st_plain) and "k_strand_vote" not in st_exact
        assert t_exact == t_vote
        st_fwd, cells_fwd, t_fwd = _run(g, good, mode, _vote_amb())
        assert t_fwd == t_plain and cells_fwd == cells_plain and _sweeps(st_fwd) == _sweeps(st_plain)


def test_edges(oracle):
    from recgraph_amd import api
    g, og, kmers, good = _six_path_graph(oracle)
    for m in (4, 8):
        mode, om = _amode(m), _omode(oracle, m)
        # bad-base reads: not voted, not retried, status kept, no text; their neighbours are untouched
        reads = [good[0], good[1][:80] + "X" + good[1][81:], rc(good[2]), "ACGT*" + rc(good[3])[5:], rc(good[4])]
        for r in (reads[1], reads[3]):
            assert og.align(om, r)[2] and votes(kmers, r) == (0, 0)
        texts, status = api.align_batch(g, reads, None, mode=mode, strand_vote=True)
        assert [bool(s & api.READ_BAD_BASE) for s in status] == [False, True, False, True, False]
        assert texts[1] == "" and texts[3] == ""
        e = expected_strand_vote(og, om, kmers, [reads[0], reads[2], reads[4]], prefix="x")
        assert [x[1] for x in e] == [False, True, True]
        for k, i in enumerate((0, 2, 4)):
            assert texts[i] == e[k][0].replace("x%d\t" % k, "read%d\t" % i, 1)
    tie = "ACGT" * 30
    assert rc(tie) == tie and votes(kmers, tie)[0] == votes(kmers, tie)[1]
    for m in (4, 5, 8, 9):
        mode, om = _amode(m), _omode(oracle, m)
        # a palindromic read ties at the vote, goes forward first, is retried, ties again and stays '+'
        f = og.align(om, tie, name="t")[0]
        assert printed_score(f) < 0
        b = api.Batch(g, [tie, rc(good[0])], api.make_params(mode, amb=_vote_amb()))
        b.run()
        b.fetch()
        assert b.gaf_text(0, "t") == f and "\t+\t" in f and "\t-\t" in b.gaf_text(1, "u")
        assert b.kernel_stats()["k_strand_merge"][1] == 1
        # reads shorter than 12 bases and a read of N only vote 0 / 0: forward first, and the rule from there on
        short = ["ACGTACGTACG", "T", "N" * 40, "NNNN", good[1], rc(good[5])]
        assert [votes(kmers, r) for r in short[:4]] == [(0, 0)] * 4
        e = expected_strand_vote(og, om, kmers, short)
        assert [x[1] for x in e] == [False, False, False, False, False, True]
        texts, status = api.align_batch(g, short, ["q%d" % i for i in range(6)], mode=mode, strand_vote=True)
        assert texts == [x[0] for x in e] and not any(status)
        # set_reads on a used handle: the vote and the first pass's buffer follow the new reads
        b.set_reads(short)
        b.run()
        b.fetch()
        assert [b.gaf_text(i, "q%d" % i) for i in range(6)] == texts
        b.set_reads([rc(r) for r in good] + good)
        b.run()
        b.fetch()
        e = expected_strand_vote(og, om, kmers, [rc(r) for r in good] + good)
        assert [b.gaf_text(i, "q%d" % i) for i in range(48)] == [x[0] for x in e]
        assert [x[1] for x in e] == [True] * 24 + [False] * 24
    # a pathwise stream with the vote may keep its records: they are the chosen ones
    st = api.Stream(g, api.make_params(api.MODE_RECOMBINATION), device_ids=[0], strand_vote=True, keep_records=True)
    st.push([rc(r) for r in good[:4]])
    st.finish()
    t = st.next()
    assert t.records and all(b"\t-\t" in t.text_of(i) for i in range(4))
    st.close()
    # the POA modes refuse the keyword, and a pathwise handle refuses bit 3 alone
    with pytest.raises(api._lib.RecGraphError):
        api.align_batch(g, good[:2], None, mode=api.MODE_GAP_POA, strand_vote=True)
    with pytest.raises(api._lib.RecGraphError) as ex:
        api.Batch(g, good[:2], api.make_params(api.MODE_RECOMBINATION, amb=api.AMB_STRAND_VOTE))
    assert ex.value.code == -1


def test_one_full_size_launch(oracle):
    """Config-5 shape, ONE 4 096-read tile with every second read reverse-complemented: pass A is one 4 096-read launch set
    (the sweep launches of the plain run on the source reads), nothing reaches pass B, exactly the 2 048 reversed reads come
    out '-'.  A 384-read sample against the oracle run on the expected strand of each read."""
    from recgraph_amd import api, synth
    sg, _, _ = synth.make_config("C5", n_reads=1)
    gfa = sg.gfa()
    g = api.Graph.from_gfa_text(gfa)
    og = oracle.Graph.from_gfa_text(gfa)
    kmers = kmer_set(gfa_paths(gfa))
    base = synth.haplotype_reads(sg, 4096, 1000, seed=9431, mosaic_frac=0.5)
    reads = [rc(r) if i % 2 else r for i, r in enumerate(base)]
    check = sorted({k * 4095 // 383 for k in range(384)})           # 384 reads spread over the whole index range, 0 and 4095 included
    assert len(check) == 384 and sum(i % 2 for i in check) > 150
    for i in check:
        vf, vr = votes(kmers, reads[i])
        assert (vr > vf) == bool(i % 2), (i, vf, vr)
    _, _, exp = og.bench_text(oracle.M8_ABS, [base[i] for i in check], nthreads=threads(96), name_prefix="x")
    assert all(printed_score(t.decode()) >= 0 for t in exp)      # the voted strand is accepted: pass B has nothing to do
    b = api.Batch(g, reads, api.make_params(api.MODE_RECOMBINATION, amb=_vote_amb()))
    b.run()
    b.fetch()
    st = b.kernel_stats()
    texts = b.format_all(["read%d" % i for i in range(4096)]).decode().splitlines(True)
    assert len(texts) == 4096 and not any(b.status(i) for i in check)
    bad = []
    for k, i in enumerate(check):
        e = exp[k].decode().replace("x%d\t" % k, "read%d\t" % i, 1)
        if i % 2:
            e = minus(e)
        if texts[i] != e:
            bad.append(i)
    assert not bad, (len(bad), bad[:12])
    assert sum("\t-\t" in t for t in texts) == 2048 and all(("\t-\t" in t) == bool(i % 2) for i, t in enumerate(texts))
    assert st["k_strand_vote"][1] == 1 and st["k_strand_orient"][1] == 1 and "k_strand_merge" not in st
    del b
    st_plain, _, _ = _run(g, base, api.MODE_RECOMBINATION, 0)
    assert _sweeps(st) == _sweeps(st_plain)
