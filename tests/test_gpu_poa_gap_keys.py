"""Per-base, asymmetric gap entries in every POA mode (GPU vs the oracle), and the CPU check that these fixtures can see a
kernel that reads the wrong key.

Every matrix the other tests use has one gap cost for every base and (b,'-') == ('-',b): there it makes no difference
which base's gap a cell adds.  The kernels choose between several keys — the row base (li,'-') / ('-',li), the read base
(rc,'-') / ('-',rc), the gap key of the 8-column chunk head of the AVX2 flavours, the swapped substitution key of the
multi-predecessor tail — and `k_m0_simd<*, false>` (the per-lane gap-cost scan) runs only under such a matrix.  Here every
(b,'-') and ('-',b) entry, b in ACGTN, is distinct, and the substitutions of the small matrices are asymmetric too."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BASES = "ACGTN"

# (b,'-') and ('-',b) per base, A C G T N
GAPS = {
    "small": ((-3, -5, -7, -11, -13), (-4, -6, -9, -2, -8)),
    "zero": ((-2, 0, -3, -1, -4), (-1, -3, 0, -2, -5)),          # a free gap each way: ties between L / U and D
    "hoxd70": ((-150, -210, -180, -260, -120), (-190, -140, -240, -170, -230)),
}


def _subs(name):
    if name == "hoxd70":
        from recgraph_amd import api
        d = api.create_score_matrix_i32(matrix_file_path=os.path.join(HERE, "golden", "HOXD70.mtx"))
        return {k: v for k, v in d.items() if "-" not in k}
    d = {}
    for i, a in enumerate(BASES):
        for j, b in enumerate(BASES):
            if a == b:
                d[(a, b)] = (1 if name == "zero" else 3) if a != "N" else -1
            elif "N" in (a, b):
                d[(a, b)] = -1
            else:
                d[(a, b)] = -1 if name == "zero" and (i + j) % 2 else -2 - (3 * i + j) % 5     # (a,b) != (b,a)
    return d


def matrix(name, wrong=None):
    """The fixture matrix `name` as a {(a, b): score} dict; `wrong` = the same matrix as a kernel that reads a wrong key
    sees it: 'gaps_transposed' ((b,'-') <-> ('-',b)), 'gaps_one_value' (every gap entry = (A,'-')), 'subs_transposed'
    ((a,b) <-> (b,a))."""
    rg, gr = GAPS[name]
    d = dict(_subs(name))
    for k, b in enumerate(BASES):
        d[(b, "-")] = rg[k]
        d[("-", b)] = gr[k]
    if wrong == "gaps_transposed":
        for b in BASES:
            d[(b, "-")], d[("-", b)] = d[("-", b)], d[(b, "-")]
    elif wrong == "gaps_one_value":
        for b in BASES:
            d[(b, "-")] = d[("-", b)] = rg[0]
    elif wrong == "subs_transposed":
        d = {(k[1], k[0]) if "-" not in k else k: v for k, v in d.items()}
    elif wrong is not None:
        raise ValueError(wrong)
    return d


def _mutate(s, rng, every=20):
    s = list(s)
    for _ in range(len(s) // every):
        s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
    return "".join(s)


LENGTHS = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129)


def _single_base_gfa(n=160, seed=33):
    """Every row its own node, with skip edges: every row has listed predecessors (the multi-predecessor tails)."""
    rng = np.random.default_rng(seed)
    segs = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))
    gfa = "".join("S\t%d\t%s\n" % (i + 1, c) for i, c in enumerate(segs))
    gfa += "".join("L\t%d\t+\t%d\t+\t0M\n" % (i + 1, i + 2) for i in range(n - 1))
    gfa += "".join("L\t%d\t+\t%d\t+\t0M\n" % (i + 1, i + 3) for i in range(0, n - 2, 3))
    return gfa, segs


def _example_walk(gfa):
    segs, paths = {}, []
    for line in gfa.splitlines():
        f = line.split("\t")
        if f[0] == "S":
            segs[f[1]] = f[2]
        elif f[0] == "P":
            paths.append("".join(segs[s[:-1]] for s in f[2].split(",")))
    return paths[0]


def cases(example_gfa):
    """[(graph name, gfa text, reads)]: linear, bubbles, random DAG, single-base-node chain, the example graph.  Reads: whole
    source->sink walks with errors (real CIGARs with L runs), and prefixes (anchored at the source) and suffixes (reaching the
    sink: the scalar tail end..right) of a walk at lengths around 8 k and 64 k."""
    from recgraph_amd import synth
    rng = np.random.default_rng(77)
    out = []
    sgs = [("linear", synth.linear_graph(300, seed=41)), ("bubbles", synth.haplotype_graph(300, 5, path_len=140, seed=42)),
           ("random_dag", synth.random_dag_graph(40, 4, seed=43, max_seg=6, similar=0.6))]
    for name, sg in sgs:
        walk = sg.path_sequence(0)
        reads = synth.full_walk_reads(sg, 5, seed=int(rng.integers(1, 1000)))
        reads += [_mutate(walk[:k], rng) for k in LENGTHS if k <= len(walk)]
        reads += [_mutate(walk[-k:], rng) for k in LENGTHS if k <= len(walk)]
        out.append((name, sg.gfa(), reads))
    gfa, segs = _single_base_gfa()
    reads = [_mutate(segs, rng, 15) for _ in range(3)] + [_mutate(segs[:k], rng) for k in LENGTHS] + [_mutate(segs[-k:], rng) for k in LENGTHS[:8]]
    out.append(("single_base", gfa, reads))
    walk = _example_walk(example_gfa)
    reads = [_mutate(walk, rng, 25) for _ in range(2)] + [_mutate(walk[:k], rng) for k in LENGTHS] + [_mutate(walk[-k:], rng) for k in LENGTHS]
    out.append(("example", example_gfa, reads))
    return out


def poa_modes(oracle):
    """(api mode, oracle mode, [keyword sets]) of the six POA modes; o / e where they apply."""
    from recgraph_amd import api
    oe = [{"o": -4, "e": -2}, {"o": 0, "e": -3}, {"o": -10, "e": -1}]
    return [(api.MODE_GLOBAL_POA, oracle.M0_SIMD, [{}]), (api.MODE_GLOBAL_POA_SCALAR, oracle.M0_SCALAR, [{}]),
            (api.MODE_GAP_POA, oracle.M2, oe), (api.MODE_LOCAL_POA, oracle.M1_SIMD, [{}]),
            (api.MODE_LOCAL_POA_SCALAR, oracle.M1_SCALAR, [{}]), (api.MODE_GAP_LOCAL_POA, oracle.M3, oe)]


def _oracle_texts(oracle, og, omode, reads, scores, **kw):
    return [og.align(omode, rd, name="r%d" % i, idx=i + 1, scores=scores, **kw)[:3] for i, rd in enumerate(reads)]


# ---- CPU: the fixtures see a wrong key ------------------------------------------------------------------------------------
# Share of reads (over all graphs) whose oracle output changes when the matrix is read with a wrong key: lower bounds per
# (mode, wrong key) that every matrix must reach (measured on these fixtures: -m 0 0.88-1.00 for the gap keys and 0.18-0.82
# for the substitution key, -m 1 0.08-0.67 and 0.18-0.58, -m 2 / -m 3 0.31-0.62 for the substitution key).  -m 2 / -m 3 take
# their gaps from o / e and read no gap entry, so only the substitution key is visible there; HOXD70 is symmetric, so a
# transposed substitution key is invisible under it (the two small matrices are not).
POWER = {
    "M0_SIMD": {"gaps_transposed": 0.5, "gaps_one_value": 0.5, "subs_transposed": 0.1},
    "M0_SCALAR": {"gaps_transposed": 0.5, "gaps_one_value": 0.5, "subs_transposed": 0.1},
    "M2": {"subs_transposed": 0.1},
    "M1_SIMD": {"gaps_transposed": 0.05, "gaps_one_value": 0.05, "subs_transposed": 0.1},
    "M1_SCALAR": {"gaps_transposed": 0.05, "gaps_one_value": 0.05, "subs_transposed": 0.1},
    "M3": {"subs_transposed": 0.1},
}
SYMMETRIC_SUBS = ("hoxd70",)


def power_table(oracle, example_gfa):
    """{(mode name, matrix name, wrong key): (reads that differ, reads)}"""
    cs = cases(example_gfa)
    graphs = [(oracle.Graph.from_gfa_text(gfa, want_path=False), reads) for _, gfa, reads in cs]
    res = {}
    for mname in POWER:
        omode = getattr(oracle, mname)
        kw = {"o": -4, "e": -2} if mname in ("M2", "M3") else {}
        for name in GAPS:
            true_sc = oracle.scores_from_dict(matrix(name))
            base = [_oracle_texts(oracle, og, omode, reads, true_sc, **kw) for og, reads in graphs]
            for wrong in ("gaps_transposed", "gaps_one_value", "subs_transposed"):
                sc = oracle.scores_from_dict(matrix(name, wrong))
                diff = total = 0
                for (og, reads), b in zip(graphs, base):
                    w = _oracle_texts(oracle, og, omode, reads, sc, **kw)
                    diff += sum(x[:2] != y[:2] for x, y in zip(b, w))
                    total += len(reads)
                res[(mname, name, wrong)] = (diff, total)
    return res


def test_fixtures_detect_a_wrong_key(oracle, example_gfa):
    """The mistake each fixture targets changes the reference's output (text or score) on a stated share of the reads, in
    every mode that reads that key and every matrix under which the key matters."""
    t = power_table(oracle, example_gfa)
    need = {k: POWER[k[0]][k[2]] for k in t if k[2] in POWER[k[0]] and not (k[2] == "subs_transposed" and k[1] in SYMMETRIC_SUBS)}
    assert len(need) == 6 * 2 + 4 * 6
    weak = [(k, t[k], share) for k, share in need.items() if t[k][0] < share * t[k][1]]
    assert not weak, weak


# ---- GPU: every POA mode under these matrices -----------------------------------------------------------------------------
def compare(oracle, gfa, reads, mode, omode, sc, **kw):
    """Byte-identical text and the same Batch.score(i) as the oracle for every read."""
    from recgraph_amd import api
    og = oracle.Graph.from_gfa_text(gfa, want_path=False)
    g = api.Graph.from_gfa_text(gfa)
    b = api.Batch(g, reads, api.make_params(mode, score_matrix=sc, **kw))
    b.run()
    b.fetch()
    osc = oracle.scores_from_dict(sc)
    bad = []
    for i, rd in enumerate(reads):
        name = "r%d" % i
        exp, score, panic, _ = og.align(omode, rd, name=name, idx=i + 1, scores=osc, **kw)
        if panic:
            if not b.status(i) & api.READ_WOULD_PANIC:
                bad.append((i, "expected the panic status", b.status(i)))
            continue
        got = b.gaf_text(i, name, i + 1)
        if got != exp or b.score(i) != score:
            bad.append((i, len(rd), b.score(i), score, got[-300:], exp[-300:]))
    assert not bad, (len(bad), bad[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GAPS))
def test_per_base_asymmetric_gaps_every_poa_mode(oracle, example_gfa, name):
    sc = matrix(name)
    for gname, gfa, reads in cases(example_gfa):
        for mode, omode, kws in poa_modes(oracle):
            for kw in kws:
                compare(oracle, gfa, reads, mode, omode, sc, **kw)
