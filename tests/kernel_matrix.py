"""The kernel matrix: one entry per compiled `__global__` instantiation of recgraph_amd/csrc/*.hip, as data.

MATRIX maps the name of an instantiation — the demangled symbol without its parameter list, what
tools/kernel_resources.py report() prints and what the launch log (RG_LAUNCH_LOG, csrc/rg_launch_log.hpp) records as
"inst:<name>" — to the id of a CASE that launches it, or to an Unreachable with its reason.  A case is one or more batches of
one mode on one synthetic graph: (mode, graph recipe of recgraph_amd/synth.py, read lengths per batch, score matrix, option
switches, alignment parameters).  tests/test_kernel_matrix_cpu.py checks that the key set equals what hipcc compiles and
that the oracle answers every case; tests/test_gpu_kernel_matrix.py runs every case with the log on, compares every read with
the oracle byte for byte and asserts that the entry's instantiation was launched.

How the cases are shaped:
  * the plan doubles C (columns per lane) from 4 while 64 C < n + 1, so the longest read of a batch sits ON a boundary: 255 (C = 4),
    511 and 256 (C = 8), 1023 and 512 (16), 2047 and 1024 (32), 2048 (the first striped batch); every batch also has a 1-base
    read (idle lanes) and one of 64 C / 2 bases (the half-row boundary of the packed rows);
  * paths: 1, 5, 6, 3 and 64 on the narrow side; 65 (the first kWide count), 129 and 256 (both page edges of the 4 x u64 path
    sets) on the wide side;
  * k_sweep16: every C x {records (-m 8 / 9), no tracking (-m 4 / 5), column maxima (three_sweeps / no_frec)} x {<= 64, > 64
    paths} x {global, semiglobal}; the i32 kernels through sweep_i32 (uniform gaps) and a matrix with per-base gap costs;
  * the POA kernels on both sides of `lds_read = max_n <= 16000` (rg_poa_driver.hip): a longest read of 16000 and of 16001 bases;
  * graphs alternate between synth.random_dag_graph and synth.haplotype_graph; graphs for C <= 8 run at retire_shift 4 so that
    path retirement is live on them.

Oracle budget: a pathwise case costs the oracle about rows x bases x paths cells per read; the largest case here (C = 32,
65 paths, reads of 2047 + 1024 + 1024 bases on ~1900 rows) is 5e8 cells, every other one less (the cap: 1e9 per case).
test_kernel_matrix_cpu.py prints the oracle's wall time over the whole matrix (see its docstring for the measured figure).
"""
from collections import namedtuple

# ---- names ------------------------------------------------------------------------------------------------------------------
CS = (4, 8, 16, 32)
STRIPE_CS = (8, 16, 32)


def _b(x):
    return "true" if x else "false"


def sweep16(C, colmax, rec, wide, semi):
    """rg::k_sweep16<C, kColmax, kRec, kWide, kSemi>"""
    return "rg::k_sweep16<%d, %d, %s, %s, %s>" % (C, colmax, _b(rec), _b(wide), _b(semi))


def sweep(C, uni, stripes=False):
    return "rg::k_sweep<%d, %s, %s>" % (C, _b(uni), _b(stripes))


def layer(C, stripes=False):
    return "rg::k_layer<%d, %s>" % (C, _b(stripes))


def templ(kernel, *args):
    return "rg::%s<%s>" % (kernel, ", ".join(_b(a) if isinstance(a, bool) else str(a) for a in args))


# the variants tests/test_kernel_resources.py holds to register budgets
SWEEP16_M8 = sweep16(16, 0, True, False, False)
SWEEP16_M4 = sweep16(16, 0, False, False, False)
SWEEP16_M8_C32 = sweep16(32, 0, True, False, False)
LAYER16_C16 = templ("k_layer16", 16)
SWEEP16_NO_SCRATCH = [sweep16(c, 0, rec, False, semi) for c in (4, 8) for rec in (True, False) for semi in (False, True)]

# ---- cases ------------------------------------------------------------------------------------------------------------------
# mode: the -m number (api.MODE_* / the oracle's *_ABS restatement of it); graph: (recipe, arguments of the synth function);
# batches: read lengths, one list per batch; scores: "default" | "pergap"; options: rg_set_option switches for the GPU run;
# kw: alignment parameters for both sides; stream: tile size for a second run through the streaming engine (0: none);
# strands: the batch runs with RG_AMB_BOTH_STRANDS | RG_AMB_STRAND_VOTE on a read set with reverse complements
Case = namedtuple("Case", "mode graph batches scores options kw stream strands")
Unreachable = namedtuple("Unreachable", "reason proof")      # proof: the host-only check that states the impossibility

CASES = {}
MATRIX = {}
LONGEST = {4: (255,), 8: (511, 256), 16: (1023, 512), 32: (2047, 1024)}
NARROW_P = {4: 5, 8: 64, 16: 6, 32: 3}
WIDE_P = {4: 256, 8: 129, 16: 65, 32: 65}


def _graph(n, P, seed, dag):
    """A graph whose paths are about n bases long."""
    if dag:
        return ("random_dag", dict(n_segments=max(8, n * 10 // 36), n_paths=P, seed=seed, max_seg=9, max_jump=2, similar=0.5))
    return ("haplotype", dict(target_rows=max(40, n * 13 // 10), n_paths=P, path_len=max(24, n), seed=seed))


def _batches(C):
    hi, lo = LONGEST[C][0], LONGEST[C][-1]
    out = [[hi, 32 * C, 1] + ([hi * 2 // 3] if C < 32 else [])]
    if lo != hi:
        out.append([lo, 1] + ([lo // 2] if C < 32 else []))
    return out


def _case(cid, **kw):
    d = dict(mode=8, graph=None, batches=None, scores="default", options={}, kw={}, stream=0, strands=False)
    d.update(kw)
    assert cid not in CASES, cid
    CASES[cid] = Case(**d)
    return cid


def _entry(name, cid):
    assert name not in MATRIX, name
    MATRIX[name] = cid


def _small(C, opts):
    """graphs for C <= 8 are small: path retirement only evaluates on them at a short period"""
    return dict(opts, retire_shift=4) if C <= 8 else dict(opts)


def _fill():
    seed = 9000
    # ---- k_sweep16: 4 C x 3 pipelines x 2 widths x 2 end rules -------------------------------------------------------------
    for ci, C in enumerate(CS):
        for wide in (False, True):
            for semi in (False, True):
                P = WIDE_P[C] if wide else (1 if (C == 4 and semi) else NARROW_P[C])
                for colmax, rec in ((0, True), (0, False), (1, False)):
                    seed += 1
                    mode = (5 if semi else 4) if (colmax, rec) == (0, False) else (9 if semi else 8)
                    opts = {}
                    if (colmax, rec) == (1, False):
                        opts = {"three_sweeps": 1} if C in (4, 16) else {"no_frec": 1}
                    cid = "sweep16-C%d-%d%s-%s-%s" % (C, colmax, "rec" if rec else "", "wide" if wide else "narrow", "semi" if semi else "global")
                    # (the packed rows are only admitted while every stored value fits 16 bits, sweep16_admissible in rg_path_plan.cpp:
                    # with the default scores 8 (rows of a path + 2) + 10 (n + 2) <= 32000 — a 2047-base read needs paths of at most
                    # 1436 rows, so the graphs for C = 32 have paths of about 1100 rows and the long reads run past their end)
                    g = _graph(min(LONGEST[C][0], 1100), P, seed, dag=(ci + int(semi) + int(wide)) % 2 == 0)
                    # one C per family also goes through the stream: tiles of one read, so the longest read of a TILE picks C
                    stream = 1 if (C == 8 and not wide and not semi) else 0
                    _entry(sweep16(C, colmax, rec, wide, semi), _case(cid, mode=mode, graph=g, batches=_batches(C), options=_small(C, opts), stream=stream))
    # ---- what rides on those batches -----------------------------------------------------------------------------------------
    for C in CS:
        m8 = "sweep16-C%d-0rec-narrow-global" % C
        for k in ("k_opt0_16", "k_layer16", "k_expand", "k_colmax_rec", "k_trace"):
            _entry(templ(k, C), m8)
    m8, m4 = "sweep16-C16-0rec-narrow-global", "sweep16-C16-0-narrow-global"
    for k in ("k_pick", "k_seed", "k_threshold", "k_bound", "k_search", "k_order", "k_need", "k_verify"):
        _entry("rg::" + k, m8)
    _entry("rg::k_verify4", m4)
    # ---- the i32 kernels: sweep_i32 (uniform read-gap cost) and per-base gap costs, -m 8 (k_opt0 and k_layer in their i32 forms too)
    for ci, C in enumerate(CS):
        for uni in (True, False):
            seed += 1
            cid = "sweep32-C%d-%s" % (C, "uni" if uni else "pergap")
            _case(cid, mode=8, graph=_graph(LONGEST[C][0], 4 + ci, seed, dag=(ci + int(uni)) % 2 == 0), batches=_batches(C),
                  scores="default" if uni else "pergap", options=_small(C, {"sweep_i32": 1} if uni else {}), stream=1 if (C == 8 and uni) else 0)
            _entry(sweep(C, uni), cid)
        _entry(templ("k_opt0", C), "sweep32-C%d-uni" % C)
        _entry(layer(C), "sweep32-C%d-pergap" % C)
    # ---- reads of more than 2047 bases: column stripes (i32 rows; 8 columns per lane only through stripe_c) ---------------------
    for C, n, opts in ((8, 2048, {"stripe_c": 8}), (16, 2048, {}), (32, 8192, {})):
        seed += 1
        cid = "striped-C%d" % C
        _case(cid, mode=8, graph=_graph(n, 2, seed, dag=False), batches=[[n, 32 * C, 1]], options=opts)
        _entry(sweep(C, True, True), cid)
        _entry(templ("k_opt0_striped", C), cid)
        _entry(layer(C, True), cid)
    # ---- second pass (every read fails a speculative bound of +10^6) and both strands with the 12-mer vote ----------------------
    seed += 1
    _case("second-pass", mode=8, graph=_graph(300, 6, seed, dag=True), batches=[[300, 255, 1, 128, 200, 77]], options={"spec_margin": -1000000, "retire_shift": 4})
    _entry("rg::k_gather_reads", "second-pass")
    _entry("rg::k_scatter_results", "second-pass")
    seed += 1
    _case("strand-vote", mode=8, graph=_graph(300, 6, seed, dag=False), batches=[[300, 255, 280, 128, 200, 290, 150, 260]], strands=True)
    for k in ("k_strand_vote", "k_strand_orient", "k_strand_gate", "k_revcomp", "k_strand_merge"):
        _entry("rg::" + k, "strand-vote")
    # ---- POA: both sides of lds_read (longest read 16000 / 16001), uniform and per-base gap costs ------------------------------
    poa_kw = {"b": 2000.0, "f": 0.0}
    for lds in (True, False):
        n = 16000 if lds else 16001
        side = "lds" if lds else "global"
        for uni in (True, False):
            cid = "m0-%s-%s" % (side, "uni" if uni else "pergap")
            _case(cid, mode=0, graph=("linear", dict(target_rows=1200, seed=13)), batches=[[n, 1200, 64, 1]], scores="default" if uni else "pergap", kw=poa_kw)
            _entry(templ("k_m0_simd", lds, uni), cid)
        for gap, mode in ((True, 2), (False, 10)):
            cid = "m%d-%s" % (mode, side)
            _case(cid, mode=mode, graph=("linear", dict(target_rows=1200, seed=14)), batches=[[n, 1200, 64, 1]], kw=dict(poa_kw, **({"o": -4, "e": -2} if gap else {})))
            _entry(templ("k_poa_banded", gap, lds), cid)
        for var, mode in ((0, 1), (1, 11), (2, 3)):
            cid = "m%d-%s" % (mode, side)
            _case(cid, mode=mode, graph=("linear", dict(target_rows=600, seed=15)), batches=[[n, 600, 64, 1]], kw={"o": -6, "e": -1} if mode == 3 else {})
            _entry(templ("k_poa_local", var, lds), cid)


_fill()
# the entry whose instantiation the stream run of a case must show as well (one C per family)
MATRIX_STREAM_KEYS = {"sweep16-C8-0rec-narrow-global": sweep16(8, 0, True, False, False), "sweep32-C8-uni": sweep(8, True)}
REACHABLE = sorted(k for k, v in MATRIX.items() if not isinstance(v, Unreachable))


# ---- building a case ---------------------------------------------------------------------------------------------------------
def scores_table(case, default36):
    """36 ints (ALPHABET "ACGTN-" x itself) for make_params(score_matrix=...) and oracle align(scores=...), or None for the mode's default.
    "pergap": match 3 / mismatch -5 with the gap entries of A at -7 and of G at -12 (the other bases: -10) — `default36` is
    scores_match_mis(3, -5) of either side."""
    if case.scores == "default":
        return None
    t = list(default36)
    for base, v in ((0, -7), (2, -12)):
        t[base * 6 + 5] = v
        t[5 * 6 + base] = v
    return t


def build(case):
    """(SynthGraph, [reads of batch 0, reads of batch 1, ...]) of a case."""
    import numpy as np
    from recgraph_amd import synth
    kind, args = case.graph
    g = {"random_dag": synth.random_dag_graph, "haplotype": synth.haplotype_graph, "linear": synth.linear_graph}[kind](**args)
    seed = 7 * args["seed"]
    batches = []
    for bi, lens in enumerate(case.batches):
        reads = []
        for k, n in enumerate(lens):
            if kind == "linear":        # POA: a walk of the backbone, continued at random behind the graph's end
                rng = np.random.default_rng(seed + 100 * bi + k)
                walk = g.path_sequence(0)
                reads.append((walk + "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=max(0, n - len(walk)))))[:n])
            else:
                reads.append(synth.haplotype_reads(g, 1, length=n, seed=seed + 100 * bi + k, mosaic_frac=0.5)[0])
        if case.strands:                # every second read on the other strand, and two reads that fit neither
            comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
            reads = [("".join(comp[c] for c in reversed(r)) if i % 2 else r) for i, r in enumerate(reads)]
            rng = np.random.default_rng(seed + 1)
            reads += ["".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=m)) for m in (90, 200)]
        batches.append(reads)
    return g, batches


def oracle_mode(O, mode):
    return {0: O.M0_SIMD, 10: O.M0_SCALAR, 2: O.M2, 1: O.M1_SIMD, 11: O.M1_SCALAR, 3: O.M3, 4: O.M4_ABS, 5: O.M5_ABS, 8: O.M8_ABS, 9: O.M9_ABS}[mode]


def oracle_texts(O, case, gfa, reads, threads=8):
    """[(text, would_panic)] per read of one batch, read i named r<i> with sequence index i + 1."""
    from concurrent.futures import ThreadPoolExecutor
    og = O.Graph.from_gfa_text(gfa, want_path=case.mode in (4, 5, 8, 9))
    sc = scores_table(case, O.scores_match_mis(3, -5))
    om = oracle_mode(O, case.mode)

    def one(i):
        t = og.align(om, reads[i], name="r%d" % i, idx=i + 1, scores=sc, **case.kw)
        return t[0], t[2]
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range(len(reads))))


def oracle_cells(g, case):
    """rows x bases x paths summed over the reads of a case (pathwise modes): the oracle's cost in cells."""
    P = len(g.paths) if case.mode in (4, 5, 8, 9) else 1
    return g.rows * P * sum(sum(b) for b in case.batches)
