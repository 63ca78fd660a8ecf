"""The value the forward-bound kernels write (`k_opt0`, `k_opt0_striped`, `k_opt0_16`: lb[rd]) never reaches the output: a bound that
is too low only prunes less, one that is too high only sends the read through a second pass, and both leave every byte right.  This
pins it from both sides on inputs where its exact value is known.

The graph has ONE path through rows of a random sequence, so k_pick picks path 0, no recombination exists, and the search maximum
k_verify compares with the bound (`fscore`) is the seed: the read's exact global score against that path — what the bound kernel
computes before it subtracts the margin.  k_verify retries a read iff fscore < lb, and a retry shows as `inst:rg::k_gather_reads`
in the batch's kernel statistics (launch log on).  One read per batch, -m 8, default scores:

  * `spec_margin` 0: lb = the score; no k_gather_reads — the bound is not too high;
  * `spec_margin` -1: lb = the score + 1 (+ 3 for the striped reads: long reads scale the margin per kbp); one k_gather_reads — the
    bound is not too low;
  * in every run the text equals the oracle's (M8_ABS), and the launch log names the intended instantiation.

Shapes, the smallest that reach each kernel (the longest read of a shape decides the columns per lane, so the rows are one fewer than
the shape's bases and the insertion read reaches them): `sweep_i32` at 255 (C = 4) and 1023 bases (C = 16) for k_opt0; 2050 bases
with `stripe_c` 8 and plain for k_opt0_striped<8> / <16>; the defaults with `no_dsel` at 255 and 1023 bases for k_opt0_16.  Reads per
shape: the path itself, five substitutions, one inserted base, one deleted base.  The CPU half asks plan_pathwise (tests/c/
forward_bound_plan.cpp) that these shapes and options give the geometry, `spec` on and `dsel` off: a plan change cannot empty the GPU
half silently."""
import subprocess

import numpy as np
import pytest

import plan_check_build

# id -> (bases of the longest read, options, instantiation of the bound kernel, (C, nwv, use16 / opt16), lb - score at spec_margin -1)
CASES = {
    "i32_c4": (255, {"sweep_i32": 1}, "rg::k_opt0<4>", (4, 1, 0), 1),
    "i32_c16": (1023, {"sweep_i32": 1}, "rg::k_opt0<16>", (16, 1, 0), 1),
    "striped_c8": (2050, {"stripe_c": 8}, "rg::k_opt0_striped<8>", (8, 5, 0), 3),
    "striped_c16": (2050, {}, "rg::k_opt0_striped<16>", (16, 3, 0), 3),
    "packed_c4": (255, {"no_dsel": 1}, "rg::k_opt0_16<4>", (4, 1, 1), 1),
    "packed_c16": (1023, {"no_dsel": 1}, "rg::k_opt0_16<16>", (16, 1, 1), 1),
}
OPTS = ("sweep_i32", "stripe_c", "no_dsel", "spec_margin", "launch_log")


def _inputs(bases):
    """(gfa of a one-path graph of bases - 1 rows, the reads): deterministic per shape."""
    from recgraph_amd import synth
    rng = np.random.default_rng(bases)
    seq = synth._rand_seq(rng, bases - 1)
    segments, at = [], 0
    while at < len(seq):
        ln = int(rng.integers(1, 40))
        segments.append((len(segments) + 1, seq[at:at + ln]))
        at += ln
    ids = [i for i, _ in segments]
    g = synth.SynthGraph(segments, list(zip(ids, ids[1:])), [ids])
    other = lambda c: "ACGT"[("ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]
    sub = list(seq)
    for k in rng.choice(len(seq), size=5, replace=False):
        sub[int(k)] = other(sub[int(k)])
    k_ins, k_del = int(rng.integers(20, len(seq) - 20)), int(rng.integers(20, len(seq) - 20))
    reads = [seq, "".join(sub), seq[:k_ins] + other(seq[k_ins]) + seq[k_ins:], seq[:k_del] + seq[k_del + 1:]]
    assert max(len(r) for r in reads) == bases and min(len(r) for r in reads) == bases - 2
    return g.gfa(), reads


_REF = {}


def _reference(oracle, bases):
    """The oracle's texts of a shape, computed once (the packed and the i32 cases share theirs) and left unchanged."""
    if bases not in _REF:
        gfa, reads = _inputs(bases)
        og = oracle.Graph.from_gfa_text(gfa)
        _REF[bases] = (gfa, reads, tuple(og.align(oracle.M8_ABS, rd, name="r", idx=1)[0] for rd in reads))
    return _REF[bases]


def _run(gg, read, options):
    """(text, {instantiation: launches}) of a one-read batch under `options` and the launch log (options restored afterwards)."""
    from recgraph_amd import api
    lib = api._lib.load()
    before = {k: lib.rg_get_option(k.encode()) for k in OPTS}
    try:
        for k, v in dict(options, launch_log=1).items():
            api.set_option(k, v)
        b = api.Batch(gg, [read], api.make_params(api.MODE_RECOMBINATION))
        b.run()
        b.fetch()
        text = b.gaf_text(0, "r", 1)
        stats = b.kernel_stats()
    finally:
        for k, v in before.items():
            api.set_option(k, v)
    return text, {k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_bound_is_the_exact_score(oracle, case):
    from recgraph_amd import api
    bases, options, kernel, _, _ = CASES[case]
    gfa, reads, expected = _reference(oracle, bases)
    assert len(reads) >= 2
    gg = api.Graph.from_gfa_text(gfa)
    for i, rd in enumerate(reads):
        for margin, retries in ((0, 0), (-1, 1)):
            text, insts = _run(gg, rd, dict(options, spec_margin=margin))
            opt0 = {k: v for k, v in insts.items() if k.startswith("rg::k_opt0")}
            print(case, "read", i, "margin", margin, "k_gather_reads", insts.get("rg::k_gather_reads", 0), opt0)
            assert text == expected[i], (case, i, margin, text[-200:], expected[i][-200:])
            assert kernel in opt0, (case, i, margin, opt0)
            assert insts.get("rg::k_gather_reads", 0) == retries, (case, i, margin, insts)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return plan_check_build.build("forward_bound_plan", tmp_path_factory.mktemp("forward_bound"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_speculates_without_words_on_demand(plan_exe, case):
    """CPU: the plan of every batch of the GPU half — each read alone is the longest of its batch."""
    bases, options, kernel, (C, nwv, packed), above = CASES[case]
    for n in (bases - 2, bases - 1, bases):
        for margin in (0, -1):
            args = [plan_exe, str(bases - 1 + 2), str(n)] + ["%s=%d" % kv for kv in dict(options, spec_margin=margin).items()]
            out = subprocess.run(args, capture_output=True, text=True, timeout=60)
            assert out.returncode == 0, out.stderr
            qC, qnwv, use16, opt16, spec, dsel, qmargin = (int(x) for x in out.stdout.split())
            assert (qC, qnwv, use16, opt16) == (C, nwv, packed, packed), (case, n, out.stdout)
            assert spec == 1 and dsel == 0, (case, n, out.stdout)
            assert qmargin == (0 if margin == 0 else -above), (case, n, margin, out.stdout)
    # the kernel the launchers pick from that plan: packed -> k_opt0_16, stripes -> k_opt0_striped, else k_opt0
    assert kernel == ("rg::k_opt0_16<%d>" % C if packed else "rg::k_opt0_striped<%d>" % C if nwv > 1 else "rg::k_opt0<%d>" % C)
