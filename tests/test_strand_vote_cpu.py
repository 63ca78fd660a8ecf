"""CPU: the interface of RG_AMB_STRAND_VOTE (the first strand of RG_AMB_BOTH_STRANDS by a 12-mer vote) without a device —
the constant in the header, the ctypes binding, the Python API and the Rust shim agree, the keyword and the CLI flag exist
and are refused for modes 0-3, the parameter checks of rg_batch_create answer before any device is needed, the path has no
CPU fallback, the two kernels of rg_strand_vote.hip stay small, and the Python statement of the vote
(tests/strand_vote_rule.py) sends walks of a path forward first and their reverse complements reverse first."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from strand_vote_rule import first_reverse, gfa_paths, kmer_set, rc, votes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rg():
    from recgraph_amd import _lib
    _lib.build_library()
    import recgraph_amd
    return recgraph_amd


def test_constant_agrees_everywhere(rg):
    from recgraph_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "recgraph_hip.h")).read()
    m = re.search(r"^#define RG_AMB_STRAND_VOTE (\d+)$", hdr, re.M)
    assert m and int(m.group(1)) == 8 == _lib.AMB_STRAND_VOTE == api.AMB_STRAND_VOTE
    assert api.make_params(api.MODE_RECOMBINATION, amb=api.AMB_BOTH_STRANDS | api.AMB_STRAND_VOTE).amb_mode == 12
    ffi = open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    assert re.search(r"RG_AMB_STRAND_VOTE\b.*=\s*8\s*;", ffi)
    # the library keeps its 63 symbols: the feature is a parameter bit, not an entry point
    assert len(_lib.SYMBOLS) == 63
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream, api.Stream.__init__):
        assert inspect.signature(fn).parameters["strand_vote"].default is False, fn


def test_cli_flag():
    from recgraph_amd import cli
    p = cli.build_parser()
    assert p.parse_args(["r.fa", "g.gfa", "-m", "8"]).strand_vote is False
    assert p.parse_args(["r.fa", "g.gfa", "-m", "8", "--strand-vote"]).strand_vote is True
    for m in ("0", "1", "2", "3"):
        with pytest.raises(SystemExit) as ex:        # refused before the graph file is even opened
            cli.main(["no_such_reads.fa", "no_such_graph.gfa", "-m", m, "--strand-vote"])
        assert "--strand-vote" in str(ex.value) and "-s true" in str(ex.value)


def test_refusals_need_no_device_and_the_path_has_no_cpu_fallback(rg, example_gfa):
    from recgraph_amd import _lib, api
    g = api.Graph.from_gfa_text(example_gfa)
    rd = ["ACGTACGTACGTACGTAC", "TTGACCA"]
    # bit 3 without bit 2, bit 3 in a POA mode, a higher bit: RG_ERR_ARG
    for mode, amb in ((api.MODE_PATHWISE, 8), (api.MODE_RECOMBINATION, 8), (api.MODE_RECOMBINATION_SEMI, 9), (api.MODE_PATHWISE_SEMI, 9),
                      (api.MODE_GLOBAL_POA, 12), (api.MODE_GAP_LOCAL_POA, 12), (api.MODE_RECOMBINATION, 16), (api.MODE_PATHWISE, 28)):
        with pytest.raises(_lib.RecGraphError) as e:
            api.Batch(g, rd, api.make_params(mode, amb=amb))
        assert e.value.code == -1, (mode, amb)
    # the Python keyword is refused for the POA modes before the library is asked
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
        with pytest.raises(_lib.RecGraphError) as e:
            fn(g, rd, None, mode=api.MODE_GAP_POA, strand_vote=True)
        assert e.value.code == -1 and "strand_vote" in str(e.value) and "-s true" in str(e.value)
    if _lib.load().rg_device_count() > 0:
        texts, status = api.align_batch(g, rd, None, mode=api.MODE_PATHWISE, strand_vote=True)
        assert len(texts) == 2 and not any(status)
        return
    # amb_mode = 12 on a pathwise mode passes the parameter check: what stops the call is the missing device
    for mode in api.PATHWISE_MODES:
        with pytest.raises(_lib.RecGraphError) as e:
            api.Batch(g, rd, api.make_params(mode, amb=12))
        assert e.value.code == -3, mode
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
        with pytest.raises(_lib.RecGraphError) as e:
            fn(g, rd, None, mode=api.MODE_RECOMBINATION, strand_vote=True)
        assert e.value.code == -3, fn


def test_vote_kernels_are_small():
    """They run beside the sweeps of the other handles, which leave 64 VGPRs per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = {k["name"].split("(")[0]: k for k in kernel_resources.report("rg_strand_vote.hip")}
    assert set(ks) == {"rg::k_strand_vote", "rg::k_strand_orient"}, sorted(ks)
    for name, k in ks.items():
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["VGPRs"] <= 64, (name, k)
    hits, stores = kernel_resources.store_hazards("rg_strand_vote.hip")
    assert not hits, hits[:4]


def test_python_vote_on_the_example_graph(example_gfa):
    paths = gfa_paths(example_gfa)
    kmers = kmer_set(paths)
    rng = np.random.default_rng(12)
    for p in paths:
        for _ in range(4):
            w = "".join(c if rng.random() >= 0.01 else "ACGT"[int(rng.integers(0, 4))] for c in p)
            vf, vr = votes(kmers, w)
            assert vf > 10 * max(vr, 1), (vf, vr)
            assert votes(kmers, rc(w)) == (vr, vf)          # the vote of the reverse complement is the mirror image
            assert not first_reverse(kmers, w) and first_reverse(kmers, rc(w))
    # ties go forward; short reads, N-only reads and reads with a character outside ACGTN vote 0 / 0
    assert votes(kmers, "ACGT" * 30)[0] == votes(kmers, "ACGT" * 30)[1] and not first_reverse(kmers, "ACGT" * 30)
    for r in ("ACGTACGTACG", "N" * 50, paths[0][:40] + "X" + paths[0][41:]):
        assert votes(kmers, r) == (0, 0) and not first_reverse(kmers, r)
    # the sampling: at most 256 windows, every ceil(npos / 256)-th one
    long_walk = (paths[0] * 40)[:3000]
    assert votes(kmer_set([long_walk]), long_walk)[0] == len(range(0, 3000 - 11, 12)) == 250
