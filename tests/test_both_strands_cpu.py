"""CPU: the interface of RG_AMB_BOTH_STRANDS (both strands inside a pathwise batch) without a device — the constant in the
header, the ctypes binding and the Python API agree, the CLI knows `--both-strands` and refuses it for modes 0-3, the
parameter checks of rg_batch_create answer before any device is needed, the new path has no CPU fallback, and the three
kernels of rg_strand.hip stay small (no scratch, at most 64 VGPRs, no wide store with a VALU write behind it)."""
import os
import re
import sys

import pytest

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
    m = re.search(r"^#define RG_AMB_BOTH_STRANDS (\d+)$", hdr, re.M)
    assert m and int(m.group(1)) == 4 == _lib.AMB_BOTH_STRANDS == api.AMB_BOTH_STRANDS
    assert api.make_params(api.MODE_RECOMBINATION, amb=api.AMB_BOTH_STRANDS).amb_mode == 4
    assert api.make_params(api.MODE_RECOMBINATION).amb_mode == 0
    # the Rust shim carries the header's defines
    ffi = open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    assert re.search(r"RG_AMB_BOTH_STRANDS\b.*=\s*4\s*;", ffi)
    # the library keeps its 63 symbols: the feature is a parameter bit, not an entry point
    assert len(_lib.SYMBOLS) == 63
    import inspect
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream, api.Stream.__init__):
        assert inspect.signature(fn).parameters["both_strands"].default is False, fn


def test_cli_flag():
    from recgraph_amd import cli
    p = cli.build_parser()
    assert p.parse_args(["r.fa", "g.gfa", "-m", "8"]).both_strands is False
    assert p.parse_args(["r.fa", "g.gfa", "-m", "8", "--both-strands"]).both_strands is True
    for m in ("0", "1", "2", "3"):
        with pytest.raises(SystemExit) as ex:        # refused before the graph file is even opened
            cli.main(["no_such_reads.fa", "no_such_graph.gfa", "-m", m, "--both-strands"])
        assert "--both-strands" in str(ex.value) and "-s true" in str(ex.value)


def test_refusals_need_no_device_and_the_path_has_no_cpu_fallback(rg, example_gfa):
    from recgraph_amd import _lib, api
    g = api.Graph.from_gfa_text(example_gfa)
    rd = ["ACGTACGTAC", "TTGACCA"]
    # bit 2 with a POA mode, bits 0 / 1 with a pathwise mode, an undefined bit: RG_ERR_ARG
    for mode, amb in ((api.MODE_GLOBAL_POA, 4), (api.MODE_GAP_LOCAL_POA, 7), (api.MODE_RECOMBINATION, 5), (api.MODE_PATHWISE, 2),
                      (api.MODE_RECOMBINATION_SEMI, 8)):
        with pytest.raises(_lib.RecGraphError) as e:
            api.Batch(g, rd, api.make_params(mode, amb=amb))
        assert e.value.code == -1, (mode, amb)
    with pytest.raises(_lib.RecGraphError) as e:
        api.Batch(g, rd, api.make_params(api.MODE_GLOBAL_POA, amb=4))
    assert "rg_stream_opts.amb_strand" in str(e.value) and "-s true" in str(e.value)
    # the Python keyword is refused for the POA modes before the library is asked
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
        with pytest.raises(_lib.RecGraphError) as e:
            fn(g, rd, None, mode=api.MODE_GAP_POA, both_strands=True)
        assert e.value.code == -1 and "-s true" in str(e.value)
    if _lib.load().rg_device_count() > 0:
        texts, status = api.align_batch(g, rd, None, mode=api.MODE_PATHWISE, both_strands=True)
        assert len(texts) == 2 and not any(status)
        return
    for fn in (api.align_batch, api.align_batch_multi, api.align_stream):
        with pytest.raises(_lib.RecGraphError) as e:
            fn(g, rd, None, mode=api.MODE_RECOMBINATION, both_strands=True)
        assert e.value.code == -3, fn


def test_strand_kernels_are_small():
    """They run beside the sweeps of the other handles, which leave 64 VGPRs per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = {k["name"].split("(")[0]: k for k in kernel_resources.report("rg_strand.hip")}
    assert set(ks) == {"rg::k_strand_gate", "rg::k_revcomp", "rg::k_strand_merge"}, sorted(ks)
    for name, k in ks.items():
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["VGPRs"] <= 64, (name, k)
    hits, stores = kernel_resources.store_hazards("rg_strand.hip")
    assert not hits, hits[:4]


def test_synth_reverse_complements_a_share_of_a_read_set():
    from recgraph_amd import api, synth
    sg = synth.haplotype_graph(300, 4, path_len=100, seed=3)
    rd = synth.haplotype_reads(sg, 40, 100, seed=4)
    out, flipped = synth.reverse_complement_share(rd, 0.5, seed=9)
    assert len(out) == 40 and len(flipped) == 40 and flipped.sum() == 20
    for a, b, f in zip(rd, out, flipped):
        assert b == (api.rev_and_compl(a) if f else a)
    again, flipped2 = synth.reverse_complement_share(rd, 0.5, seed=9)
    assert again == out and (flipped2 == flipped).all()
    assert synth.reverse_complement_share(rd, 0.0)[0] == rd
    assert synth.reverse_complement_share(rd, 1.0)[1].all()
