"""GPU: the parts of the C ABI a non-Python caller relies on — structured GAFStruct fields (no text parsing), the
multi-device call, handle re-use with new reads."""
import pytest

pytestmark = pytest.mark.gpu

MODES = ("MODE_GLOBAL_POA", "MODE_GLOBAL_POA_SCALAR", "MODE_GAP_POA", "MODE_LOCAL_POA", "MODE_GAP_LOCAL_POA", "MODE_PATHWISE",
         "MODE_PATHWISE_SEMI", "MODE_RECOMBINATION", "MODE_RECOMBINATION_SEMI")


def test_result_fields_rebuild_the_gaf_line(example_gfa, example_reads):
    """rg_result_fields carries every field of the reference's GAFStruct (gaf_output.rs:6-20): GAFStruct::to_string
    over them is the record line rg_result_gaf prints, in every mode, including the empty record of a band failure."""
    from recgraph_amd import api, synth
    names, reads = example_reads
    g = api.Graph.from_gfa_text(example_gfa)
    seen_empty = seen_warning = False
    for mname in MODES:
        b = api.Batch(g, reads, api.make_params(getattr(api, mname)))
        b.run()
        b.fetch()
        for i in range(len(reads)):
            text = b.gaf_text(i, names[i], i + 1)
            f = b.fields(i, names[i])
            assert f is not None and f.to_string() + "\n" == text.split("\n", text.count("\n") - 1)[-1], (mname, i)
            seen_empty |= f.to_string() == api.GAFStruct().to_string()
    # a band failure (GAFStruct::new()) and a band warning, on a long linear-ish graph with short reads
    sg = synth.linear_graph(1500, seed=9)
    rd = synth.substring_reads(sg, 60, 80, seed=10)
    g2 = api.Graph.from_gfa_text(sg.gfa())
    for mode in (api.MODE_GLOBAL_POA, api.MODE_GAP_POA):
        b = api.Batch(g2, rd, api.make_params(mode, b=1.0, f=0.0))
        b.run()
        b.fetch()
        for i in range(len(rd)):
            text = b.gaf_text(i, "q", i + 1)
            f = b.fields(i, "q")
            lines = text.split("\n")[:-1]
            assert f.to_string() == lines[-1]
            seen_empty |= f.to_string() == api.GAFStruct().to_string()
            seen_warning |= len(lines) > 1
    assert seen_empty and seen_warning


def test_multi_device_call_equals_one_batch(oracle):
    """rg_align_batch_multi: the streaming engine behind one call — tiles of contiguous reads (at least one per entry of
    device_ids) pulled by the batch handles of every listed device, text in input order.  One GPU here: the device list
    names it several times (its handles then share the device and its graph tables)."""
    from recgraph_amd import api, synth
    sg = synth.haplotype_graph(1500, 8, path_len=300, seed=11)
    reads = synth.haplotype_reads(sg, 37, length=300, seed=12, mosaic_frac=0.5)
    names = ["q%d" % i for i in range(len(reads))]
    g = api.Graph.from_gfa_text(sg.gfa())
    for mode in (api.MODE_RECOMBINATION, api.MODE_PATHWISE, api.MODE_GLOBAL_POA, api.MODE_GAP_POA):
        one, _ = api.align_batch(g, reads, names, mode=mode)
        for devs in ([0], [0, 0, 0], None):
            m = api.MultiBatch(g, reads, api.make_params(mode), device_ids=devs)
            assert m.begin[0] == 0 and m.begin[-1] == len(reads) and len(m.shards) >= (len(devs) if devs else 1)
            assert m.begin == sorted(m.begin) and sum(sh.n for sh in m.shards) == len(reads)
            assert m.format_all(names, 1, 4).decode() == "".join(one), (mode, devs)
            sh, j = m.locate(20)
            assert sh.gaf_text(j, names[20], 21) == one[20]
    og = oracle.Graph.from_gfa_text(sg.gfa())
    assert one[5] == og.align(oracle.M2, reads[5], name=names[5], idx=6)[0]
    with pytest.raises(Exception):
        api.MultiBatch(g, reads, api.make_params(api.MODE_PATHWISE), device_ids=[0, 99])    # no such device: status code


def test_handle_reuse_with_new_reads(oracle):
    """rg_batch_set_reads: one handle, several read sets of different sizes and lengths; same records as fresh handles."""
    from recgraph_amd import api, synth
    sg = synth.haplotype_graph(1500, 8, path_len=300, seed=11)
    g = api.Graph.from_gfa_text(sg.gfa())
    sets = [synth.haplotype_reads(sg, n, length=ln, seed=s, mosaic_frac=0.5) for n, ln, s in ((20, 300, 1), (45, 120, 2), (7, 330, 3), (20, 300, 1))]
    for mode in (api.MODE_RECOMBINATION, api.MODE_GLOBAL_POA, api.MODE_GAP_POA, api.MODE_LOCAL_POA):
        b = api.Batch(g, sets[0], api.make_params(mode))
        for k, rs in enumerate(sets):
            if k:
                b.set_reads(rs)
            b.run()
            b.fetch()
            fresh, _ = api.align_batch(g, rs, None, mode=mode)
            assert [b.gaf_text(i, "read%d" % i, i + 1) for i in range(len(rs))] == fresh, (mode, k)


def test_one_handle_run_twice():
    """rg_batch_run resets the handle's statistics and its event cursor: a second run() of the same reads reports the same
    kernel names and launch counts as the first (nothing accumulates, no name twice) and the same records as a fresh handle.
    The pathwise case takes both strands with the vote: its vote kernels are recorded in front of pass A and collected with it."""
    from recgraph_amd import api, synth
    from strand_vote_rule import rc
    sg = synth.haplotype_graph(600, 6, path_len=200, seed=31)
    g = api.Graph.from_gfa_text(sg.gfa())
    good = synth.haplotype_reads(sg, 12, 200, seed=5, mosaic_frac=0.5)
    reads = [rc(r) if i % 3 == 0 else r for i, r in enumerate(good)] + ["ACGT" * 30]       # (the palindrome reaches pass B)
    lib = api._lib.load()
    for mode, amb in ((api.MODE_GAP_POA, None), (api.MODE_RECOMBINATION, api.AMB_BOTH_STRANDS | api.AMB_STRAND_VOTE)):
        seen = []
        for handle in range(2):
            b = api.Batch(g, reads, api.make_params(mode, amb=amb))
            for run in range(2 if handle == 0 else 1):
                b.run()
                b.fetch()
                names = [lib.rg_batch_kernel_name(b._h, k).decode() for k in range(lib.rg_batch_kernel_count(b._h))]
                assert len(names) == len(set(names)), names
                seen.append(({k: v[1] for k, v in b.kernel_stats().items()}, [b.gaf_text(i, "q%d" % i, i + 1) for i in range(len(reads))]))
        assert seen[0] == seen[1] == seen[2], (mode, [s[0] for s in seen])
        assert all(n >= 1 for n in seen[0][0].values())
        if amb:
            assert {"k_strand_vote", "k_strand_orient", "k_strand_gate", "k_strand_merge", "mem:work_bytes_per_read"} <= set(seen[0][0])
            assert any("\t-\t" in t for t in seen[0][1]) and any("\t+\t" in t for t in seen[0][1])
