"""GPU: every reachable kernel instantiation ran and was right.

One test per entry of tests/kernel_matrix.py: the entry's case is aligned with the launch log on (rg_set_option
"launch_log": every launcher reports the instantiation it dispatched as an "inst:<name>" pseudo-entry of kernel_stats()),
every read's text must equal the oracle's byte for byte, and the entry's instantiation must be among the launched ones —
twice for the sweeps of -m 8 / -m 9 (forward and reverse).  Cases that several entries share run once.  The last test asserts
that the union of everything the run launched is exactly the reachable key set of the matrix."""
import pytest

import kernel_matrix as KM

pytestmark = pytest.mark.gpu

_RESULTS = {}          # case id -> {"inst:" name: launches} of its batches (the stream's under "stream")
_LAUNCHED = set()      # every instantiation any case of this module launched
DEFAULTS = {"spec_margin": 112, "retire_shift": 8}


def _run_batch(api, gg, case, reads, sc):
    amb = (api.AMB_BOTH_STRANDS | api.AMB_STRAND_VOTE) if case.strands else None
    b = api.Batch(gg, reads, api.make_params(case.mode, score_matrix=sc, amb=amb, **case.kw))
    b.run()
    b.fetch()
    texts = [b.gaf_text(i, "r%d" % i, i + 1) for i in range(len(reads))]
    stats = b.kernel_stats()
    return texts, [b.status(i) for i in range(len(reads))], stats


def _expected(oracle, case, gfa, reads):
    if not case.strands:
        exp = KM.oracle_texts(oracle, case, gfa, reads)
        assert not any(p for _, p in exp)
        return [t for t, _ in exp]
    from strand_vote_rule import expected_strand_vote, gfa_paths, kmer_set
    og = oracle.Graph.from_gfa_text(gfa)
    exp = expected_strand_vote(og, KM.oracle_mode(oracle, case.mode), kmer_set(gfa_paths(gfa)), reads, prefix="r")
    assert any(e[1] for e in exp) and any(e[2] for e in exp)         # some read goes reverse first, some is aligned on both strands
    return [e[0] for e in exp]


def _run_case(oracle, cid):
    """Aligns the case once (launch log on, its switches set, everything restored afterwards) and checks every read."""
    if cid in _RESULTS:
        return _RESULTS[cid]
    from recgraph_amd import api
    case = KM.CASES[cid]
    g, batches = KM.build(case)
    gfa = g.gfa()
    sc = KM.scores_table(case, oracle.scores_match_mis(3, -5))
    expected = [_expected(oracle, case, gfa, reads) for reads in batches]
    seen, stream_seen, coarse, per_batch = {}, {}, set(), []
    try:
        api.set_option("launch_log", 1)
        for name, val in case.options.items():
            api.set_option(name, val)
        gg = api.Graph.from_gfa_text(gfa)
        for reads, exp in zip(batches, expected):
            texts, status, stats = _run_batch(api, gg, case, reads, sc)
            bad = [(i, len(reads[i]), texts[i][-300:], exp[i][-300:]) for i in range(len(reads)) if texts[i] != exp[i]]
            # (a status may carry the band warnings of the POA modes: the reference prints them, so they are in the text that was
            # just compared — a 16 001-base read against 1 200 rows gets "Band length probably too short"; no read may be refused)
            errors = [x & (api.READ_WOULD_PANIC | api.READ_BAD_BASE) for x in status]
            assert not bad and not any(errors), (cid, len(bad), bad[:2], status)
            assert [bool(x & api.READ_BAND_WARNING) for x in status] == ["Band length probably too short" in t for t in texts], (cid, status)
            per_batch.append({k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")})
            for k, (ms, launches) in stats.items():
                if k.startswith("inst:"):
                    assert ms == 0 and launches >= 1, (k, ms, launches)
                    seen[k[5:]] = seen.get(k[5:], 0) + launches
                else:
                    coarse.add(k)
        if case.stream:
            # the same reads through the streaming engine in tiles of `stream` reads: the longest read of a TILE picks C
            reads, exp = batches[0], expected[0]
            st = api.Stream(gg, api.make_params(case.mode, score_matrix=sc, **case.kw), device_ids=[0], handles_per_device=2, tile_reads=case.stream)
            st.push(reads, ["r%d" % i for i in range(len(reads))])
            st.finish()
            texts = []
            for t in st:
                texts += [t.text_of(i).decode() for i in range(t.n)]
            stats = st.kernel_stats()
            st.close()
            assert texts == exp, cid
            stream_seen = {k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")}
    finally:
        api.set_option("launch_log", 0)
        for name in case.options:
            api.set_option(name, DEFAULTS.get(name, 0))
    _LAUNCHED.update(seen)
    _LAUNCHED.update(stream_seen)
    _RESULTS[cid] = (seen, stream_seen, coarse, per_batch)
    return _RESULTS[cid]


@pytest.mark.parametrize("name", KM.REACHABLE)
def test_instantiation_ran_and_matched_the_oracle(oracle, name):
    cid = KM.MATRIX[name]
    case = KM.CASES[cid]
    seen, stream_seen, coarse, per_batch = _run_case(oracle, cid)
    assert seen.get(name, 0) >= 1, (name, cid, sorted(seen))
    if "k_sweep" in name:
        # EVERY batch of the case (one per boundary length) ran this instantiation; -m 8 / -m 9 sweep forward and backward with it
        assert len(per_batch) == len(case.batches)
        for b in per_batch:
            assert b.get(name, 0) >= (2 if case.mode in (8, 9) else 1), (name, cid, sorted(b.items()))
        fam = "k_sweep16" if "k_sweep16" in name else "k_sweep"
        assert fam + "_fwd" in coarse and (case.mode not in (8, 9) or fam + "_rev" in coarse), sorted(coarse)
    if case.stream and name == KM.MATRIX_STREAM_KEYS.get(cid):
        assert stream_seen.get(name, 0) >= 1, (name, sorted(stream_seen))
        # ... and the tiles with shorter reads took a narrower instantiation of the same family than the batch did
        assert len({k for k in stream_seen if k.startswith(name.split("<")[0] + "<")}) >= 2, sorted(stream_seen)


def test_the_log_is_off_by_default(oracle):
    """No "inst:" entry without the option, and the same kernel names as with it."""
    from recgraph_amd import api
    case = KM.CASES["sweep16-C4-0rec-narrow-global"]
    g, batches = KM.build(case)
    gg = api.Graph.from_gfa_text(g.gfa())
    assert api._lib.load().rg_get_option(b"launch_log") == 0
    _, _, off = _run_batch(api, gg, case, batches[0], None)
    try:
        api.set_option("launch_log", 1)
        _, _, on = _run_batch(api, gg, case, batches[0], None)
    finally:
        api.set_option("launch_log", 0)
    assert not [k for k in off if k.startswith("inst:")]
    assert set(off) == {k for k in on if not k.startswith("inst:")} and any(k.startswith("inst:") for k in on)


def test_every_reachable_instantiation_was_launched(oracle):
    """The union over the whole matrix (cases not yet run by the parametrised test — a `-k` selection — run here)."""
    for cid in KM.CASES:
        _run_case(oracle, cid)
    assert _LAUNCHED == set(KM.REACHABLE), {"never launched": sorted(set(KM.REACHABLE) - _LAUNCHED), "launched without an entry": sorted(_LAUNCHED - set(KM.REACHABLE))}
