"""GPU: every instantiation of the local gap kernels (tests/kernel_matrix_gap_local.py) ran and was right.

One test per entry: the entry's case is aligned with the launch log on, every read is checked against the rule (check_batch of
tests/test_gpu_pathwise_gap_local.py: whole line, re-scored CIGAR, status), and EVERY batch of the case — one per boundary length —
must have launched the entry's instantiation.  Cases that several entries share run once."""
import pytest

import kernel_matrix_gap_local as KL
from test_gpu_pathwise_gap_local import check_batch

pytestmark = pytest.mark.gpu
_RESULTS = {}


def _run_case(cid):
    if cid in _RESULTS:
        return _RESULTS[cid]
    from recgraph_amd import api
    case = KL.CASES[cid]
    g, batches = KL.build(case)
    gg = api.Graph.from_gfa_text(g.gfa())
    per_batch, coarse = [], set()
    try:
        api.set_option("launch_log", 1)
        for reads in batches:
            b = api.Batch(gg, reads, api.make_params(case.mode, **case.kw))
            b.run()
            b.fetch()
            status = [b.status(i) for i in range(len(reads))]
            assert status == [0] * len(reads), cid
            texts = [b.gaf_text(i, "r%d" % i, i + 1) for i in range(len(reads))]
            stats = b.kernel_stats()
            per_batch.append({k[5:]: v[1] for k, v in stats.items() if k.startswith("inst:")})
            coarse |= {k for k in stats if not k.startswith("inst:")}
            api.set_option("launch_log", 0)
            check_batch(g.gfa(), reads, texts=texts, status=status, **case.kw)
            api.set_option("launch_log", 1)
            # the flanked read is clipped on both sides; a whole path ends on its last column
            f = texts[0].split("\t")
            assert int(f[2]) > 0 and int(f[3]) < len(reads[0]) - 1, (cid, f[:4])
    finally:
        api.set_option("launch_log", 0)
    _RESULTS[cid] = (per_batch, coarse)
    return _RESULTS[cid]


@pytest.mark.parametrize("name", sorted(KL.MATRIX))
def test_instantiation_ran_and_matched_the_rule(name):
    cid = KL.MATRIX[name]
    per_batch, coarse = _run_case(cid)
    assert len(per_batch) == len(KL.CASES[cid].batches)
    for b in per_batch:
        assert b.get(name, 0) >= 1, (name, cid, sorted(b.items()))
        # nothing but the local gap kernels of this C
        assert len(b) == 4 and all("k_gap_" in k and "_local" in k for k in b), sorted(b)
    assert {"k_gap_score_local", "k_gap_pick_local", "k_gap_dirs_local", "k_gap_trace_local"} <= coarse
