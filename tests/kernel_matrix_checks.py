"""The two checks every kernel matrix of the pathwise families (tests/kernel_matrix_gap*.py, tests/kernel_matrix_edit.py) gets: on
the CPU, that its key set is exactly what hipcc compiles from the family's one .hip; on the GPU, one case run with the launch log on
and every read checked.  What a family asserts about its own kernel set stays in its test file.  A plain module: every assert carries
its own message."""
import os

from pathwise_support import ROOT, check_mode, graph_tuple, kernel_resources, run_batch


def assert_matrix_is_complete(K, src, count):
    """K.MATRIX names exactly the `count` `__global__` instantiations compiled from csrc/`src`, and the directory of `src` holds no
    other .hip (a kernel there would have no matrix)."""
    d = os.path.join(ROOT, "recgraph_amd", "csrc", os.path.dirname(src))
    hips = sorted(f for f in os.listdir(d) if f.endswith(".hip"))
    assert hips == [os.path.basename(src)], (d, hips)
    names = [k["name"] for k in kernel_resources().report(src)]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    compiled, keys = set(names), set(K.MATRIX)
    assert compiled == keys, {"compiled without an entry": sorted(compiled - keys), "entries without a kernel": sorted(keys - compiled)}
    assert len(compiled) == count, (src, len(compiled), count)


def batch_of_case(gg, reads, case):
    return run_batch(gg, reads, case.mode, **case.kw)


def check_case(graph, reads, case, run):
    check_mode(graph, reads, case.mode, texts=run.texts, status=run.status, **case.kw)


def run_case(K, cid, results, align=batch_of_case, check=check_case):
    """One case of the kernel matrix K, cached in `results`: every batch is run by align(api.Graph, reads, case) -> pathwise_support.Run
    with the launch log on, must have status 0 for every read, and is handed to check(graph_tuple, reads, case, run) with the log
    off again (the checker's own batches are not the case's).  Returns (the instantiations each batch launched, the coarse kernel
    names of all batches)."""
    if cid in results:
        return results[cid]
    from recgraph_amd import api
    case = K.CASES[cid]
    g, batches = K.build(case)
    graph = graph_tuple(g)
    per_batch, coarse = [], set()
    try:
        for reads in batches:
            api.set_option("launch_log", 1)
            run = align(graph[1], reads, case)
            api.set_option("launch_log", 0)
            assert run.status == [0] * len(reads), (cid, run.status)
            per_batch.append(run.instantiations)
            coarse |= run.kernels
            check(graph, reads, case, run)
    finally:
        api.set_option("launch_log", 0)
    results[cid] = (per_batch, coarse)
    return results[cid]
