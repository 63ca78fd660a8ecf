"""The shared POA walkers and scan steps (csrc/rg_poa_common.hpp) against the oracle: whole output text byte for byte.

One graph of 68 rows with one bubble.  Affine runs (-m 2 / -m 3 with a cheap extension: X and Y runs of two and more ops), the
band edge (-m 2 and scalar -m 0 in a band too narrow for some reads: band_ampl_enough and the j_pos translation), local start and
stop (-m 1 in both flavours and -m 3 on reads with unrelated ends).  Every case also holds the DP cell counter to the oracle's."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEGS = ("ACGTTGCAAGGCTTACCGATAGGCTA", "GATTACAG", "CTGGCATC", "TTGACCGGATCAGTTCAAGGTACC")
GFA = "".join("S\t%d\t%s\n" % (i + 1, s) for i, s in enumerate(SEGS)) + "".join("L\t%d\t+\t%d\t+\t0M\n" % l for l in ((1, 2), (1, 3), (2, 4), (3, 4)))
PATHS = (SEGS[0] + SEGS[1] + SEGS[3], SEGS[0] + SEGS[2] + SEGS[3])
AFFINE = {"o": -10, "e": -1}
WIDE = {"b": 100.0, "f": 0.0}        # -m 2: no read meets the band
NARROW = {"b": 2.0, "f": 0.0}        # 12 (-m 2) / 10 (scalar -m 0) of the 16 reads meet it, the others do not
SEED = 5


def _junk(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def indel_reads(seed=SEED):
    """16 reads of 40 to 80 bases: a path cut or continued to that length, one 3-base insertion, one 3-base deletion."""
    rng = np.random.default_rng(seed)
    reads = []
    for k in range(16):
        n = 40 + (k * 40) // 15
        s = list((PATHS[k % 2] + _junk(rng, 25))[:n])
        a = int(rng.integers(5, 18))
        b = int(rng.integers(22, 35))
        del s[a:a + 3]
        s[b:b] = list(_junk(rng, 3))
        reads.append("".join(s))
    return reads


def flanked_reads(seed=SEED):
    """Path substrings between 10 unrelated bases on either side (homopolymers the graph does not hold)."""
    rng = np.random.default_rng(seed + 1)
    reads = []
    for k in range(12):
        a = int(rng.integers(0, 20))
        core = PATHS[k % 2][a:a + 25 + 2 * k]
        reads.append("A" * 10 + core + ("T" * 10 if k % 2 else "G" * 10))
    return reads


def long_runs(texts):
    """reads whose CIGAR has an I run and a D run of two and more"""
    n = 0
    for t in texts:
        runs = re.findall(r"(\d+)([IDMX=])", t.split("\t")[-1])
        n += any(c == "I" and int(k) >= 2 for k, c in runs) and any(c == "D" and int(k) >= 2 for k, c in runs)
    return n


def _modes(oracle):
    from recgraph_amd import api
    return {"m2": (api.MODE_GAP_POA, oracle.M2), "m0s": (api.MODE_GLOBAL_POA_SCALAR, oracle.M0_SCALAR), "m1": (api.MODE_LOCAL_POA, oracle.M1_SIMD),
            "m1s": (api.MODE_LOCAL_POA_SCALAR, oracle.M1_SCALAR), "m3": (api.MODE_GAP_LOCAL_POA, oracle.M3)}


def oracle_run(oracle, omode, reads, kw):
    og = oracle.Graph.from_gfa_text(GFA, want_path=False)
    return [og.align(omode, rd, name="r%d" % i, idx=i + 1, **kw) for i, rd in enumerate(reads)]


def _check(oracle, key, reads, kw):
    """texts of the oracle; the batch's texts, panic bits and cell counters equal them"""
    from recgraph_amd import api
    mode, omode = _modes(oracle)[key]
    exp = oracle_run(oracle, omode, reads, kw)
    b = api.Batch(api.Graph.from_gfa_text(GFA), reads, api.make_params(mode, **kw))
    b.run()
    b.fetch()
    for i, (text, score, panic, _) in enumerate(exp):
        if panic:
            assert b.status(i) & api.READ_WOULD_PANIC, (key, i)
        else:
            assert b.gaf_text(i, "r%d" % i, i + 1) == text, (key, i, reads[i])
    cells = sum(e[3] for e in exp)
    print(key, kw, "cells: device %d performed %d oracle %d" % (b.cell_updates, b.cell_updates_performed, cells))
    assert b.cell_updates == b.cell_updates_performed == cells, (key, b.cell_updates, b.cell_updates_performed, cells)
    return [e[0] for e in exp if not e[2]]


@pytest.mark.parametrize("key", ["m2", "m3"])
def test_affine_runs(oracle, key):
    reads = indel_reads()
    texts = _check(oracle, key, reads, dict(AFFINE, **(WIDE if key == "m2" else {})))
    assert long_runs(texts) >= len(reads) // 2, long_runs(texts)


@pytest.mark.parametrize("key", ["m2", "m0s"])
def test_band_edge(oracle, key):
    kw = dict(NARROW, **(AFFINE if key == "m2" else {}))
    texts = _check(oracle, key, indel_reads(), kw)
    short = sum("Band length probably too short" in t for t in texts)
    assert 1 <= short < len(texts), (short, len(texts))


@pytest.mark.parametrize("key", ["m1", "m1s", "m3"])
def test_local_start_and_stop(oracle, key):
    reads = flanked_reads()
    texts = _check(oracle, key, reads, AFFINE if key == "m3" else {})
    # the alignment starts and stops inside the read (GAF columns 3 and 4): the walk ends at an 'O' cell, not at the border
    for rd, t in zip(reads, texts):
        f = t.strip().split("\n")[-1].split("\t")
        assert 0 < int(f[2]) < int(f[3]) < len(rd), (rd, f[:4])
