"""CPU: the contract of the windowed layer rebuild as tests/layer_window_rule.py states it, against the oracle and against the header.

On a graph with ONE path the rebuilt values are linear-gap Needleman-Wunsch of the read against the path, so the rule's sources,
walked to the end, must give the oracle's CIGAR (M4_ABS / M5_ABS) and its score:
  * with a window as wide as the row nothing is ever unknown: no read falls back, every walk is the oracle's;
  * with W = 128 and 256, on the read families of the GPU test (tests/test_gpu_layer_window_walks.py): wherever the rule says "no
    fallback" its windowed walk is the oracle's again, and a walk of the oracle's that leaves the window (walk_leaves_window: no DP)
    implies a fallback;
  * every (n, W) holds reads of both kinds, and walks that wander a quarter of the window without falling back;
  * layer_window_left restated equals the one of rg_layer_window.hpp."""
import os
import subprocess

import numpy as np
import pytest

import layer_window_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recgraph_amd", "csrc")


def _score_sets(oracle):
    return (("2/-4", oracle.scores_match_mis(2, -4)), ("3/-5", oracle.scores_match_mis(3, -5)))


def _indel_read(rng, p):
    """A read of 30 .. 300 bases: a piece of the path with a few indels of 1 .. 20 bases."""
    n = int(rng.integers(30, 301))
    s = p[:n + 40]
    events, at = [], int(rng.integers(5, 30))
    while at + 25 < len(s):
        k = int(rng.integers(1, 21))
        events.append((at, k if rng.random() < 0.5 else -k))
        at += k + int(rng.integers(20, 120))
    return R.apply_events(s, events, rng)[:300]


@pytest.mark.parametrize("seg", [1, 23])
def test_a_window_as_wide_as_the_row_never_falls_back(oracle, seg):
    rng = np.random.default_rng(40 + seg)
    p = R.rand_bases(rng, 280)
    og = oracle.Graph.from_gfa_text(R.one_path_gfa(p, seg))
    reads = [_indel_read(rng, p) for _ in range(20)] + ["A", p, R.rand_bases(rng, 150)]
    for name, scores in _score_sets(oracle):
        for semi, omode in ((False, oracle.M4_ABS), (True, oracle.M5_ABS)):
            for rd in reads:
                wpad = 64 * R.columns_per_lane(len(rd))
                text, score = og.align(omode, rd, scores=scores)[:2]
                for W in (wpad, 2 * wpad):
                    m = R.Model(p, rd, scores, W, semi)
                    falls_back, why, _, ops = m.verdict()
                    assert not falls_back, (name, semi, len(rd), W, why)
                    assert ops == R.cigar_ops(text), (name, semi, len(rd), W)
                    assert m.score == score, (name, semi, len(rd), m.score, score)


def _against_the_oracle(oracle, scores, family, n, W, seg):
    for path, reads, semi in R.family_reads(family, n, W):
        wpad = R.batch_wpad(reads)
        assert wpad == 64 * R.columns_per_lane(n), (family, n, W, sorted(map(len, reads)))       # the shape the case is named for
        assert abs(len(path) - n) <= 150 + (120 if semi else 0) and len(reads) <= 12             # (semi: 60 more bases at either end)
        og = oracle.Graph.from_gfa_text(R.one_path_gfa(path, seg))
        for i, rd in enumerate(reads):
            r = R.analyse(path, rd, scores, W, semi, wpad)
            text, score = og.align(oracle.M5_ABS if semi else oracle.M4_ABS, rd, scores=scores)[:2]
            want = R.cigar_ops(text)
            assert r["score"] == score and r["true_ops"] == want, (family, i)
            if not r["falls_back"]:
                assert r["ops"] == want, (family, i)
            if R.walk_leaves_window(want, r["t_start"], len(rd), W, wpad):
                assert r["falls_back"], (family, i, "the oracle's walk leaves the window")
            assert r["excursion"] == R.walk_excursion(want, r["t_start"], len(rd), W, wpad)


@pytest.mark.parametrize("family", R.FAMILIES + ("semi",))
@pytest.mark.parametrize("n,W", R.SHAPES)
def test_no_fallback_means_the_oracles_walk(oracle, n, W, family):
    _against_the_oracle(oracle, oracle.scores_match_mis(2, -4), family, n, W, 9)


@pytest.mark.parametrize("n,W", R.SHAPES)
def test_every_shape_holds_both_kinds_of_read(oracle, n, W):
    """Per (n, W), over the global families: at least two reads that fall back, four that do not, two of those with a walk a quarter
    of the window off its diagonal."""
    fb, ok, wide = R.shape_census(oracle.scores_match_mis(2, -4), n, W)
    print("n %d, W %d: %d reads fall back, %d do not, %d of those wander >= W / 4" % (n, W, fb, ok, wide))
    assert fb >= 2 and ok >= 4 and wide >= 2, (n, W, fb, ok, wide)


@pytest.mark.parametrize("family", ["drift_del", "drift_ins", "lane_wrap", "semi"])
def test_the_second_score_matrix_walks_the_same_way(oracle, family):
    """create_score_matrix_i32(3, -5), one segment per base, on the smallest shape with a whole window."""
    _against_the_oracle(oracle, oracle.scores_match_mis(3, -5), family, 300, 128, 1)


@pytest.mark.parametrize("n,W", R.SHAPES)
def test_a_known_left_edge_neighbour_changes_a_verdict(oracle, n, W):
    """The families bite at the window's left edge: a rule that lets the column left of the window count as known (Model's
    `edge_known`, which is NOT the contract) keeps a read that the contract sends to the full-width kernels, in every (n, W) —
    a kernel whose edge lane read its neighbour instead of the sentinel would miss the exact counts of the GPU test."""
    scores = oracle.scores_match_mis(2, -4)
    for family in ("drift_ins", "staircase", "lane_wrap", "clamp_end", "clamp_start", "drift_del", "excursion"):
        for path, reads, semi in R.family_reads(family, n, W):
            wpad = R.batch_wpad(reads)
            for rd in reads:
                if R.window_verdict(path, rd, scores, W, semi, wpad)[0] and not R.Model(path, rd, scores, W, semi, wpad, edge_known=True).verdict()[0]:
                    return
    assert False, (n, W)


_TABLE_CPP = r"""
#include <cstdio>
#include <initializer_list>
#include "layer_window/rg_layer_window.hpp"
int main() {
    const int ns[] = {1, 63, 255, 256, 1000, 1023};
    for (int n : ns) {
        int C = 4;
        while (C * 64 < n + 1) C *= 2;
        for (int W : {rg::LAYER_WINDOW_NARROW, rg::LAYER_WINDOW_DEFAULT})
            for (int sc = 0; sc <= n; sc += (sc < n && sc + 37 > n) ? n - sc : 37)
                for (int ts : {1, 2, n / 2 + 1, n, n + 70})
                    for (int t = 0; t <= ts; t += (t < ts && t + 29 > ts) ? ts - t : 29)
                        printf("%d %d %d %d %d %d\n", n, W, sc, ts, t, rg::layer_window_left(sc, ts, t, W, C * 64));
    }
    return 0;
}
"""


def test_the_restated_window_function_is_the_headers(tmp_path):
    """On the grid of tests/c/layer_window_check.cpp (its read lengths, both widths; start cells and rows sampled, the last of each
    included): a table printed by a stand-alone program built from the header."""
    src = tmp_path / "window_table.cpp"
    src.write_text(_TABLE_CPP)
    exe = tmp_path / "window_table"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [tuple(map(int, ln.split())) for ln in r.stdout.splitlines()]
    assert len(rows) > 10000
    seen = set()
    for n, W, sc, ts, t, left in rows:
        wpad = 64 * R.columns_per_lane(n)
        assert R.layer_window_left(sc, ts, t, W, wpad) == left, (n, W, sc, ts, t, left)
        seen.add((n, W, sc == n, t == ts))
    for n in (1, 63, 255, 256, 1000, 1023):
        for W in (128, 256):
            assert (n, W, True, True) in seen and (n, W, False, False) in seen, (n, W)      # the last start cell and the last row too
