#!/usr/bin/env python3
"""Throughput OUTSIDE the headline's exact shape (VERDICT r4 "the headline is a point, not a region"): the same streaming
engine on other read lengths, score parameters and path counts, with the sweep kernel that ran and a parity check of a
few reads against the oracle.  One JSON line per case.

    python tools/region_bench.py [case ...]        cases: c5 x6 m3x5 hoxd70 len1500 p128 len600 gap gap_local gap_long gap_strands gap_xlong gap_xstrands edit edit_xlong edit_strands (default: all but the strand cases, the six `gap` cases and the three `edit` cases)

The strand cases (RG_AMB_BOTH_STRANDS, config-5 shape; `reads_per_s` counts SOURCE reads): `both_strands_fwd` — option on, every
read forward (what the option costs when nothing qualifies: compare with `c5`); `both_strands` — option on, half of the reads
reverse-complemented; `two_n` — option off, every read AND its reverse complement in the tiles, which is what a caller without
the option has to submit (half of a tile's reads are source reads).  `strand_vote_fwd` / `strand_vote` — the same two read sets
(the same seeds) with RG_AMB_STRAND_VOTE on top: the first strand by a 12-mer vote; their parity check builds the expected
text by that option's rule (include/recgraph_hip.h) from the oracle and the vote stated below.

`gap` (only when named): -m 6 beside -m 4 on the same inputs — the C4 / C5 graph shapes (16 paths on 5 000 rows, 32 on 10 000) with
reads of 150 and 1000 bases; one batch handle, timed over whole rg_batch_run calls after a warm-up run; a few reads of every
-m 6 batch are checked against the rule (tests/pathwise_gap_rule.py).  One JSON line per (shape, length, mode).

`gap_local` (only when named): -m 12 beside -m 7 on the same inputs in the same process — the shapes of `gap`, reads whose ends
are random overhangs (an eighth of the read on either side); both handles are warmed up, then timed over whole rg_batch_run calls in
alternating rounds (median and minimum per mode, and -m 12 as a ratio to -m 7); five reads of every -m 12 batch are checked against
the rule (tests/pathwise_gap_local_rule.py).  One JSON line per (shape, length).

`gap_long` (only when named): -m 16 at 4000 bases beside -m 6 at 2047 bases (the same reads, cut) on the same graph — 16 paths of
about 4000 rows — in the same process: both handles are warmed up, then timed over whole rg_batch_run calls in alternating rounds;
median and minimum per mode, the time per COUNTED cell update (rows_k * n per path and read) of both and their ratio, and the time of
every kernel.  Two reads of the -m 16 batch are checked against the rule (tests/pathwise_gap_rule.py): the printed score is the
rule's, and the printed CIGAR re-scores to it.  One JSON line.

`gap_strands` (only when named): -m 26 / 27 / 32 beside -m 16 / 17 / 22 OF THE SAME BUILD on the same reads, in one process, in
alternating rounds — the C4 shape (16 paths on 5 000 rows) at 150 and 1000 bases and one set of 4000-base reads on 16 paths of about
4000 rows.  Per set: (a) all-forward reads, -m 26 against -m 16 and -m 27 against -m 17 (the price of the gate, the reverse complement
and the eight-byte read-back); (b) half of the reads reverse-complemented (synth.reverse_complement_share, seed 5678): -m 26 by the
exact rule and by the vote rule, both relative to (a)'s -m 16; (c) -m 32 against -m 22 on the reads of (b).  Five reads of every
both-strands batch are checked against the composed rule (tests/pathwise_gap_strands_rule.py; at 4000 bases: strand, score and the
re-scored CIGAR of two reads).  One JSON line per set.

`gap_xlong` (only when named): the protocol of `gap_long` — one process, warm-up, alternating rounds, whole rg_batch_run calls, the
handle's kernel timer.  (a) -m 56 beside -m 16 OF THE SAME BUILD on the same 512 reads of 4000 bases and the 16-path graph of
4000-row paths of `gap_long`: the same bytes (compared), the time per counted cell update of both and their ratio, the work bytes per
read of both.  (b) one batch no earlier mode accepts: 32 reads of 50 000 bases on 16 paths of about 50 000 rows in -m 56 — time per
counted cell update, the work bytes per read beside what the layout of -m 16 would have needed.  Two reads of each part are checked
against the rule (tests/pathwise_gap_rule.py): the printed score is the rule's (part (b): the rule's score of the printed path), and
the printed CIGAR re-scores to it and consumes the read.  One JSON line per part.

`gap_xstrands` (only when named): -m 76 / 77 / 82 beside -m 56 / 57 / 62 OF THE SAME BUILD on the reads of `gap_xlong`'s two parts, in
one process, in alternating rounds: all-forward reads, and half of them reverse-complemented (synth.reverse_complement_share, seed
5678) under the exact rule and, in modes 76 and 77, under the vote.  Every ratio is relative to the as-given mode on the all-forward
reads; beside mode 82's stands the prediction (2 S + T) / (S + T) from this run's own kernel times of mode 62 (S: score pass and
pick, T: the traceback).  Every read of every both-strands batch is compared with the as-given mode's line of its source read and
with the flip; reads spread over the batch are checked against the numpy rules.  Two JSON lines per part (the first before the
rule check, which takes minutes at 50 000 bases); RG_REGION_PART=a or b runs one part.

`edit` (only when named): the bit-vector modes beside the affine-gap modes OF THE SAME BUILD at unit costs (match 0, mismatch -1, o = 0,
e = -1 on both sides), by the protocol of `gap_long` — one process, warm-up, alternating rounds, whole rg_batch_run calls, the handle's
kernel timer.  (a) -m 44 beside -m 16 on the 512 reads of 4000 bases and the 16-path graph of 4000-row paths of `gap_long`; (b), (c)
-m 44 beside -m 6 on 1000-base reads at the C4 / C5 graph shapes (16 paths on 5 000 rows, 32 on 10 000).  Per part: the same texts
(compared), time per batch, time per counted cell update, the time of every kernel, the score pass of -m 44 as a ratio to the other
mode's per counted cell, and the work bytes per read.  Two reads of each part are checked against the rule
(tests/pathwise_gap_rule.py at unit costs): the printed score is the rule's and the printed CIGAR re-scores to it.  One JSON line per part.

`edit_xlong` (only when named): -m 94 beside -m 56 OF THE SAME BUILD at unit costs on the shape of `gap_xlong`'s part (b) — 32 reads of
50 000 bases on 16 paths of about 50 000 rows — by the same protocol: one process, warm-up, alternating rounds, whole rg_batch_run calls,
the handle's kernel timer.  All texts, statuses and counted cells of the two modes are compared; per mode: time per batch, time per
counted cell update, performed over counted cells, the time of every kernel, the work bytes per read; and -m 94 as a ratio to -m 56.  One
JSON line.

`edit_strands` (only when named): -m 64 beside -m 26 OF THE SAME BUILD (the only other way to these bytes) and beside TWO -m 44 batches — the
reads as given, and the same reads reverse-complemented on the host: what a caller without the mode submits — at unit costs, by the same
protocol: one process, warm-up, alternating rounds, whole rg_batch_run calls, the handle's kernel timer.  Shapes (a) and (b) of `edit`;
half of the reads are reverse-complemented (synth.reverse_complement_share, seed 5678).  Texts, statuses and strands of -m 64 and -m 26
are compared; per mode: time per batch, the time of every kernel, the work bytes per read; and the ratios -m 64 / -m 26, k_edit_score_pair /
(the two k_edit_score), -m 64 / (the two -m 44 batches).  One JSON line per part; RG_REGION_PART=a or b runs one part.

Every case: TILES tiles of TILE reads through one rg_stream (3 handles), timed after one warm-up tile per handle."""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    # name: (mode, rows, paths, read length, score kwargs, tile reads, tiles)
    "c5": (8, 10000, 32, 1000, {}, 4096, 6),
    "x6": (8, 10000, 32, 1000, {"mm": (2, -6)}, 4096, 6),
    "m3x5": (8, 10000, 32, 1000, {"mm": (3, -5)}, 4096, 6),
    "hoxd70": (8, 10000, 32, 1000, {"mtx": "HOXD70.mtx"}, 2048, 4),
    "len1500": (8, 15000, 32, 1500, {}, 2048, 6),
    "len600": (8, 6000, 32, 600, {}, 4096, 6),
    "p128": (8, 10000, 128, 1000, {}, 2048, 6),
    "m4_len1500": (4, 15000, 32, 1500, {}, 2048, 6),
    "len5000": (8, 50000, 32, 5000, {}, 256, 4),
    "both_strands_fwd": (8, 10000, 32, 1000, {"strands": "on_fwd"}, 4096, 6),
    "both_strands": (8, 10000, 32, 1000, {"strands": "on_half"}, 4096, 6),
    "two_n": (8, 10000, 32, 1000, {"strands": "two_n"}, 4096, 12),
    "strand_vote_fwd": (8, 10000, 32, 1000, {"strands": "on_fwd", "vote": True}, 4096, 6),
    "strand_vote": (8, 10000, 32, 1000, {"strands": "on_half", "vote": True}, 4096, 6),
}


def vote_first_reverse(kmers, read):
    """RG_AMB_STRAND_VOTE, rule 1 and 2: up to 256 sampled 12-mers of the read and of its reverse complement against the paths'."""
    def count(s):
        npos = len(s) - 11
        step = -(-npos // 256) if npos > 0 else 1
        return sum(1 for q in range(0, max(npos, 0), step) if s[q:q + 12] in kmers)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    return count("".join(comp[c] for c in reversed(read))) > count(read)


def gap_case():
    from recgraph_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathwise_gap_rule as R
    runs = 3
    for shape, rows, paths in (("C4", 5000, 16), ("C5", 10000, 32)):
        for rlen, nreads in ((150, 4096), (1000, 2048)):
            g = synth.haplotype_graph(rows, paths, path_len=rlen, seed=1234)
            gg = api.Graph.from_gfa_text(g.gfa())
            reads = synth.haplotype_reads(g, nreads, length=rlen, seed=900, mosaic_frac=0.0)
            for mode in (api.MODE_PATHWISE_GAP, api.MODE_PATHWISE):
                b = api.Batch(gg, reads, api.make_params(mode))
                b.run()
                ks0 = b.kernel_stats()
                t0 = time.perf_counter()
                ks = {}
                for _ in range(runs):
                    b.run()
                    for k, v in b.kernel_stats().items():
                        if not k.startswith(("host:", "mem:", "inst:")):
                            ks[k] = ks.get(k, 0.0) + v[0] / runs
                dt = (time.perf_counter() - t0) / runs
                b.fetch()
                ok = True
                if mode == api.MODE_PATHWISE_GAP:
                    lnz, prow = R.graph_paths(gg)
                    for i in sorted({0, nreads - 1, nreads // 2, nreads // 3, 777 % nreads}):
                        ok = ok and "\t".join(b.gaf_text(i, "r", 1)[:-1].split("\t")[12:]) == R.comments(lnz, prow, reads[i])
                print(json.dumps({"case": "gap", "shape": shape, "mode": mode, "rows": gg.rows, "paths": paths, "read_len": rlen, "reads": nreads,
                                  "reads_per_s": round(nreads / dt, 1), "ms_per_batch": round(dt * 1e3, 2), "cell_updates_per_s": round(b.cell_updates / dt),
                                  "cell_updates_performed_per_s": round(b.cell_updates_performed / dt),
                                  "kernel_ms_per_batch": {k: round(v, 2) for k, v in ks.items()}, "first_run_kernels": sorted(k for k in ks0 if not k.startswith(("mem:", "inst:"))),
                                  "rule_checked": 5 if ok else "FAILED"}), flush=True)


def gap_local_case():
    import numpy as np
    from recgraph_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathwise_gap_local_rule as L
    rounds = 5
    for shape, rows, paths in (("C4", 5000, 16), ("C5", 10000, 32)):
        for rlen, nreads in ((150, 4096), (1000, 2048)):
            g = synth.haplotype_graph(rows, paths, path_len=rlen, seed=1234)
            gg = api.Graph.from_gfa_text(g.gfa())
            rng = np.random.default_rng(901)
            hang = rlen // 8

            def flank():
                return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=hang))
            reads = [flank() + r[hang:len(r) - hang] + flank() for r in synth.haplotype_reads(g, nreads, length=rlen, seed=900, mosaic_frac=0.0)]
            modes = (api.MODE_PATHWISE_GAP_LOCAL, api.MODE_PATHWISE_GAP_SEMI)
            batch = {m: api.Batch(gg, reads, api.make_params(m)) for m in modes}
            times = {m: [] for m in modes}
            ks = {m: {} for m in modes}
            for m in modes:
                batch[m].run()                       # warm-up: code objects, work buffers
            for _ in range(rounds):
                for m in modes:                      # alternating: both modes see the same machine
                    t0 = time.perf_counter()
                    batch[m].run()                   # (returns after the chunk's read-back: the device is idle again)
                    times[m].append(time.perf_counter() - t0)
                    for k, v in batch[m].kernel_stats().items():
                        if not k.startswith(("host:", "mem:", "inst:")):
                            ks[m][k] = ks[m].get(k, 0.0) + v[0] / rounds
            for m in modes:
                batch[m].fetch()
            b = batch[api.MODE_PATHWISE_GAP_LOCAL]
            lnz, prow = L.graph_paths(gg)
            ids = L.graph_node_ids(gg)
            ok = all(b.gaf_text(i, "r", 1) == L.line_local(lnz, prow, ids, "r", reads[i])
                     for i in sorted({0, nreads - 1, nreads // 2, nreads // 3, 777 % nreads}))
            clipped = sum(1 for i in range(nreads) if b.gaf_text(i, "r", 1).split("\t")[2:4] != ["0", str(rlen - 1)])
            med = {m: sorted(times[m])[rounds // 2] for m in modes}
            out = {"case": "gap_local", "shape": shape, "rows": gg.rows, "paths": paths, "read_len": rlen, "overhang": hang, "reads": nreads,
                   "rounds": rounds, "reads_clipped_by_m12": clipped, "unaligned": sum(1 for i in range(nreads) if b.status(i) & api.READ_UNALIGNED)}
            for m in modes:
                bm = batch[m]
                out["m%d" % m] = {"ms_per_batch_median": round(med[m] * 1e3, 2), "ms_per_batch_min": round(min(times[m]) * 1e3, 2),
                                  "reads_per_s": round(nreads / med[m], 1), "cell_updates_per_s": round(bm.cell_updates / med[m]),
                                  "performed_over_counted": round(bm.cell_updates_performed / bm.cell_updates, 3),
                                  "kernel_ms_per_batch": {k: round(v, 2) for k, v in ks[m].items()}}
            out["m12_over_m7_time_median"] = round(med[modes[0]] / med[modes[1]], 3)
            out["m12_over_m7_time_min"] = round(min(times[modes[0]]) / min(times[modes[1]]), 3)
            out["rule_checked"] = 5 if ok else "FAILED"
            print(json.dumps(out), flush=True)


def gap_long_case():
    from recgraph_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathwise_gap_rule as R
    rounds, paths, plen, nreads = 5, 16, 4000, 512
    g = synth.haplotype_graph(3 * plen, paths, path_len=plen, seed=1234)
    gg = api.Graph.from_gfa_text(g.gfa())
    long_reads = synth.haplotype_reads(g, nreads, length=plen, seed=900, mosaic_frac=0.0)
    reads = {api.MODE_PATHWISE_GAP_LONG: long_reads, api.MODE_PATHWISE_GAP: [r[:2047] for r in long_reads]}
    modes = tuple(reads)
    batch = {m: api.Batch(gg, reads[m], api.make_params(m)) for m in modes}
    times = {m: [] for m in modes}
    ks = {m: {} for m in modes}
    for m in modes:
        batch[m].run()                       # warm-up: code objects, work buffers
    for _ in range(rounds):
        for m in modes:                      # alternating: both modes see the same machine
            t0 = time.perf_counter()
            batch[m].run()                   # (returns after the chunk's read-back: the device is idle again)
            times[m].append(time.perf_counter() - t0)
            for k, v in batch[m].kernel_stats().items():
                if not k.startswith(("host:", "mem:", "inst:")):
                    ks[m][k] = ks[m].get(k, 0.0) + v[0] / rounds
    for m in modes:
        batch[m].fetch()
    b = batch[api.MODE_PATHWISE_GAP_LONG]
    lnz, prow = R.graph_paths(gg)
    ok = True
    for i in (0, nreads - 1):
        f = b.gaf_text(i, "r", 1)[:-1].split("\t")
        mm = re.fullmatch(r"([0-9MXID]+), best path: (\d+), score: (-?\d+)", f[12])
        last, lens = R.all_paths_last(lnz, prow, long_reads[i], R.default_scores(), -4, -2, False)
        best = max((int(last[k, lens[k]]), -k) for k in range(paths))
        ok = ok and mm is not None and (int(mm.group(3)), -int(mm.group(2))) == best
        ok = ok and R.rescore(mm.group(1), f[13], long_reads[i])[:2] == (best[0], len(long_reads[i]))
    med = {m: sorted(times[m])[rounds // 2] for m in modes}
    out = {"case": "gap_long", "rows": gg.rows, "paths": paths, "path_rows": max(len(r) for r in prow), "reads": nreads, "rounds": rounds}
    for m in modes:
        bm = batch[m]
        out["m%d" % m] = {"read_len": len(reads[m][0]), "ms_per_batch_median": round(med[m] * 1e3, 2), "ms_per_batch_min": round(min(times[m]) * 1e3, 2),
                          "counted_cell_updates": bm.cell_updates, "ps_per_counted_cell_update": round(med[m] / bm.cell_updates * 1e12, 3),
                          "performed_over_counted": round(bm.cell_updates_performed / bm.cell_updates, 3),
                          "kernel_ms_per_batch": {k: round(v, 2) for k, v in ks[m].items()}}
    out["m16_over_m6_time_per_cell_median"] = round(out["m16"]["ps_per_counted_cell_update"] / out["m6"]["ps_per_counted_cell_update"], 3)
    out["rule_checked"] = 2 if ok else "FAILED"
    print(json.dumps(out), flush=True)


def edit_case():
    from recgraph_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathwise_gap_rule as R
    unit = api.create_score_matrix_i32(0, -1)
    table = R.default_scores(0, -1)
    rounds = 5
    # (part, other mode, its score kernel, rows of the graph, paths, rows of a path = read length, reads)
    parts = (("a", api.MODE_PATHWISE_GAP_LONG, "k_gap_score_long", 12000, 16, 4000, 512), ("b", api.MODE_PATHWISE_GAP, "k_gap_score", 5000, 16, 1000, 2048),
             ("c", api.MODE_PATHWISE_GAP, "k_gap_score", 10000, 32, 1000, 2048))
    for part, other, other_score, grows, paths, plen, nreads in parts:
        if os.environ.get("RG_REGION_PART", part) != part:
            continue
        g = synth.haplotype_graph(grows, paths, path_len=plen, seed=1234)
        gg = api.Graph.from_gfa_text(g.gfa())
        reads = synth.haplotype_reads(g, nreads, length=plen, seed=900, mosaic_frac=0.0)
        modes = (api.MODE_PATHWISE_EDIT, other)
        batch = {m: api.Batch(gg, reads, api.make_params(m, score_matrix=unit, o=0, e=-1)) for m in modes}
        times = {m: [] for m in modes}
        ks = {m: {} for m in modes}
        mem = {}
        for m in modes:
            batch[m].run()                       # warm-up: code objects, work buffers
        for _ in range(rounds):
            for m in modes:                      # alternating: both modes see the same machine
                t0 = time.perf_counter()
                batch[m].run()
                times[m].append(time.perf_counter() - t0)
                for k, v in batch[m].kernel_stats().items():
                    if k == "mem:work_bytes_per_read":
                        mem[m] = v[0] / max(1, v[1])
                    if not k.startswith(("host:", "mem:", "inst:")):
                        ks[m][k] = ks[m].get(k, 0.0) + v[0] / rounds
        for m in modes:
            batch[m].fetch()
        b = batch[api.MODE_PATHWISE_EDIT]
        same = all(b.gaf_text(i, "r", 1) == batch[other].gaf_text(i, "r", 1) for i in range(nreads))
        same = same and (b.cell_updates, b.cell_updates_performed) == (batch[other].cell_updates, batch[other].cell_updates_performed)
        lnz, prow = R.graph_paths(gg)
        ok = True
        for i in (0, nreads - 1):
            f = b.gaf_text(i, "r", 1)[:-1].split("\t")
            mm = re.fullmatch(r"([0-9MXID]+), best path: (\d+), score: (-?\d+)", f[12])
            last, lens = R.all_paths_last(lnz, prow, reads[i], table, 0, -1, False)
            best = max((int(last[k, lens[k]]), -k) for k in range(paths))
            ok = ok and mm is not None and (int(mm.group(3)), -int(mm.group(2))) == best
            ok = ok and R.rescore(mm.group(1), f[13], reads[i], table, 0, -1)[:2] == (best[0], len(reads[i]))
        med = {m: sorted(times[m])[rounds // 2] for m in modes}
        out = {"case": "edit", "part": part, "rows": gg.rows, "paths": paths, "path_rows": max(len(r) for r in prow), "reads": nreads, "read_len": plen, "rounds": rounds}
        for m in modes:
            bm = batch[m]
            out["m%d" % m] = {"ms_per_batch_median": round(med[m] * 1e3, 2), "ms_per_batch_min": round(min(times[m]) * 1e3, 2),
                              "counted_cell_updates": bm.cell_updates, "ps_per_counted_cell_update": round(med[m] / bm.cell_updates * 1e12, 3),
                              "kernel_ms_per_batch": {k: round(v, 3) for k, v in ks[m].items()}, "work_bytes_per_read": int(mem.get(m, 0))}
        out["m44_over_m%d_time_per_batch_median" % other] = round(med[api.MODE_PATHWISE_EDIT] / med[other], 3)
        out["k_edit_score_over_%s" % other_score] = round(ks[api.MODE_PATHWISE_EDIT]["k_edit_score"] / ks[other][other_score], 3)
        out["same_texts_and_counters"] = bool(same)
        out["rule_checked"] = 2 if ok else "FAILED"
        print(json.dumps(out), flush=True)


def edit_xlong_case():
    from recgraph_amd import api, synth
    unit = api.create_score_matrix_i32(0, -1)
    rounds, paths, plen, nreads = 3, 16, 50000, 32
    g = synth.haplotype_graph(3 * plen, paths, path_len=plen, seed=1234)
    gg = api.Graph.from_gfa_text(g.gfa())
    reads = synth.haplotype_reads(g, nreads, length=plen, seed=901, mosaic_frac=0.0)
    modes = (api.MODE_PATHWISE_EDIT_XLONG, api.MODE_PATHWISE_GAP_XLONG)
    batch = {m: api.Batch(gg, reads, api.make_params(m, score_matrix=unit, o=0, e=-1)) for m in modes}
    times = {m: [] for m in modes}
    ks = {m: {} for m in modes}
    mem = {}
    for m in modes:
        batch[m].run()                           # warm-up: code objects, work buffers
    for _ in range(rounds):
        for m in modes:                          # alternating: both modes see the same machine
            t0 = time.perf_counter()
            batch[m].run()
            times[m].append(time.perf_counter() - t0)
            for k, v in batch[m].kernel_stats().items():
                if k == "mem:work_bytes_per_read":
                    mem[m] = v[0] / max(1, v[1])
                if not k.startswith(("host:", "mem:", "inst:")):
                    ks[m][k] = ks[m].get(k, 0.0) + v[0] / rounds
    for m in modes:
        batch[m].fetch()
    b, o = batch[modes[0]], batch[modes[1]]
    same = all(b.gaf_text(i, "r", 1) == o.gaf_text(i, "r", 1) and b.status(i) == o.status(i) == 0 and b.score(i) == o.score(i) for i in range(nreads))
    same = same and b.cell_updates == o.cell_updates
    med = {m: sorted(times[m])[rounds // 2] for m in modes}
    out = {"case": "edit_xlong", "rows": gg.rows, "paths": paths, "reads": nreads, "read_len": plen, "rounds": rounds,
           "stripes": {"m94": (max(len(r) for r in reads) + 16383) // 16384, "m56": (max(len(r) for r in reads) + 2048) // 2048}}
    for m in modes:
        bm = batch[m]
        out["m%d" % m] = {"ms_per_batch_median": round(med[m] * 1e3, 2), "ms_per_batch_min": round(min(times[m]) * 1e3, 2),
                          "counted_cell_updates": bm.cell_updates, "ps_per_counted_cell_update": round(med[m] / bm.cell_updates * 1e12, 3),
                          "performed_over_counted": round(bm.cell_updates_performed / bm.cell_updates, 3),
                          "kernel_ms_per_batch": {k: round(v, 3) for k, v in ks[m].items()}, "work_bytes_per_read": int(mem.get(m, 0))}
    out["m94_over_m56_time_per_batch_median"] = round(med[modes[0]] / med[modes[1]], 4)
    out["m94_over_m56_time_per_batch_min"] = round(min(times[modes[0]]) / min(times[modes[1]]), 4)
    out["k_edit_score_xlong_over_k_gap_score_long"] = round(ks[modes[0]]["k_edit_score_xlong"] / ks[modes[1]]["k_gap_score_long"], 4)
    out["same_texts_statuses_scores_and_counted_cells"] = bool(same)
    print(json.dumps(out), flush=True)


def edit_strands_case():
    from recgraph_amd import api, synth
    unit = api.create_score_matrix_i32(0, -1)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    rc = lambda r: "".join(comp[c] for c in reversed(r))
    # (part, rows of the graph, paths, rows of a path = read length, reads, rounds)
    parts = (("a", 12000, 16, 4000, 512, 3), ("b", 5000, 16, 1000, 2048, 5))
    for part, grows, paths, plen, nreads, rounds in parts:
        if os.environ.get("RG_REGION_PART", part) != part:
            continue
        g = synth.haplotype_graph(grows, paths, path_len=plen, seed=1234)
        gg = api.Graph.from_gfa_text(g.gfa())
        reads, _ = synth.reverse_complement_share(synth.haplotype_reads(g, nreads, length=plen, seed=900, mosaic_frac=0.0), 0.5, seed=5678)
        M64, M26, M44 = api.MODE_PATHWISE_EDIT_STRANDS, api.MODE_PATHWISE_GAP_STRANDS, api.MODE_PATHWISE_EDIT
        make = lambda m, rs: api.Batch(gg, rs, api.make_params(m, score_matrix=unit, o=0, e=-1))
        # the runs of a round: -m 64, -m 26, and the two -m 44 batches a caller without the mode submits
        batch = {"m64": make(M64, reads), "m26": make(M26, reads), "m44_given": make(M44, reads), "m44_revcomp": make(M44, [rc(r) for r in reads])}
        times = {k: [] for k in batch}
        ks = {k: {} for k in batch}
        mem = {}
        for k in batch:
            batch[k].run()                       # warm-up: code objects, work buffers
        for _ in range(rounds):
            for k in batch:                      # alternating: every run sees the same machine
                t0 = time.perf_counter()
                batch[k].run()
                times[k].append(time.perf_counter() - t0)
                for name, v in batch[k].kernel_stats().items():
                    if name == "mem:work_bytes_per_read":
                        mem[k] = v[0] / max(1, v[1])
                    if not name.startswith(("host:", "mem:", "inst:")):
                        ks[k][name] = ks[k].get(name, 0.0) + v[0] / rounds
        for k in batch:
            batch[k].fetch()
        a, b = batch["m64"], batch["m26"]
        strand = lambda bt, i: (bt.fields(i).strand if bt.fields(i) else None)
        same = all(a.gaf_text(i, "r", 1) == b.gaf_text(i, "r", 1) and a.status(i) == b.status(i) and a.score(i) == b.score(i) and strand(a, i) == strand(b, i)
                   for i in range(nreads))
        minus = sum(1 for i in range(nreads) if strand(a, i) == "-")
        # ... and the better of the two -m 44 records is the -m 64 record (reverse only when strictly greater)
        f, r = batch["m44_given"], batch["m44_revcomp"]
        agree = all(a.score(i) == max(f.score(i), r.score(i)) and (strand(a, i) == "-") == (r.score(i) > f.score(i)) for i in range(nreads))
        med = {k: sorted(times[k])[rounds // 2] for k in batch}
        out = {"case": "edit_strands", "part": part, "rows": gg.rows, "paths": paths, "reads": nreads, "read_len": plen, "rounds": rounds,
               "reverse_winners": minus}
        for k in batch:
            bm = batch[k]
            out[k] = {"ms_per_batch_median": round(med[k] * 1e3, 2), "ms_per_batch_min": round(min(times[k]) * 1e3, 2),
                      "counted_cell_updates": bm.cell_updates, "performed_cell_updates": bm.cell_updates_performed,
                      "kernel_ms_per_batch": {name: round(v, 3) for name, v in ks[k].items()}, "work_bytes_per_read": int(mem.get(k, 0))}
        two44 = med["m44_given"] + med["m44_revcomp"]
        two_scores = ks["m44_given"]["k_edit_score"] + ks["m44_revcomp"]["k_edit_score"]
        out["m64_over_m26_time_per_batch_median"] = round(med["m64"] / med["m26"], 4)
        out["m64_over_two_m44_batches_time_median"] = round(med["m64"] / two44, 4)
        out["k_edit_score_pair_over_two_k_edit_score"] = round(ks["m64"]["k_edit_score_pair"] / two_scores, 4)
        out["m64_kernel_sum_over_two_m44_kernel_sums"] = round(sum(ks["m64"].values()) / (sum(ks["m44_given"].values()) + sum(ks["m44_revcomp"].values())), 4)
        out["same_texts_statuses_scores_and_strands_as_m26"] = bool(same)
        out["agrees_with_the_better_of_the_two_m44_records"] = bool(agree)
        print(json.dumps(out), flush=True)


def gap_xlong_case():
    from recgraph_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathwise_gap_rule as R

    def timed(batch, rounds):
        times = {m: [] for m in batch}
        ks = {m: {} for m in batch}
        for m in batch:
            batch[m].run()                       # warm-up: code objects, work buffers
        for _ in range(rounds):
            for m in batch:                      # alternating: both modes see the same machine
                t0 = time.perf_counter()
                batch[m].run()
                times[m].append(time.perf_counter() - t0)
                for k, v in batch[m].kernel_stats().items():
                    if not k.startswith(("host:", "mem:", "inst:")):
                        ks[m][k] = ks[m].get(k, 0.0) + v[0] / rounds
        for m in batch:
            batch[m].fetch()
        return times, ks

    def entry(bm, rd, times, ks, rounds):
        med = sorted(times)[rounds // 2]
        return {"read_len": len(rd[0]), "ms_per_batch_median": round(med * 1e3, 2), "ms_per_batch_min": round(min(times) * 1e3, 2),
                "counted_cell_updates": bm.cell_updates, "ps_per_counted_cell_update": round(med / bm.cell_updates * 1e12, 3),
                "performed_over_counted": round(bm.cell_updates_performed / bm.cell_updates, 3),
                "work_bytes_per_read": int(bm.kernel_stats().get("mem:work_bytes_per_read", (0, 1))[0]),
                "kernel_ms_per_batch": {k: round(v, 2) for k, v in ks.items()}}

    def checked(b, reads, picks, lnz, prow, paths, all_paths):
        ok = True
        for i in picks:
            f = b.gaf_text(i, "r", 1)[:-1].split("\t")
            mm = re.fullmatch(r"([0-9MXID]+), best path: (\d+), score: (-?\d+)", f[12])
            if mm is None:
                return False
            k = int(mm.group(2))
            if all_paths:
                last, lens = R.all_paths_last(lnz, prow, reads[i], R.default_scores(), -4, -2, False)
                ok = ok and (int(mm.group(3)), -k) == max((int(last[q, lens[q]]), -q) for q in range(paths))
            else:
                last, lens = R.all_paths_last(lnz, [prow[k]], reads[i], R.default_scores(), -4, -2, False)
                ok = ok and int(mm.group(3)) == int(last[0, lens[0]])
            ok = ok and R.rescore(mm.group(1), f[13], reads[i])[:2] == (int(mm.group(3)), len(reads[i]))
        return ok

    # (a) -m 56 beside -m 16 on what both take
    rounds, paths, plen, nreads = 5, 16, 4000, 512
    g = synth.haplotype_graph(3 * plen, paths, path_len=plen, seed=1234)
    gg = api.Graph.from_gfa_text(g.gfa())
    reads = synth.haplotype_reads(g, nreads, length=plen, seed=900, mosaic_frac=0.0)
    modes = (api.MODE_PATHWISE_GAP_XLONG, api.MODE_PATHWISE_GAP_LONG)
    batch = {m: api.Batch(gg, reads, api.make_params(m)) for m in modes}
    times, ks = timed(batch, rounds)
    lnz, prow = R.graph_paths(gg)
    same = all(batch[56].gaf_text(i, "r", 1) == batch[16].gaf_text(i, "r", 1) and batch[56].status(i) == batch[16].status(i) for i in range(nreads))
    out = {"case": "gap_xlong", "part": "a", "rows": gg.rows, "paths": paths, "path_rows": max(len(r) for r in prow), "reads": nreads, "rounds": rounds}
    for m in modes:
        out["m%d" % m] = entry(batch[m], reads, times[m], ks[m], rounds)
    out["m56_over_m16_time_median"] = round(out["m56"]["ms_per_batch_median"] / out["m16"]["ms_per_batch_median"], 3)
    out["m56_over_m16_time_min"] = round(out["m56"]["ms_per_batch_min"] / out["m16"]["ms_per_batch_min"], 3)
    out["same_bytes_as_m16"] = same
    out["rule_checked"] = 2 if checked(batch[56], reads, (0, nreads - 1), lnz, prow, paths, True) else "FAILED"
    print(json.dumps(out), flush=True)
    del batch
    # (b) what no earlier mode accepts
    rounds, plen, nreads = 3, 50000, 32
    g = synth.haplotype_graph(3 * plen, paths, path_len=plen, seed=1234)
    gg = api.Graph.from_gfa_text(g.gfa())
    reads = synth.haplotype_reads(g, nreads, length=plen, seed=901, mosaic_frac=0.0)
    batch = {56: api.Batch(gg, reads, api.make_params(api.MODE_PATHWISE_GAP_XLONG))}
    times, ks = timed(batch, rounds)
    lnz, prow = R.graph_paths(gg)
    rows1 = max(len(r) for r in prow) + 1
    stripes = (max(len(r) for r in reads) + 2048) // 2048
    out = {"case": "gap_xlong", "part": "b", "rows": gg.rows, "paths": paths, "path_rows": rows1 - 1, "reads": nreads, "rounds": rounds, "stripes": stripes}
    out["m56"] = entry(batch[56], reads, times[56], ks[56], rounds)
    # what the layout of -m 16 takes for this geometry: stripes x rows1 KiB of direction words and both boundary buffers
    out["m16_layout_work_bytes_per_read"] = stripes * rows1 * 1024 + 8 * rows1 * (paths + 1)
    print(json.dumps(dict(out, rule_checked="pending")), flush=True)
    out["rule_checked"] = 2 if checked(batch[56], reads, (0, nreads - 1), lnz, prow, paths, False) else "FAILED"
    print(json.dumps(out), flush=True)


def gap_xstrands_case():
    """-m 76 / -m 77 / -m 82 beside -m 56 / -m 57 / -m 62 of the same build on the same reads, one process, alternating rounds: all
    forward, and half of the reads reverse-complemented (seed 5678), under the exact rule and (76 / 77) under the vote.  Shapes (a)
    and (b) of gap_xlong (RG_REGION_PART=a or b runs one of them).  Per both-strands batch, reads spread over the batch are checked:
    the strand against the flip, the line against the as-given mode's line of the source read (column 5 apart), the score against the
    numpy rule over all paths ((a); (b): over the printed path) and the re-scored CIGAR."""
    from recgraph_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathwise_gap_local_rule as L
    import pathwise_gap_rule as R
    import strand_vote_rule as V
    part = os.environ.get("RG_REGION_PART", "ab")
    paths = 16
    for tag, rounds, plen, nreads, seed in (("a", 5, 4000, 512, 900), ("b", 2, 50000, 32, 901)):
        if tag not in part:
            continue
        g = synth.haplotype_graph(3 * plen, paths, path_len=plen, seed=1234)
        gg = api.Graph.from_gfa_text(g.gfa())
        fwd = synth.haplotype_reads(g, nreads, length=plen, seed=seed, mosaic_frac=0.0)
        half, flipped = synth.reverse_complement_share(fwd, 0.5, seed=5678)
        runs = {"m62_fwd": (62, 0, fwd), "m82_fwd": (82, 0, fwd), "m82_half": (82, 0, half),
                "m56_fwd": (56, 0, fwd), "m76_fwd": (76, 0, fwd), "m76_half_exact": (76, 0, half), "m76_half_vote": (76, 12, half),
                "m57_fwd": (57, 0, fwd), "m77_fwd": (77, 0, fwd), "m77_half_exact": (77, 0, half), "m77_half_vote": (77, 12, half)}
        batch = {k: api.Batch(gg, rd, api.make_params(m, amb=amb or None)) for k, (m, amb, rd) in runs.items()}
        times = {k: [] for k in runs}
        ks = {k: {} for k in runs}
        for k in runs:
            batch[k].run()                       # warm-up: code objects, work buffers of every stage
        for _ in range(rounds):
            for k in runs:                       # alternating: every run sees the same machine
                t0 = time.perf_counter()
                batch[k].run()
                times[k].append(time.perf_counter() - t0)
                for name, v in batch[k].kernel_stats().items():
                    if not name.startswith(("host:", "mem:", "inst:")):
                        ks[k][name] = ks[k].get(name, 0.0) + v[0] / rounds
        for k in runs:
            batch[k].fetch()
        med = {k: sorted(times[k])[rounds // 2] for k in runs}
        out = {"case": "gap_xstrands", "part": tag, "rows": gg.rows, "paths": paths, "read_len": plen, "reads": nreads, "rounds": rounds,
               "reads_reverse_complemented": int(flipped.sum()), "seed": 5678}
        for k in runs:
            b = batch[k]
            out[k] = {"ms_per_batch_median": round(med[k] * 1e3, 2), "ms_per_batch_min": round(min(times[k]) * 1e3, 2),
                      "counted_cell_updates": b.cell_updates, "performed_over_counted": round(b.cell_updates_performed / b.cell_updates, 3),
                      "minus_records": sum(1 for i in range(nreads) if b.gaf_text(i, "r", 1).split("\t")[4:5] == ["-"]),
                      "work_bytes_per_read_summed_over_chunks": int(b.kernel_stats().get("mem:work_bytes_per_read", (0, 1))[0]),
                      "kernel_ms_per_batch": {name: round(v, 3) for name, v in ks[k].items()}}
        for num, den in (("m82_fwd", "m62_fwd"), ("m82_half", "m62_fwd"), ("m76_fwd", "m56_fwd"), ("m76_half_exact", "m56_fwd"), ("m76_half_vote", "m56_fwd"),
                         ("m77_fwd", "m57_fwd"), ("m77_half_exact", "m57_fwd"), ("m77_half_vote", "m57_fwd")):
            out["%s_over_%s" % (num, den)] = {"median": round(med[num] / med[den], 3), "min": round(min(times[num]) / min(times[den]), 3)}
        # the prediction for mode 82 from this run's own kernel times of mode 62: S the score pass and pick, T everything behind them
        k62 = ks["m62_fwd"]
        s = sum(v for name, v in k62.items() if name.startswith(("k_gap_score", "k_gap_pick")))
        t = sum(k62.values()) - s
        out["m82_predicted_from_m62_kernels"] = round((2 * s + t) / (s + t), 3) if s + t > 0 else None
        print(json.dumps(dict(out, rule_checked="pending")), flush=True)
        lnz, prow = R.graph_paths(gg)
        picks = sorted({0, nreads - 1} if tag == "a" else {nreads // 2})
        ok = True
        for k, (m, amb, rd) in runs.items():
            if m not in (76, 77, 82):
                continue
            b, base = batch[k], batch["m%d_fwd" % (m - 20)]
            for i in range(nreads):
                f = b.gaf_text(i, "r", 1).split("\t")
                want = base.gaf_text(i, "r", 1).split("\t")
                minus = bool(rd is half and flipped[i])
                # the line of the source read in the as-given mode, column 5 apart; the strand is the flip
                ok = ok and f[4] == ("-" if minus else "+") and f[:4] + f[5:] == want[:4] + want[5:] and b.status(i) == base.status(i)
            if tag == "b" and k not in ("m82_half", "m76_half_exact"):
                continue                             # (a numpy pass over 50 000 x 50 000 cells takes a minute: two batches stand for the eight)
            for i in picks:
                f = b.gaf_text(i, "r", 1)[:-1].split("\t")
                mm = re.fullmatch(r"([0-9MXID]+), best path: (\d+), score: (-?\d+)", f[12])
                chosen = V.rc(rd[i]) if f[4] == "-" else rd[i]
                ok = ok and mm is not None
                if not ok:
                    break
                score, q = int(mm.group(3)), int(mm.group(2))
                rows = prow if tag == "a" else [prow[q]]
                if m == 82:
                    best, _ = L.all_paths_best(lnz, rows, chosen, R.default_scores(), -4, -2)      # (no matrix is kept)
                    ok = ok and int(max(best)) == score and int(best[q if tag == "a" else 0]) == score
                    ok = ok and L.rescore(mm.group(1), f[13], chosen, int(f[2]), int(f[3]))[0] == score
                else:
                    last, lens = R.all_paths_last(lnz, rows, chosen, R.default_scores(), -4, -2, m == 77)
                    if m == 76:
                        best = max((int(last[p, lens[p]]), -p) for p in range(len(rows)))
                        ok = ok and best[0] == score and (tag != "a" or -best[1] == q)
                    ok = ok and R.rescore(mm.group(1), f[13], chosen)[:2] == (score, len(chosen))
        out["rule_checked"] = "FAILED" if not ok else len(picks)
        print(json.dumps(out), flush=True)
        del batch


def gap_strands_case():
    from recgraph_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathwise_gap_rule as R
    import pathwise_gap_strands_rule as S
    import strand_vote_rule as V
    rounds = 5
    for shape, rows, paths, rlen, nreads in (("C4", 5000, 16, 150, 4096), ("C4", 5000, 16, 1000, 2048), ("long", 12000, 16, 4000, 256)):
        g = synth.haplotype_graph(rows, paths, path_len=rlen, seed=1234)
        gg = api.Graph.from_gfa_text(g.gfa())
        fwd = synth.haplotype_reads(g, nreads, length=rlen, seed=900, mosaic_frac=0.0)
        half, flipped = synth.reverse_complement_share(fwd, 0.5, seed=5678)
        runs = {"m16_fwd": (16, 0, fwd), "m26_fwd": (26, 0, fwd), "m17_fwd": (17, 0, fwd), "m27_fwd": (27, 0, fwd),
                "m26_half_exact": (26, 0, half), "m26_half_vote": (26, 12, half), "m22_half": (22, 0, half), "m32_half": (32, 0, half)}
        batch = {k: api.Batch(gg, rd, api.make_params(m, amb=amb or None)) for k, (m, amb, rd) in runs.items()}
        times = {k: [] for k in runs}
        ks = {k: {} for k in runs}
        for k in runs:
            batch[k].run()                       # warm-up: code objects, work buffers of both passes
        for _ in range(rounds):
            for k in runs:                       # alternating: every run sees the same machine
                t0 = time.perf_counter()
                batch[k].run()
                times[k].append(time.perf_counter() - t0)
                for name, v in batch[k].kernel_stats().items():
                    if not name.startswith(("host:", "mem:", "inst:")):
                        ks[k][name] = ks[k].get(name, 0.0) + v[0] / rounds
        for k in runs:
            batch[k].fetch()
        lnz, prow = R.graph_paths(gg)
        ids = R.graph_node_ids(gg)
        kmers = V.kmer_set([g.path_sequence(q) for q in range(paths)])
        picks = sorted({0, nreads - 1, nreads // 2, nreads // 3, 777 % nreads})
        ok = True
        for k, (m, amb, rd) in runs.items():
            if m not in (26, 27, 32):
                continue
            b = batch[k]
            if rlen <= 1000:
                for i in picks:
                    text, status, strand, _ = S.expected(m, rd[i], S.line_fn(m, lnz, prow, ids, "r"), kmers if amb == 12 else None)
                    ok = ok and b.gaf_text(i, "r", 1) == text and b.status(i) == status
            elif m == 26:
                for i in picks[:2]:
                    f = b.gaf_text(i, "r", 1)[:-1].split("\t")
                    mm = re.fullmatch(r"([0-9MXID]+), best path: (\d+), score: (-?\d+)", f[12])
                    chosen = V.rc(rd[i]) if f[4] == "-" else rd[i]
                    last, lens = R.all_paths_last(lnz, prow, chosen, R.default_scores(), -4, -2, False)
                    best = max((int(last[q, lens[q]]), -q) for q in range(paths))
                    ok = ok and mm is not None and (int(mm.group(3)), -int(mm.group(2))) == best and best[0] >= 0
                    ok = ok and (f[4] == "-") == bool(rd is half and flipped[i])
                    ok = ok and R.rescore(mm.group(1), f[13], chosen)[:2] == (best[0], len(chosen))
        med = {k: sorted(times[k])[rounds // 2] for k in runs}
        out = {"case": "gap_strands", "shape": shape, "rows": gg.rows, "paths": paths, "read_len": rlen, "reads": nreads, "rounds": rounds,
               "reads_reverse_complemented": int(flipped.sum()), "seed": 5678}
        for k in runs:
            b = batch[k]
            out[k] = {"ms_per_batch_median": round(med[k] * 1e3, 2), "ms_per_batch_min": round(min(times[k]) * 1e3, 2),
                      "counted_cell_updates": b.cell_updates, "minus_records": sum(1 for i in range(nreads) if b.gaf_text(i, "r", 1).split("\t")[4:5] == ["-"]),
                      "kernel_ms_per_batch": {name: round(v, 3) for name, v in ks[k].items()}}
        for num, den in (("m26_fwd", "m16_fwd"), ("m27_fwd", "m17_fwd"), ("m26_half_exact", "m16_fwd"), ("m26_half_vote", "m16_fwd"), ("m32_half", "m22_half")):
            out["%s_over_%s" % (num, den)] = {"median": round(med[num] / med[den], 3), "min": round(min(times[num]) / min(times[den]), 3)}
        out["rule_checked"] = "FAILED" if not ok else 5 if rlen <= 1000 else 2
        print(json.dumps(out), flush=True)


def main():
    from recgraph_amd import api, synth
    from oracle import oracle as O
    if "edit_strands" in sys.argv[1:]:
        edit_strands_case()
        sys.argv = [a for a in sys.argv if a != "edit_strands"]
        if len(sys.argv) == 1:
            return
    if "edit_xlong" in sys.argv[1:]:
        edit_xlong_case()
        sys.argv = [a for a in sys.argv if a != "edit_xlong"]
        if len(sys.argv) == 1:
            return
    if "edit" in sys.argv[1:]:
        edit_case()
        sys.argv = [a for a in sys.argv if a != "edit"]
        if len(sys.argv) == 1:
            return
    if "gap_xlong" in sys.argv[1:]:
        gap_xlong_case()
        sys.argv = [a for a in sys.argv if a != "gap_xlong"]
        if len(sys.argv) == 1:
            return
    if "gap_xstrands" in sys.argv[1:]:
        gap_xstrands_case()
        sys.argv = [a for a in sys.argv if a != "gap_xstrands"]
        if len(sys.argv) == 1:
            return
    if "gap_strands" in sys.argv[1:]:
        gap_strands_case()
        sys.argv = [a for a in sys.argv if a != "gap_strands"]
        if len(sys.argv) == 1:
            return
    if "gap_long" in sys.argv[1:]:
        gap_long_case()
        sys.argv = [a for a in sys.argv if a != "gap_long"]
        if len(sys.argv) == 1:
            return
    if "gap_local" in sys.argv[1:]:
        gap_local_case()
        sys.argv = [a for a in sys.argv if a != "gap_local"]
        if len(sys.argv) == 1:
            return
    if "gap" in sys.argv[1:]:
        gap_case()
        sys.argv = [a for a in sys.argv if a != "gap"]
        if len(sys.argv) == 1:
            return
    names = [a for a in sys.argv[1:] if not a.startswith("-")] or [c for c in CASES if "strands" not in CASES[c][4]]
    check = 12
    handles = int(os.environ.get("RG_REGION_HANDLES", "3"))      # (1: the kernels' lone durations)
    opts = [kv.split("=") for kv in os.environ.get("RG_REGION_OPTS", "").split(",") if kv]      # e.g. sweep_i32=1,no_retire=1
    for k, v in opts:
        api.set_option(k, int(v))
    for name in names:
        mode, rows, paths, rlen, sk, tile, tiles = CASES[name]
        tiles *= int(os.environ.get("RG_REGION_TILES_X", "1"))        # (longer timed windows for A/B comparisons)
        g = synth.haplotype_graph(rows, paths, path_len=rlen, seed=1234)
        gfa = g.gfa()
        sm = None
        if "mm" in sk:
            sm = api.create_score_matrix_i32(*sk["mm"])
        elif "mtx" in sk:
            sm = api.create_score_matrix_i32(matrix_file_path=os.path.join(ROOT, "tests", "golden", sk["mtx"]))
        gg = api.Graph.from_gfa_text(gfa)
        strands = sk.get("strands")
        vote = bool(sk.get("vote"))
        params = api.make_params(mode, score_matrix=sm, amb=(api.AMB_BOTH_STRANDS | (api.AMB_STRAND_VOTE if vote else 0)) if strands in ("on_fwd", "on_half") else None)

        def tile_reads(k):
            """(reads of tile set k, per read: the source read the oracle aligns, whether the record must carry '-')"""
            src = synth.haplotype_reads(g, tile // 2 if strands == "two_n" else tile, length=rlen, seed=900 + k, mosaic_frac=0.5 if mode == 8 else 0.0)
            if strands == "on_half":
                rd, fl = synth.reverse_complement_share(src, 0.5, seed=900 + k)
                return rd, src, list(fl)
            if strands == "two_n":
                rd = [x for r in src for x in (r, api.rev_and_compl(r))]
                return rd, [x for r in src for x in (r, None)], [False] * len(rd)
            return src, src, [False] * len(src)
        sets = [api.Batch.pack_reads(tile_reads(k)[0]) for k in range(min(tiles, 3))]
        st = api.Stream(gg, params, device_ids=[0], handles_per_device=handles, tile_reads=tile)
        for k in range(3):
            st.push(sets[k % len(sets)])
        for k in range(3):
            st.next()
        k0 = st.kernel_stats()
        t0 = time.perf_counter()
        for k in range(tiles):
            st.push(sets[k % len(sets)])
        got = [st.next() for _ in range(tiles)]
        dt = time.perf_counter() - t0
        k1 = st.kernel_stats()
        ks = {k: round((v[0] - k0.get(k, (0, 0))[0]) / tiles, 2) for k, v in k1.items() if not k.startswith(("host:", "mem:", "inst:"))}
        st.close()
        # parity: reads spread over the whole index range of the LAST timed tile (every wave slot of a full launch: the round's
        # one wrong result only showed behind index 768 of a 4096-read launch), against the oracle's threaded runner
        og = O.Graph.from_gfa_text(gfa)
        osc = None if sm is None else O.scores_from_dict({k: int(v) for k, v in sm.items()})
        omode = {4: O.M4_ABS, 8: O.M8_ABS}[mode]
        last = got[-1]
        given, last_reads, minus = tile_reads((tiles - 1) % len(sets))
        idx = sorted(set([0, tile - 1] + [int(k * (tile - 1) / (check - 1)) for k in range(check)]))
        idx = [i for i in idx if last_reads[i] is not None]        # (two_n: the source reads; their reverse complements are the caller's to merge)
        kw = {} if osc is None else {"scores": osc}
        _, _, exp = og.bench_text(omode, [last_reads[i] for i in idx], nthreads=min(os.cpu_count() or 1, 32), name_prefix="x", **kw)
        ok = True
        if vote:
            # the vote must send every checked read to the strand it was drawn from, and that strand must be accepted (score >= 0):
            # then the rule's expected record is the source read's, '-' where the read was given reverse-complemented
            kmers = {p[q:q + 12] for p in (g.path_sequence(k) for k in range(paths)) for q in range(len(p) - 11)}
            ok = all(vote_first_reverse(kmers, given[i]) == bool(minus[i]) for i in idx) and \
                all(float(re.search(r"score: (-?[0-9.]+)", t.decode()).group(1)) >= 0 for t in exp)
        for k, i in enumerate(idx):
            e = exp[k].decode().replace("x%d\t" % k, "read%d\t" % (last.first + i), 1)
            if minus[i]:
                e = e.replace("\t+\t", "\t-\t", 1)
            # (bench_text numbers the reads by their position in the subset: everything but the trailing read index)
            ok = ok and last.text_of(i).decode().rsplit("\t", 1)[0] == e.rsplit("\t", 1)[0]
        sweeps = sorted(k for k in ks if k.startswith("k_sweep"))
        cu = sum(t.cell_updates for t in got)
        cp = sum(t.cell_updates_performed for t in got)
        source = tile // 2 if strands == "two_n" else tile
        print(json.dumps({"case": name, "mode": mode, "rows": gg.rows, "paths": paths, "read_len": rlen, "scores": sk or "default",
                          "tile_reads": tile, "tiles": tiles, "handles": handles, "options": dict((k, int(v)) for k, v in opts), "reads_per_s": round(source * tiles / dt, 1), "ms_per_tile": round(dt / tiles * 1e3, 2),
                          "cell_updates_per_s": round(cu / dt), "performed_over_counted": round(cp / cu, 3) if cu else None, "sweep_kernels": sweeps, "kernel_ms_per_tile": ks, "parity_checked": len(idx) if ok else "FAILED"}), flush=True)


if __name__ == "__main__":
    main()
