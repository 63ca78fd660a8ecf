"""-m 26 / -m 27 / -m 32 (modes 6 / 7 / 12 on both strands, reads of up to 16383 bases) on the GPU against the composed rule of
tests/pathwise_gap_strands_rule.py: which strands are aligned and which record is kept by the rules of RG_AMB_BOTH_STRANDS and
RG_AMB_STRAND_VOTE, every pass by the numpy rules of the base modes.

Every read is checked the same way (check_strands of tests/pathwise_support.py): (a) the whole line equals the rule's — the forward
line, or the line of the reverse complement with strand '-' — and is empty for a read without a record; (b) the status; (c)
rg_result_fields().strand and rg_result_score describe the chosen record; (d) the printed CIGAR, re-scored against the printed path
bases and the read ON THE STRAND THAT WAS CHOSEN (mode 32: its slice [query start, query end]), gives exactly the printed score.

The graphs are those of tests/test_gpu_pathwise_gap_long.py (haplotype of tests/pathwise_support.py); the rule's matrices stay under
rows * (n + 1) <= 1.2e7 per read."""
import re

import numpy as np
import pytest

import pathwise_gap_local_rule as L
import pathwise_gap_rule as R
import pathwise_gap_strands_rule as S
import strand_vote_rule as V
from pathwise_support import (NO_A, PALINDROME, check_strands, expect_strands, graph_tuple, haplotype, long_read, mixed_reads, noisy, rand_bases,
                              run_batch_strands, with_bad_base, wrong_strand_read_that_scores_above_zero)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("amb", [0, 4])
@pytest.mark.parametrize("mode", [26, 27])
def test_mixed_batch(mode, amb):
    """Both strands, a 1-base read, N only, a bad base (never in pass B), a reverse palindrome (a tie: '+'); amb_mode 4 is redundant."""
    from recgraph_amd import api
    graph = haplotype(300, 3)
    reads = list(mixed_reads(mode))
    assert V.rc(PALINDROME) == PALINDROME
    res = run_batch_strands(graph[1], reads, mode, amb=amb)
    exp = check_strands(graph, reads, mode, res)
    # (the 1-base read: whichever strand the rule says — globally, "T" may well beat "A")
    assert [e[2] for e in exp[:4] + exp[5:10]] == ["+", "+", "-", "-", "+", " ", "+", "-", "+"], [e[2] for e in exp]
    assert res["status"][6] == api.READ_BAD_BASE and res["texts"][6] == "" and exp[6][3] == []
    assert exp[7][3] == ["+", "-"] or mode == 27                  # (global: the palindrome scores below 0 on 300 rows, both ways alike)
    if mode == 27:
        rd, f, r = wrong_strand_read_that_scores_above_zero()
        assert 12 <= len(rd) <= 20 and f >= 0 and r > f
        # the exact rule keeps the FORWARD record of this read: its reverse complement was never aligned
        assert exp[10][2:] == ("+", ["+"]) and res["strand"][10] == "+" and res["score"][10] == f
    # pass B ran the qualifying reads only: one launch more of every pipeline kernel, and the three strand kernels once
    assert res["stats"]["k_gap_score"] == 2 and res["stats"]["k_strand_gate"] == res["stats"]["k_revcomp"] == res["stats"]["k_strand_merge"] == 1
    assert "k_gap_strands_gate" not in res["stats"] and "k_strand_vote" not in res["stats"]


@pytest.mark.parametrize("mode", [26, 27])
def test_pass_b_empty_and_pass_b_full(mode):
    """No forward score below 0: the bytes, statuses and scores of mode 16 / 17, and no merge.  Every read on the other strand: '-'."""
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(mode)
    w = [g.path_sequence(k) for k in range(3)]
    fwd = [noisy(rng, w[k]) for k in range(3)] if mode == 26 else [noisy(rng, w[0]), w[1][30:180], w[2][100:160], w[0][5:60]]
    exp = expect_strands(graph, fwd, mode)
    assert all(S.score_of(e[0]) >= 0 and e[3] == ["+"] for e in exp)
    res = run_batch_strands(gg, fwd, mode)
    check_strands(graph, fwd, mode, res, exp=exp)
    base = run_batch_strands(gg, fwd, mode - 10)
    assert (res["texts"], res["status"], res["score"]) == (base["texts"], base["status"], base["score"])
    assert "k_strand_merge" not in res["stats"] and res["stats"]["k_strand_gate"] == 1 and res["stats"]["k_gap_score"] == 1
    assert res["cells"] == base["cells"]
    rev = [V.rc(r) for r in fwd]
    res = run_batch_strands(gg, rev, mode)
    exp = check_strands(graph, rev, mode, res)
    assert [e[2] for e in exp] == ["-"] * len(rev) and all(t.split("\t")[4] == "-" for t in res["texts"])
    # reported exactly as the reverse complement would be had it been submitted by itself in mode 16 / 17, but for the strand
    assert [V.minus(t) for t in base["texts"]] == res["texts"] and res["score"] == base["score"]
    assert res["stats"]["k_strand_merge"] == 1 and res["stats"]["k_gap_score"] == 2


def _n_ops(text):
    return sum(int(x) for x in re.findall(r"(\d+)[MXID]", text.split("\t")[12].split(",")[0]))


@pytest.mark.parametrize("mode", [26, 27])
def test_the_passes_run_in_different_length_classes(mode):
    graph = haplotype(2200)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(40 + mode)
    w = g.path_sequence(0)
    short = [noisy(rng, w[300 * k + 20: 300 * k + 170], every=37) for k in range(4)]
    # (a) pass A striped (the 2100-base read is on the forward strand and stays there), pass B on the base kernels
    reads = [V.rc(short[0]), long_read(), V.rc(short[1]), V.rc(short[2]), short[3]]
    res = run_batch_strands(gg, reads, mode, log=True)
    exp = check_strands(graph, reads, mode, res)
    assert exp[1][2:] == ("+", ["+"]) and [e[2] for e in exp] == ["-", "+", "-", "-", "+"]
    assert max(len(reads[i]) for i, e in enumerate(exp) if "-" in e[3]) == 150
    kind = mode - 26
    assert res["inst"].get("rg::k_gap_score_long<%d>" % kind) == 1 and res["inst"].get("rg::k_gap_dirs_long<%d>" % kind) == 1, sorted(res["inst"])
    base = [k for k in res["inst"] if k.startswith("rg::k_gap_score<")]
    assert len(base) == 1 and res["inst"][base[0]] == 1, sorted(res["inst"])
    assert res["inst"].get("rg::k_strand_gate") == 1 and res["inst"].get("rg::k_strand_merge") == 1 and "rg::k_gap_strands_gate" not in res["inst"]
    # (b) the 2100-base read on the reverse strand: striped kernels in both passes, and a merge of more than 1024 op bytes that ends on
    # a partial 16-byte piece (more than one round per lane of k_strand_merge's copy loop)
    reads = [short[0], V.rc(long_read()), short[1]]
    res = run_batch_strands(gg, reads, mode, log=True)
    exp = check_strands(graph, reads, mode, res)
    assert exp[1][2:] == ("-", ["+", "-"])
    n_ops = _n_ops(exp[1][0])
    assert n_ops > 1024 and n_ops % 16 != 0, n_ops
    assert res["inst"].get("rg::k_gap_score_long<%d>" % kind) == 2 and res["inst"].get("rg::k_gap_dirs_long<%d>" % kind) == 2, sorted(res["inst"])
    assert not [k for k in res["inst"] if k.startswith("rg::k_gap_score<")], sorted(res["inst"])


def test_local_both_strands():
    from recgraph_amd import api
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(32)
    w = [g.path_sequence(k) for k in range(3)]
    flanked = [rand_bases(rng, 15) + noisy(rng, w[k][40 + 10 * k: 190 + 10 * k], every=31) + rand_bases(rng, 15) for k in range(3)]
    reads = [flanked[0], V.rc(flanked[1]), V.rc(flanked[2]), PALINDROME, "N" * 30, with_bad_base(w[0][10:90]), "A", w[1][100:130]]
    res = run_batch_strands(gg, reads, 32, log=True)
    exp = check_strands(graph, reads, 32, res)
    assert [e[2] for e in exp[:3]] == ["+", "-", "-"] and exp[3][2] in "+ " and exp[7][2] == "+"
    for i in range(3):
        # query start and end in the coordinates of the strand that was chosen: the flanks are clipped on both sides
        qs, qe = res["query"][i]
        assert 10 <= qs <= 20 and 160 <= qe <= 170, (i, qs, qe)
    assert (res["status"][4], res["texts"][4], exp[4][3]) == (api.READ_UNALIGNED, "", ["+", "-"])
    assert res["status"][5] == api.READ_BAD_BASE and exp[5][3] == []
    # every read with a record went through pass B, through the gate of this mode
    assert res["inst"].get("rg::k_gap_strands_gate") == 1 and "rg::k_strand_gate" not in res["inst"], sorted(res["inst"])
    assert res["stats"]["k_gap_strands_gate"] == 1 and res["stats"]["k_gap_score_local"] == 2 and res["stats"]["k_strand_merge"] == 1
    assert res["inst"].get("rg::k_revcomp") == 1 and res["inst"].get("rg::k_strand_merge") == 1
    # amb_mode 4 is redundant
    again = run_batch_strands(gg, reads, 32, amb=4)
    assert (again["texts"], again["status"], again["score"], again["strand"]) == (res["texts"], res["status"], res["score"], res["strand"])


def test_local_forward_unaligned_and_reverse_aligned():
    graph = graph_tuple(NO_A)
    gg, lnz, rows = graph[1:4]
    assert "A" not in "".join(lnz[r] for pr in rows for r in pr)
    reads = ["AAAAAA", "TTTTTT", "AAAA"]
    assert L.align_local(lnz, rows, "AAAAAA") is None or L.align_local(lnz, rows, "AAAAAA")[0] == 0
    res = run_batch_strands(gg, reads, 32)
    exp = check_strands(graph, reads, 32, res)
    assert [(e[1], e[2]) for e in exp] == [(0, "-"), (0, "+"), (0, "-")]
    assert res["score"][:2] == [12, 12] and res["strand"] == ["-", "+", "-"] and res["status"] == [0, 0, 0]
    assert res["texts"][0].split("\t")[1:] == V.minus(res["texts"][1]).split("\t")[1:]


def test_local_gate_feeds_the_striped_pass():
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(33)
    w = g.path_sequence(2)
    long_rd = rand_bases(rng, 1000) + noisy(rng, w) + rand_bases(rng, 2100 - 1000 - len(w))
    assert len(long_rd) == 2100
    reads = [g.path_sequence(0)[30:130], V.rc(long_rd), "N" * 12]
    res = run_batch_strands(gg, reads, 32, log=True)
    exp = check_strands(graph, reads, 32, res)
    assert [e[2] for e in exp] == ["+", "-", " "]
    assert res["inst"].get("rg::k_gap_strands_gate") == 1 and res["inst"].get("rg::k_gap_score_long<2>") == 2 and "rg::k_strand_gate" not in res["inst"]
    assert res["inst"].get("rg::k_gap_trace_local_long") == 2


def _cells(graph, reads, mode, exp):
    """(counted, performed) summed over the passes the rule says were run: rows_k * n per path, plus the direction pass of the chosen
    path (mode 26: all its rows; mode 27: up to the end row) times n."""
    g, gg, lnz, rows, node_ids = graph
    counted = performed = 0
    for rd, e in zip(reads, exp):
        for strand in e[3]:
            s = V.rc(S.canonical(rd)) if strand == "-" else S.canonical(rd)
            _, k, end_row = R.align(lnz, rows, s, semi=mode == 27)[:3]
            counted += sum(len(r) for r in rows) * len(s)
            performed += (rows[k].index(end_row) + 1 if mode == 27 else len(rows[k])) * len(s)
    return counted, counted + performed


@pytest.mark.parametrize("mode", [26, 27])
def test_strand_vote(mode):
    graph = haplotype(300, 3)
    g, gg = graph[0], graph[1]
    rng = np.random.default_rng(120 + mode)
    w = [g.path_sequence(k) for k in range(3)]
    kmers = V.kmer_set(w)
    short = w[0][5:12]
    good_rev = V.rc(noisy(rng, w[0], every=61)) if mode == 26 else V.rc(w[1][40:190])
    chimera = w[0][100:140] + V.rc(w[1][50:200])                       # its forward piece is the shorter one: the vote sends it reverse first
    hopeless_rev = V.rc(w[2][50:90]) + rand_bases(rng, 200)                  # reverse first, below 0 there: the forward strand is aligned too
    reads = [short, good_rev, chimera, hopeless_rev, noisy(rng, w[2]), V.rc(noisy(rng, w[1])), "N" * 40, with_bad_base(w[0][:80]), w[1][10:150]]
    assert V.votes(kmers, short) == (0, 0)
    vf, vr = V.votes(kmers, chimera)
    assert vr > vf > 0, (vf, vr)
    vf, vr = V.votes(kmers, hopeless_rev)
    assert vr > vf == 0
    res = run_batch_strands(gg, reads, mode, amb=12)
    exp = check_strands(graph, reads, mode, res, kmers=kmers)
    assert exp[0][3][0] == "+"                                         # votes 0 / 0: forward first
    assert exp[1][2:] == ("-", ["-"]) and S.score_of(exp[1][0]) >= 0    # reverse first and >= 0 there: forward never aligned
    assert exp[2][3][0] == "-" and exp[3][3] == ["-", "+"] and exp[7][3] == []
    if mode == 27:
        assert exp[2][2:] == ("-", ["-"])                               # ... and the same for the chimera the vote sent the wrong way
    assert res["stats"]["k_strand_vote"] == 1 and res["stats"]["k_strand_orient"] == 1 and res["stats"]["k_strand_gate"] == 1
    assert res["cells"] == _cells(graph, reads, mode, exp), (res["cells"], _cells(graph, reads, mode, exp))
    # the exact rule on the same reads runs other passes, and counts them
    exact = run_batch_strands(gg, reads, mode)
    exp0 = check_strands(graph, reads, mode, exact)
    assert exact["cells"] == _cells(graph, reads, mode, exp0)
    assert [e[3] for e in exp0] != [e[3] for e in exp]


@pytest.mark.parametrize("mode", [26, 32])
def test_stream_and_multi_give_the_batch_text(mode):
    from recgraph_amd import api
    graph = haplotype(300, 3)
    gg = graph[1]
    reads = list(mixed_reads(26))
    names = ["r%d" % i for i in range(len(reads))]
    res = run_batch_strands(gg, reads, mode)
    check_strands(graph, reads, mode, res)
    for kw in ({}, {"both_strands": True}):
        assert api.align_batch(gg, reads, names, mode=mode, **kw) == (res["texts"], res["status"])
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4, **kw)
        assert list(st) == res["texts"] and list(sstatus) == res["status"]
        mt, mstatus = api.align_batch_multi(gg, reads, names, mode=mode, device_ids=[0], **kw)
        assert mt == res["texts"] and mstatus == res["status"]
    st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], tile_reads=3, amb_strand=True)       # (`-s true` stays ignored)
    assert list(st) == res["texts"] and list(sstatus) == res["status"]
    if mode == 32:
        with pytest.raises(api._lib.RecGraphError) as ex:
            api.Stream(gg, api.make_params(32), device_ids=[0], strand_vote=True)
        assert ex.value.code == -1 and "hopeless" in str(ex.value)          # RG_ERR_ARG, and the message says why
        with pytest.raises(api._lib.RecGraphError):
            api.Batch(gg, reads, api.make_params(32, amb=12))
        one = api.pathwise_alignment_gap_local_exec(["$"] + list(reads[3]), gg, both_strands=True)
        assert one.strand == "-" and one.to_string() == res["texts"][3].replace("r3\t", "Temp\t", 1).rstrip("\n")
        assert api.pathwise_alignment_gap_local_exec(["$"] + list(V.rc(reads[3])), gg, both_strands=True).strand == "+"
    else:
        vote = run_batch_strands(gg, reads, mode, amb=12)
        st, sstatus = api.align_stream(gg, reads, names, mode=mode, device_ids=[0], handles_per_device=2, tile_reads=4, strand_vote=True)
        assert list(st) == vote["texts"] and list(sstatus) == vote["status"]
        assert api.align_batch(gg, reads, names, mode=mode, strand_vote=True) == (vote["texts"], vote["status"])
        one = api.pathwise_alignment_gap_exec(["$"] + list(reads[2]), gg, both_strands=True)
        assert one.strand == "-" and one.to_string() == res["texts"][2].replace("r2\t", "Temp\t", 1).rstrip("\n")


def test_the_cli_runs_the_modes(tmp_path, capsys):
    from recgraph_amd import api, cli
    g, gg = haplotype(300, 3)[:2]
    reads = [g.path_sequence(0)[20:170], V.rc(g.path_sequence(1)[20:170]), "NNNN"]
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fa").write_text("".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    for m, flags in ((27, []), (27, ["--strand-vote"]), (32, ["--both-strands"])):
        exp, st = api.align_batch(gg, reads, ["s%d" % i for i in range(3)], mode=m, strand_vote="--strand-vote" in flags)
        assert exp[1].split("\t")[4] == "-"
        cli.main([str(tmp_path / "r.fa"), str(tmp_path / "g.gfa"), "-m", str(m), "--devices", "0"] + flags)
        assert capsys.readouterr().out == "".join(exp)
