"""The rule of RG_AMB_STRAND_VOTE (include/recgraph_hip.h) stated in Python, for tests/test_strand_vote_cpu.py and
tests/test_gpu_strand_vote.py: the 12-mer vote from the path sequences of the GFA, and the expected text of a read set
built from the oracle by that rule.  Nothing here asks the product anything."""
import os
import re

K = 12
SAMPLES = 256
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def threads(cap=32):
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(cap, n))


def gfa_paths(gfa):
    """Sequences of the P lines of a GFA (forward segments only, as the graphs of these tests have them)."""
    seg, paths = {}, []
    for ln in gfa.splitlines():
        f = ln.split("\t")
        if f[0] == "S":
            seg[f[1]] = f[2]
        elif f[0] == "P":
            paths.append("".join(seg[s[:-1]] for s in f[2].split(",")))
    return paths


def kmer_set(path_seqs):
    """Every 12-mer of A/C/G/T only that some path contains."""
    out = set()
    for s in path_seqs:
        for q in range(len(s) - K + 1):
            w = s[q:q + K]
            if set(w) <= set("ACGT"):
                out.add(w)
    return out


def count(kmers, s):
    npos = len(s) - K + 1
    if npos < 1:
        return 0
    step = -(-npos // SAMPLES)
    return sum(1 for q in range(0, npos, step) if s[q:q + K] in kmers)      # (a window with an N is in no path's set)


def votes(kmers, read):
    """(V_f, V_r) of a read given as text.  A read with a character outside ACGTN ('-' counts as N) votes 0 / 0."""
    s = read.upper().replace("-", "N")
    if not set(s) <= set("ACGTN"):
        return 0, 0
    return count(kmers, s), count(kmers, rc(s))


def first_reverse(kmers, read):
    vf, vr = votes(kmers, read)
    return vr > vf


def printed_score(text):
    return float(re.search(r"score: (-?[0-9.]+)", text).group(1))


def minus(text):
    f = text.split("\t")
    assert f[4] == "+"
    f[4] = "-"
    return "\t".join(f)


def oracle_texts(og, omode, reads, prefix="q"):
    """The oracle's stdout text per read, read i called prefix + str(i).  Its threaded runner writes into a buffer of
    4096 bytes per read + 64 KiB; a 2 150-base read that aligns badly prints more than that (one CIGAR run per base, then the
    read), so the reads go in groups whose worst case (6 bytes per base + 1 KiB per read) fits."""
    out, lo = [], 0
    while lo < len(reads):
        hi, need = lo, 0
        while hi < len(reads) and (hi == lo or need + 6 * len(reads[hi]) + 1024 <= 4096 * (hi - lo + 1) + 65536):
            need += 6 * len(reads[hi]) + 1024
            hi += 1
        _, _, t = og.bench_text(omode, reads[lo:hi], nthreads=threads(), name_prefix=prefix, name_base=lo, idx_base=1 + lo)
        out += [x.decode() for x in t]
        lo = hi
    return out


def expected_strand_vote(og, omode, kmers, reads, prefix="q"):
    """Per read: (expected text, first strand is '-', both strands aligned, chosen strand is '-', the chosen record has a
    recombination), from the oracle and the vote alone.  Read i is called prefix + str(i).  Reads must be clean (ACGTN)."""
    n = len(reads)
    frev = [first_reverse(kmers, r) for r in reads]
    pa = oracle_texts(og, omode, [rc(r) if frev[i] else r for i, r in enumerate(reads)], prefix)
    retry = {i for i in range(n) if printed_score(pa[i]) < 0}
    pb = [None] * n
    if retry:
        # (the oracle names by position: the retried reads keep their places, the others are one base long)
        sub = [(reads[i] if frev[i] else rc(reads[i])) if i in retry else "A" for i in range(n)]
        got = oracle_texts(og, omode, sub, prefix)
        for i in retry:
            pb[i] = got[i]
    out = []
    for i in range(n):
        fwd, rev = (pb[i], pa[i]) if frev[i] else (pa[i], pb[i])
        if fwd is None:
            take_rev = True
        elif rev is None:
            take_rev = False
        else:
            take_rev = printed_score(rev) > printed_score(fwd)          # ties keep forward, whichever went first
        text = minus(rev) if take_rev else fwd
        out.append((text, frev[i], i in retry, take_rev, "recombination path" in text))
    return out
