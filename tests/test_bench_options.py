"""bench.py's plain run (only what the headline needs), `--full` and `--dump-outputs`: over the stub stream on the CPU
(RG_BENCH_STUB=1: no device work), and once on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, stub=True, timeout=300):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RG_BENCH_STUB"):
        env.pop(k, None)
    if stub:
        env["RG_BENCH_STUB"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _load_dump(d):
    files = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    arrs = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    for name, a in arrs.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    return arrs


def _check_dump(arrs, n):
    """The dump of a step of `n` reads: the reads it holds, their text lengths and scores, the text itself."""
    reads = arrs["reads"].astype(np.int64)
    assert len(reads) and np.all(np.diff(reads) > 0) and reads[0] >= 0 and reads[-1] < n
    assert len(arrs["text_len"]) == len(reads) and int(arrs["text_len"].sum()) == len(arrs["text"])
    for k in ("score", "status"):
        if k in arrs:
            assert len(arrs[k]) == len(reads)
    return arrs["text"].astype(np.uint8).tobytes()


def test_plain_run_leaves_the_extra_regions_to_full():
    base = ["--config", "C2", "--batch", "64", "--steps", "3", "--warmup", "1", "--gpus", "2"]
    plain = _bench(base)
    assert plain["strong_100k"] is None
    full = _bench(base + ["--full", "--no-cpu"])
    assert full["strong_100k"]["reads"] == 25 * 64
    for d in (plain, full):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 3 and d["ms_per_step"] > 0


def test_steps_sets_the_timed_steps():
    per_step = sum(len("read%d\t" % i) + 16 + 1 for i in range(64))
    for steps in (1, 4):
        d = _bench(["--config", "C2", "--batch", "64", "--steps", str(steps), "--warmup", "0"])
        assert d["steps"] == steps and d["gaf_bytes_gathered"] == steps * per_step


def test_dump_outputs_are_the_last_step_and_repeat(tmp_path):
    args = ["--config", "C5", "--batch", "64", "--steps", "3", "--warmup", "1"]
    dumps = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        _bench(args + ["--dump-outputs", d])
        dumps.append(_load_dump(d))
    a, b = dumps
    assert sorted(a) == sorted(b) == ["reads", "text", "text_len"]      # the stub has no scores
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    lines = _check_dump(a, 64).decode().splitlines()
    assert len(lines) == 64 and [ln.split("\t")[0] for ln in lines] == ["read%d" % i for i in range(64)]
    # the last timed step's reads, not the first step's: a run of one step dumps other reads
    d1 = str(tmp_path / "one")
    _bench(["--config", "C5", "--batch", "64", "--steps", "1", "--warmup", "1", "--dump-outputs", d1])
    assert not np.array_equal(_load_dump(d1)["text"], a["text"])


def test_dump_outputs_hold_every_rank(tmp_path):
    d = str(tmp_path / "two")
    _bench(["--config", "C5", "--batch", "64", "--steps", "3", "--warmup", "1", "--gpus", "2", "--dump-outputs", d])
    lines = _check_dump(_load_dump(d), 128).decode().splitlines()
    # rank 0's tile, then rank 1's (the stub names the reads of a tile read0 ..): different reads of the same step
    assert [ln.split("\t")[0] for ln in lines] == ["read%d" % i for i in range(64)] * 2
    assert lines[:64] != lines[64:]


def test_dump_of_a_large_step_is_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)

    def part(r, n):
        text = b"".join(b"r%dread%d\t%s\n" % (r, i, b"ACGT" * (1 + i % 7)) for i in range(n))
        off = np.cumsum([0] + [len(ln) + 1 for ln in text.split(b"\n")[:-1]]).astype(np.int64)
        return text, off, np.arange(n, dtype=np.int32) - 7 + 1000 * r, np.full(n, r, dtype=np.uint32)
    parts = [part(0, 120), part(1, 80)]
    dumps = []
    for k in range(2):
        d = str(tmp_path / ("d%d" % k))
        bench.dump_outputs(d, parts)
        dumps.append(_load_dump(d))
    a, b = dumps
    assert sorted(a) == ["reads", "score", "status", "text", "text_len"]
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    blob = _check_dump(a, 200)
    reads = a["reads"].astype(np.int64)
    assert 0 < len(reads) < 200 and 8 * 4 * len(reads) + 4 * len(blob) <= 4000
    whole = parts[0][0] + parts[1][0]
    lines = whole.decode().splitlines(keepends=True)
    assert blob.decode() == "".join(lines[i] for i in reads)
    score = np.concatenate([parts[0][2], parts[1][2]])
    assert np.array_equal(a["score"], score[reads].astype(np.float64))
    assert np.array_equal(a["status"], (reads >= 120).astype(np.float64))


def test_profile_pass_asks_for_the_roofline():
    """tools/make_counters.py reads the `roofline` object of the bench lines tools/profile_round.sh records: only --full
    prints it."""
    calls = [ln for ln in open(os.path.join(ROOT, "tools", "profile_round.sh")) if "bench.py" in ln and not ln.lstrip().startswith("#")]
    assert len(calls) == 2 and all(" --full" in ln for ln in calls)


@pytest.mark.gpu
def test_gpu_plain_run_dumps_what_the_stream_returned(tmp_path):
    d = str(tmp_path / "dump")
    out = _bench(["--gpus", "1", "--batch", "256", "--steps", "2", "--warmup", "1", "--dump-outputs", d], stub=False, timeout=600)
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 2
    assert out["cpu_baseline"] is None and out["strong_proxy"] is None and out["int32"] is None and out["roofline"] is None
    arrs = _load_dump(d)
    assert sorted(arrs) == ["reads", "score", "status", "text", "text_len"]
    blob = _check_dump(arrs, 256)
    assert len(arrs["reads"]) == 256 and len(blob) > 0


@pytest.mark.gpu
def test_gpu_profile_pass_flags_print_the_roofline_make_counters_reads():
    """The flags tools/profile_round.sh runs bench.py with under rocprofv3 (--pmc passes, config 5) print the roofline fields
    tools/make_counters.py needs."""
    out = _bench(["--config", "C5", "--batch", "2048", "--steps", "2", "--warmup", "0", "--no-cpu", "--no-strong", "--no-probe",
                  "--handles", "1", "--full"], stub=False, timeout=600)
    roof = out["roofline"]
    assert roof["reads_per_launch"] > 0 and roof["kernel"].startswith("k_sweep") and roof["code_hash"]
    assert out["strong_proxy"] is None and out["int32"] is None and out["cpu_baseline"] is None
