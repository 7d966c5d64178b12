"""bench.py's launcher contract on the CPU (no GPU touched): `python bench.py
--gpus N` with no launcher starts torch.distributed.run with N ranks as a
child process, relays rank 0's single JSON line and exits non-zero when any
rank fails; a WORLD_SIZE / --gpus mismatch is rejected.  The ranks run the
BENCH_LAUNCH_PROBE body (join a gloo group, rank 0 prints one line); the
full N>1 bench body is rehearsed on the GPU box
(tests/test_gpu_distrib.py::test_bench_self_launch_rehearsal)."""
import json
import os
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env.update(kw)
    return env


def _run(args, env, timeout=240):
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=timeout, cwd=str(ROOT))


def test_bench_starts_its_ranks_without_a_launcher():
    r = _run(["--gpus", "2"], _env(BENCH_LAUNCH_PROBE="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d == {"probe": True, "world": 2}


def test_bench_launcher_fails_when_a_rank_fails():
    r = _run(["--gpus", "2"], _env(BENCH_LAUNCH_PROBE="fail"))
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_rejects_world_size_mismatch():
    r = _run(["--gpus", "4"], _env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", BENCH_LAUNCH_PROBE="1"), timeout=60)
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr


def test_bench_n_gt_1_defaults_to_configs3_share():
    """configs[3] = 2^32 keys over 8 GPUs: 2^29 keys per GPU at N>1, 2^28
    (configs[1]) at N=1."""
    sys.path.insert(0, str(ROOT))
    import bench
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "8"]
        a = bench.parse()
        assert a.keys_log2 == 29 and a.digit_bits == 4
        sys.argv = ["bench.py"]
        a = bench.parse()
        assert a.keys_log2 == 28 and a.digit_bits == 4
        sys.argv = ["bench.py", "--gpus", "8", "--workload", "c5"]
        assert bench.parse().keys_log2 == 28                       # 2^31 pairs over 8 GPUs
    finally:
        sys.argv = old


def test_bench_full_and_dump_outputs_options():
    sys.path.insert(0, str(ROOT))
    import bench
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse()
        assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
        sys.argv = ["bench.py", "--full", "--dump-outputs", "somewhere"]
        a = bench.parse()
        assert a.full is True and a.dump_outputs == "somewhere"
    finally:
        sys.argv = old


def test_dump_outputs_sample_and_block_sums(tmp_path):
    """bench.dump_outputs on host tensors: float64 arrays, the seeded sample
    of an array longer than the sample (the whole of a shorter one), block
    sums over every element (a short last block included), the words of a
    u64 key, one set per shard at N > 1, and at most 64 MB."""
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import bench
    rng = np.random.default_rng(3)
    n = bench.DUMP_SAMPLE + 3 * bench.DUMP_BLOCK + 5
    k = np.sort(rng.integers(0, 1 << 32, n, dtype=np.uint64)).astype(np.uint32)
    bench.dump_outputs(torch, tmp_path / "a", torch.from_numpy(k.view(np.int32)), False, 0, 1)
    got, sums = np.load(tmp_path / "a" / "sorted_keys.npy"), np.load(tmp_path / "a" / "sorted_keys_block_sums.npy")
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, bench.DUMP_SAMPLE, dtype=np.int64))
    assert got.dtype == np.float64 and sums.dtype == np.float64
    np.testing.assert_array_equal(got, k[pos].astype(np.float64))
    assert sums.size == 3 + bench.DUMP_SAMPLE // bench.DUMP_BLOCK + 1 and sums.sum() == float(k.astype(np.uint64).sum())
    assert sums[-1] == float(k[-5:].astype(np.uint64).sum())
    # pairs, two shards held by one process (the C engine's result): whole arrays (shorter than the sample)
    k64 = rng.integers(0, 1 << 64, 1000, dtype=np.uint64)
    v = rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    ks = [torch.from_numpy(k64[:600].view(np.int64)), torch.from_numpy(k64[600:].view(np.int64))]
    vs = [torch.from_numpy(v[:600].view(np.int32)), torch.from_numpy(v[600:].view(np.int32))]
    bench.dump_outputs(torch, tmp_path / "b", (ks, vs), True, 0, 2)
    for r, sl in enumerate((slice(0, 600), slice(600, 1000))):
        hi = np.load(tmp_path / "b" / ("sorted_keys_hi_shard%d.npy" % r))
        lo = np.load(tmp_path / "b" / ("sorted_keys_lo_shard%d.npy" % r))
        vv = np.load(tmp_path / "b" / ("sorted_vals_shard%d.npy" % r))
        np.testing.assert_array_equal(hi.astype(np.uint64) << np.uint64(32) | lo.astype(np.uint64), k64[sl])
        np.testing.assert_array_equal(vv, v[sl].astype(np.float64))
        assert np.load(tmp_path / "b" / ("sorted_vals_block_sums_shard%d.npy" % r))[0] == float(v[sl].astype(np.uint64).sum())
    # a rank that holds no result writes nothing
    bench.dump_outputs(torch, tmp_path / "c", None, False, 1, 2)
    assert not (tmp_path / "c").exists()
    # the largest line (configs[4] over 8 GPUs: 3 arrays of 2^28 per shard) stays under 64 MB
    worst = 3 * 8 * (bench.DUMP_SAMPLE // 8 + (1 << 28) // bench.DUMP_BLOCK) * 8
    assert worst <= 64 * 1000 * 1000
