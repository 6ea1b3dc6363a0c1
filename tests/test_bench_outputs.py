"""bench.py --dump-outputs / --full: the sample of the state a run writes (CPU: the sampler alone; GPU: a plain run end to
end, its line and its sample checked bit for bit against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, extra_env=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_options_exist():
    r = run_bench(["--help"], timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    """at the headline size: 64 blocks of 2^14 amplitudes, every row the amplitude its index names, the same files from
    call to call, within 64 MB"""
    import bench
    n = 30
    reader = lambda first, count: np.arange(2 * first, 2 * (first + count), dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 1 << n, reader)
    amps = np.load(tmp_path / "a" / "state_sample.npy")
    idx = np.load(tmp_path / "a" / "state_sample_index.npy")
    assert amps.dtype == np.float64 and idx.dtype == np.float64
    assert amps.shape == (64 << 14, 2) and idx.shape == (64 << 14,)
    assert np.array_equal(amps[:, 0], 2 * idx) and np.array_equal(amps[:, 1], 2 * idx + 1)
    assert np.unique(idx).size == idx.size and idx.min() >= 0 and idx.max() < 2 ** n
    assert np.array_equal(idx % (1 << 14), np.tile(np.arange(1 << 14), 64))          # whole, aligned blocks
    total = 0
    for f in ("state_sample.npy", "state_sample_index.npy"):
        a, b = (tmp_path / "a" / f).read_bytes(), (tmp_path / "b" / f).read_bytes()
        assert a == b
        total += len(a)
    assert total <= 64 * 2 ** 20


def test_dump_of_a_small_register_is_the_whole_state(tmp_path):
    import bench
    reader = lambda first, count: np.arange(2 * first, 2 * (first + count), dtype=np.float64)
    bench.dump_outputs(str(tmp_path), 1 << 10, reader)
    assert np.array_equal(np.load(tmp_path / "state_sample_index.npy"), np.arange(1 << 10, dtype=np.float64))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_state_the_oracle_computes(tmp_path, ob):
    """a plain run: one JSON line with the headline fields and none of the --full legs; its dumped sample = the oracle's
    state after warmup + steps sweeps of the same seeded input, bit for bit"""
    n, steps, warmup = 20, 2, 1
    r = run_bench(["--steps", str(steps), "--warmup", str(warmup), "--n-local", str(n), "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup and out["config"]["qubits"] == n
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["unit"] == "amplitude-updates/s" and out["metric"].startswith("amplitude-updates/s")
    assert out["fused_sweep"] is None and out["configs"] is None and "cpu_baseline" not in out
    amps = np.load(tmp_path / "state_sample.npy")
    idx = np.load(tmp_path / "state_sample_index.npy")
    want = ob.fill_random(n, 1)
    for _ in range(warmup + steps):
        for q in range(n):
            ob.hadamard(want, n, q)
    want = want.reshape(-1, 2)[idx.astype(np.int64)]
    assert np.array_equal(amps.view(np.uint64), want.view(np.uint64))


@pytest.mark.gpu
def test_two_rank_rehearsal_dumps_rank0_shard_as_the_oracle_computes(tmp_path, ob):
    """N > 1 (two ranks rehearsed on the one GPU over gloo): the sample comes from rank 0's shard in the identity layout,
    i.e. amplitudes 0 .. 2^n_local - 1 of the whole state, bit for bit the oracle's"""
    nl, steps, warmup = 18, 1, 1
    n = nl + 1
    r = run_bench(["--gpus", "2", "--steps", str(steps), "--warmup", str(warmup), "--n-local", str(nl), "--dump-outputs", str(tmp_path)],
                  extra_env={"QCX_BENCH_BACKEND": "gloo", "QCX_FORCE_DEVICE": "0"})
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][0])
    assert out["n_gpus"] == 2 and out["config4"] is None and "c_host" in out and out["c_host"] is None
    amps = np.load(tmp_path / "state_sample.npy")
    idx = np.load(tmp_path / "state_sample_index.npy")
    assert idx.max() < 2 ** nl
    want = ob.fill_random(n, 1)
    for _ in range(warmup + steps):
        for q in range(n):
            ob.hadamard(want, n, q)
    want = want.reshape(-1, 2)[idx.astype(np.int64)]
    assert np.array_equal(amps.view(np.uint64), want.view(np.uint64))
