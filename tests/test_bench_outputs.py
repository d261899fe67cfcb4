"""bench.py --dump-outputs / --full: a plain run does the timed workload only
(no CPU baseline, no config-1 leg), --steps sets the timed steps, and the
dumped arrays are what the last timed step computed -- the same files from run
to run, and on the GPU the oracle's ciphertext and the plaintext back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def run_bench(*args, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def chunk_sums(a, chunk):
    """dump_outputs' <name>_sums, restated: sum_j (1 + j mod 251) * byte[j] per chunk."""
    a = np.concatenate([a, np.zeros(-len(a) % chunk, dtype=np.uint8)]).reshape(-1, chunk)
    w = np.arange(chunk, dtype=np.int64) % 251 + 1
    return (a.astype(np.int64) * w).sum(axis=1).astype(np.float64)


def sample_index(n, count, seed):
    return np.sort(np.random.RandomState(seed & 0xffffffff).randint(0, n, count, dtype=np.int64))


def test_dump_outputs_whole_and_sampled(tmp_path):
    """An array up to 1 MiB is written whole; a larger one (here not a multiple
    of the chunk) as a seeded sample plus one weighted sum per 64 KiB."""
    import bench
    rng = np.random.RandomState(1)
    small = rng.randint(0, 256, 1000).astype(np.uint8)
    big = rng.randint(0, 256, (1 << 21) + 12345).astype(np.uint8)
    bench.dump_outputs(str(tmp_path), {"small": small, "big": big})
    assert sorted(os.listdir(tmp_path)) == ["big_sample.npy", "big_sums.npy", "small.npy"]
    got = np.load(tmp_path / "small.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    s = np.load(tmp_path / "big_sample.npy")
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(s, big[sample_index(len(big), bench.DUMP_SAMPLE, bench.SEED)])
    sums = np.load(tmp_path / "big_sums.npy")
    assert sums.dtype == np.float64 and np.array_equal(sums, chunk_sums(big, bench.DUMP_CHUNK))


def test_stub_plain_run_steps_and_dump(tmp_path):
    """--steps sets the timed steps (the stub flips its buffer once per step,
    the round-trip check's step and the warmup included), the dump is the same
    from run to run, and --full is accepted."""
    dumps = []
    for sub, steps, extra in (("a", 3, []), ("b", 3, ["--full"]), ("c", 4, [])):
        d = run_bench("--stub", "--records", "100", "--steps", str(steps), "--warmup", "1",
                      "--min-warmup-s", "0", "--dump-outputs", str(tmp_path / sub), *extra)
        assert d["steps"] == steps and d["ms_per_step"] > 0
        assert "cpu_baseline" not in d and "config1" not in d
        assert os.listdir(tmp_path / sub) == ["buf.npy"]
        dumps.append(np.load(tmp_path / sub / "buf.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (100 * 64,)
    # 1 check step + 1 warmup + 3 timed = 5 flips of 0x5A; + 4 timed = 6 flips
    assert np.all(dumps[0] == 0x5A) and np.array_equal(dumps[0], dumps[1]) and np.all(dumps[2] == 0)


@pytest.mark.gpu
def test_gpu_plain_run_dumps_oracle_outputs(tmp_path, oracle):
    """A plain config-2 run on the GPU: no CPU baseline or config-1 leg in the
    line, and the dumped ciphertext / plaintext / status are the oracle's,
    byte for byte through the sample and through every chunk's sum."""
    import bench
    R, L = 2050, 1024  # above 1 MiB, ciphertext no multiple of the 64 KiB chunk
    d = run_bench("--records", str(R), "--steps", "2", "--warmup", "1", "--min-warmup-s", "0",
                  "--dump-outputs", str(tmp_path))
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "u32"
    assert "cpu_baseline" not in d and "config1" not in d
    assert sorted(os.listdir(tmp_path)) == ["back_sample.npy", "back_sums.npy", "ct_sample.npy",
                                            "ct_sums.npy", "status.npy"]
    pt = np.frombuffer(oracle.synthetic(R * L, bench.SEED), dtype=np.uint8)
    ct = oracle.encrypt_uniform_np(bench.KEY, 0, pt, L, L, L + 16, R)
    assert np.array_equal(np.load(tmp_path / "status.npy"), np.zeros(R, dtype=np.float32))
    for name, want in (("back", pt), ("ct", ct)):
        assert np.array_equal(np.load(tmp_path / (name + "_sample.npy")),
                              want[sample_index(len(want), bench.DUMP_SAMPLE, bench.SEED)])
        assert np.array_equal(np.load(tmp_path / (name + "_sums.npy")),
                              chunk_sums(want, bench.DUMP_CHUNK))
