"""bench.py's own contract: --dump-outputs writes what the timed path returned (bounded, seeded sample above the cap), --steps sets the
timed passes, and a plain run carries only the headline line while --full adds the side measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_output_is_bounded_seeded_and_float32(tmp_path):
    import bench
    small = torch.randn(8, 750, 64, dtype=torch.float64)
    bench.dump_output(str(tmp_path), "small", small, bench.DUMP_BYTES)
    got = np.load(tmp_path / "small.npy")
    assert got.dtype == np.float32 and got.shape == (8, 750, 64) and np.array_equal(got, small.float().numpy())
    big = torch.arange(8 * 2 * 96000, dtype=torch.float32).reshape(8, 2, 96000)   # 6 MB against a 1 MB cap; every value distinct
    for name in ("a", "b"):
        bench.dump_output(str(tmp_path), name, big, 1 << 20)
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert a.dtype == np.float32 and a.nbytes <= 1 << 20 and a.shape == (8, (1 << 20) // 32)
    assert np.array_equal(a, b)   # the same positions every time
    flat = big.reshape(8, -1).numpy()
    idx = (a[0] - flat[0, 0]).astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(flat[:, idx], a)   # the same positions of every item, in order


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tiny", "--duration", "4", "--infer-steps", "4",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_plain_full_and_dump(gpu_device, tmp_path):
    plain = _bench(tmp_path / "a")
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(plain)
    assert not {"roofline", "cpu_baseline", "box_probe", "gpu_state_under_load"} & set(plain)
    full = _bench(tmp_path / "b", "--full", "--no-cpu-baseline")
    assert "roofline" in full and full["roofline"]["gemm_launches_per_pass"] > 0
    a, b = np.load(tmp_path / "a" / "audio.npy"), np.load(tmp_path / "b" / "audio.npy")
    assert a.dtype == np.float32 and a.shape[:2] == (8, 2) and np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a, b), "same arguments, same inputs: the dumped outputs of two runs differ"
