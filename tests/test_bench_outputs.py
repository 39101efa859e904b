"""bench.py without --full: the headline line only, and --dump-outputs writes what the timed path computed.  The timed steps multiply
a by b in place, so after the untimed first step, W warm-up and K timed steps every element of a is a0 * b^(1 + W + K); the dumped
sample is checked element for element against the oracle's product chain."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_and_dumps_the_last_step(tmp_path):
    import oracle_lib as O

    batch, steps, warmup, k = 64, 3, 2, 16
    env = {key: v for key, v in os.environ.items() if key not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(batch), "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "ring-muls/s" and d["higher_is_better"] is True and d["dtype"] == "u64" and d["steps"] == steps
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - batch) < 1e-6 * batch
    assert not {"roofline", "parity", "cpu_baseline", "clock_power", "integer_valu", "multi_gpu"} & set(d)

    c = np.load(os.path.join(str(tmp_path), "c.npy"))
    d_ = 1 << k
    n = (32 << 20) // (d_ * 16)
    assert c.dtype == np.float64 and c.shape == (n, d_, 2) and c.nbytes <= 64 << 20
    got = c[..., 0].astype(np.uint64) | (c[..., 1].astype(np.uint64) << np.uint64(32))
    idx = np.sort(np.random.default_rng(0x5EED0003).choice(batch, size=n, replace=False))
    F = O.GOLDILOCKS
    want = np.concatenate([O.fill_uniform(F, 0x5EED0001, int(e) * d_, d_) for e in idx])
    b = np.concatenate([O.fill_uniform(F, 0x5EED0002, int(e) * d_, d_) for e in idx])
    for _ in range(1 + warmup + steps):
        want = O.pow2_ring_mul(F, want, b, k, n, 8)
    assert np.array_equal(got.reshape(-1), want)
