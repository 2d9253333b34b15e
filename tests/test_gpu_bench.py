"""bench.py on the GPU at a small batch: a plain run prints the headline line
without the --full extras, --steps sets the timed epochs, and --dump-outputs
writes the state the timed path left, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS, WARMUP = 1501, 9, 2  # more than the dump's sample; an odd batch: the last instance takes the one-instance kernel


def _bench(*extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--batch-per-gpu", str(B)] + list(extra), capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_every_time(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    l1, l2 = _bench("--dump-outputs", d1), _bench("--dump-outputs", d2)
    for ln in (l1, l2):
        assert "cpu_baseline" not in ln and ln["collective_check"] is None
        assert ln["steps"] == STEPS and ln["warmup"] == WARMUP and ln["dtype"] == "f64"
        assert ln["unit"] == "steps/s" and ln["higher_is_better"] is True and ln["metric"] == bench.METRIC
        assert ln["ms_per_step"] > 0
        # value and ms_per_step are the same measurement: instance-epochs over the timed window's wall time
        assert ln["value"] == pytest.approx(B * STEPS / (ln["ms_per_step"] * 1e-3 * STEPS), rel=1e-9)
        assert ln["dumped_outputs"] == ["ensemble_stats", "sample_instances", "state_cov", "state_mean", "status"]
    total = 0
    for name in l1["dumped_outputs"]:
        u, v = np.load(os.path.join(d1, name + ".npy")), np.load(os.path.join(d2, name + ".npy"))
        assert u.dtype == np.float64 and np.array_equal(u, v), name
        total += u.nbytes
    assert total < 64 << 20
    mean, cov = np.load(os.path.join(d1, "state_mean.npy")), np.load(os.path.join(d1, "state_cov.npy"))
    idx = np.load(os.path.join(d1, "sample_instances.npy")).astype(np.int64)
    assert mean.shape == (B, 54) and cov.shape == (bench.DUMP_SAMPLE, 53, 53)
    assert np.array_equal(idx, bench.dump_sample(B))
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))
    assert np.allclose(cov, cov.transpose(0, 2, 1), rtol=1e-12, atol=1e-300)
    assert np.all(np.einsum("bii->bi", cov) > 0)
    assert not np.load(os.path.join(d1, "status.npy")).any()

