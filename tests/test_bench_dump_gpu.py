"""`bench.py --dump-outputs DIR`: the last timed step's losses and a fixed sample of its updated parameters and gradients, as float32
.npy files under 64 MB, from inputs that are the same on every run -- two runs with the same arguments compute the same bits (the
reported loss sums, accumulated with float atomics, to the last bit; they feed nothing back into the step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(d):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "VK_BENCH_DRY_RUN"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "8", "--steps", "3", "--warmup", "1", "--no-kernel-timing",
                        "--no-cpu-baseline", "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    return out, {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_of_two_runs_agree(tmp_path):
    out, a = _bench(tmp_path / "a")
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert sorted(a) == ["grads_sample", "losses", "params_sample"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["params_sample"].shape == a["grads_sample"].shape and a["grads_sample"].any()
    assert (a["losses"] == np.float32(out["losses_last_step"])).all()
    _, b = _bench(tmp_path / "b")
    assert np.allclose(a["losses"], b["losses"], rtol=1e-6, atol=0)
    for k in ("params_sample", "grads_sample"):
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))
