"""bench.py command line: result line, --dump-outputs, --full (CPU
llama-tiny path; the GPU run differs only in model size and dtype)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--device", "cpu", "--steps", "2", "--warmup", "1", *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=120,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_repeatable_and_full_flag(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = _bench("--dump-outputs", a)
    out_full = _bench("--dump-outputs", b, "--full")

    for o in (out, out_full):
        assert o["metric"] == "train_samples_per_sec"
        assert o["higher_is_better"] is True
        assert o["unit"] == "samples/s" and o["dtype"] == "fp32"
        assert o["steps"] == 2 and o["warmup"] == 1
        assert o["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps
        sps = o["config"]["global_batch"] / (o["ms_per_step"] / 1000)
        assert abs(sps - o["value"]) <= 1e-2 * o["value"]

    assert sorted(os.listdir(a)) == ["loss.npy", "param_sample.npy"]
    total = 0
    for name in os.listdir(a):
        x = np.load(os.path.join(a, name))
        y = np.load(os.path.join(b, name))
        assert x.dtype == np.float32 and x.size > 0
        assert np.isfinite(x).all()
        # same arguments -> same inputs -> same outputs, run to run
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= 64 * 1024 * 1024
    loss = np.load(os.path.join(a, "loss.npy"))
    assert loss.shape == (1,)
    assert abs(float(loss[0]) - out["config"]["final_loss"]) < 1e-3
