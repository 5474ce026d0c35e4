"""bench.py's plain run and `--dump-outputs`: the plain line carries the
headline alone (no CPU baseline, no secondary lines, no work-counter replay),
the dumped arrays are what the last timed step returned, run after run, and
timing window after window (bench.ACTION_BYTES) walks the same trajectory as
holding every step's actions resident."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"obs_blue": (4096, 4, 68), "obs_red": (4096, 4, 68), "rew_blue": (4096, 4),
          "rew_red": (4096, 4), "done": (4096,), "cog": (4096,)}


def test_plain_run_dumps_last_step(tmp_path):
    import bench
    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--global-envs", "4096", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert line["unit"] == "env-steps/sec" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(4096 * 3 / (line["ms_per_step"] * 3 / 1e3), rel=1e-9)
    assert line["err_envs"] == 0
    assert line["cpu_baseline"] is None and "secondary" not in line and "los_work" not in line
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in SHAPES)
    got = {k: np.load(d / (k + ".npy")) for k in SHAPES}
    assert {k: v.shape for k, v in got.items()} == SHAPES
    assert all(v.dtype == np.float32 for v in got.values())
    assert line["outputs"] == {k: list(s) for k, s in SHAPES.items()}
    assert np.abs(got["obs_blue"]).sum() > 0 and np.abs(got["obs_red"]).sum() > 0
    # the same arguments in this process: the same inputs, the same arrays
    res = bench.run_workload(4096, 0, "reference", 0, 0, 3, 2, count_work=False, outputs=True)
    for k in SHAPES:
        assert np.array_equal(got[k], res["outputs"][k], equal_nan=True), k


@pytest.mark.parametrize("spawns", ["reference", "melee"])
def test_windows_walk_the_same_trajectory(spawns, monkeypatch):
    """11 timed steps after 6 warmup steps with 4 action sets resident at a
    time (windows of 4, 2 and 4, 4, 3 steps) against all of them resident."""
    import bench
    E = 512
    whole = bench.run_workload(E, 0, spawns, 0, 0, 11, 6, digest=True, outputs=True)
    monkeypatch.setattr(bench, "ACTION_BYTES", 4 * E * 8 * 4 * 4)
    parts = bench.run_workload(E, 0, spawns, 0, 0, 11, 6, digest=True, outputs=True)
    assert np.array_equal(whole["digest"], parts["digest"])
    for k in SHAPES:
        # (cog is NaN where the reference returns None)
        assert np.array_equal(whole["outputs"][k], parts["outputs"][k], equal_nan=True), k
    assert whole["err"] == parts["err"] == 0 and parts["elapsed"] > 0 and parts["kernel_ms"] > 0
