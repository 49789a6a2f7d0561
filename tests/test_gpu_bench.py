"""bench.py's plain line and --dump-outputs on the real cascade: the line holds the headline fields and none of what is
measured outside the timed steps (that is --full), and two runs with the same arguments dump the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "POSEPIPE_CONV_EXACT"):
        env.pop(k, None)       # the bench's own numerics (the default kernels), one rank
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *args],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench("--dump-outputs", str(a))
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(line["config"]["frames_per_step_per_gpu"] * 1e3 / line["ms_per_step"])
    for k in ("roofline", "bit_exact_mode", "integer_exact_mode", "pcie_inclusive", "cpu_baseline", "secondary"):
        assert k not in line, k
    _bench("--dump-outputs", str(b))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"tracks.npy", "keypoints.npy", "keypoints_index.npy", "keypoints_3d.npy", "keypoints_3d_index.npy"} <= set(names)
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert np.array_equal(x, y), n
    # 3 chunks of 64 frames: the 2D rows of the last step and 3D rows past the lifting window's half-width (121 frames)
    assert len(np.load(a / "keypoints.npy")) > 0 and len(np.load(a / "keypoints_3d.npy")) > 0
    assert len(np.load(a / "keypoints.npy")) == len(np.load(a / "keypoints_index.npy"))
