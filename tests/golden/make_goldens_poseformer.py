#!/usr/bin/env python
"""Golden vectors of the PoseFormer wrapper's pre- and post-processing, by RUNNING the reference's own `process_liftformer`.

Runs only where a checkout of the reference (peabody124/PosePipeline) exists; tests/golden/poseformer_pre.npz, which it writes next
to this script, is committed and is what tests/test_poseformer.py reads.  Nothing here copies reference source:
pose_pipeline/wrappers/poseformer.py is loaded by file path and called on seeded clips, with stand-ins for what it imports and
touches around the network:
  * `pose_pipeline`: TopDownPerson / VideoInfo objects that answer `& key` and `fetch1`, and MODEL_DATA_DIR;
  * `pose_pipeline.env.add_path` and `tqdm`: no-ops;
  * `common.model_poseformer.PoseTransformer`: a parameter-free nn.Module whose forward RECORDS its input and returns the call
    index in every element of a (1, 1, 17, 3) tensor -- the network itself is not part of the reference tree;
  * `torch.load`, `Tensor.cuda` / `Module.cuda` and `torch.cuda.empty_cache`: no checkpoint, no device.
What is stored is therefore exactly what the reference feeds the network (COCO -> H36M conversion, the division by (height, width),
the float32 rounding of torch.Tensor, the windows) and how it assembles the returned array.

Two clips of N = 84 frames (4 windows each), one with width > height and one with height > width; key points are float32 inside
the frame.

usage: python tests/golden/make_goldens_poseformer.py <reference checkout>      (deterministic; rewrites poseformer_pre.npz)
"""
import contextlib
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
N = 84


class _Table:
    """`(Table & key).fetch1(*names)` over one row"""

    def __init__(self, row):
        self.row = row

    def __and__(self, key):
        return self

    def fetch1(self, *names):
        vals = tuple(self.row[n] for n in names)
        return vals[0] if len(vals) == 1 else vals


def load_reference(ref, tables, recorded):
    import torch
    import torch.nn as nn

    class PoseTransformer(nn.Module):
        def __init__(self, **kw):
            super().__init__()
            recorded["kwargs"] = dict(kw)

        def forward(self, x):
            recorded["inputs"].append(x.detach().clone())
            return torch.full((x.shape[0], 1, 17, 3), float(len(recorded["inputs"]) - 1))

    pp = types.ModuleType("pose_pipeline")
    pp.MODEL_DATA_DIR = "/nonexistent"
    pp.TopDownPerson = tables["TopDownPerson"]
    pp.VideoInfo = tables["VideoInfo"]
    env = types.ModuleType("pose_pipeline.env")
    env.add_path = lambda path: contextlib.nullcontext()
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    common = types.ModuleType("common")
    mp = types.ModuleType("common.model_poseformer")
    mp.PoseTransformer = PoseTransformer
    common.model_poseformer = mp
    sys.modules.update({"pose_pipeline": pp, "pose_pipeline.env": env, "tqdm": tq, "common": common, "common.model_poseformer": mp})
    torch.load = lambda *a, **k: {"model_pos": {}}
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self
    torch.cuda.empty_cache = lambda: None
    os.environ.setdefault("POSEFORMER_PATH", "/nonexistent")
    spec = importlib.util.spec_from_file_location("ref_poseformer", os.path.join(ref, "pose_pipeline", "wrappers", "poseformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_clip(rng, height, width):
    kp = np.empty((N, 17, 3), np.float32)
    centre = rng.uniform((0.3 * width, 0.3 * height), (0.7 * width, 0.7 * height))
    kp[..., :2] = (centre + rng.uniform(-0.25, 0.25, (N, 17, 2)) * (width, height)).astype(np.float32)
    kp[..., 2] = rng.uniform(0.3, 1.0, (N, 17)).astype(np.float32)
    assert (kp[..., 0] > 0).all() and (kp[..., 0] < width).all() and (kp[..., 1] > 0).all() and (kp[..., 1] < height).all()
    return kp


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rng = np.random.default_rng(20241018)
    tables = {"TopDownPerson": _Table({}), "VideoInfo": _Table({})}
    recorded = {"inputs": []}
    ref = load_reference(sys.argv[1], tables, recorded)
    out = {}
    for name, (height, width) in (("a", (1080, 1920)), ("b", (1280, 720))):
        kp = make_clip(rng, height, width)
        tables["TopDownPerson"].row = {"keypoints": kp}
        tables["VideoInfo"].row = {"height": height, "width": width}
        recorded["inputs"].clear()
        key = {"video_project": "golden", "filename": name}
        before = dict(key)
        res = ref.process_liftformer(key)
        assert res is key and set(res) - set(before) == {"keypoints_3d"} and all(res[k] == v for k, v in before.items())
        wins = np.stack([t.numpy() for t in recorded["inputs"]])
        k3 = res["keypoints_3d"]
        assert wins.shape == (N - 80, 1, 81, 17, 2) and wins.dtype == np.float32, (wins.shape, wins.dtype)
        assert k3.shape == (N, 17, 3) and k3.dtype == np.float64
        assert not k3[:40].any() and not k3[N - 40:].any()
        assert all((k3[40 + i] == i).all() for i in range(N - 80))
        out[f"kp_{name}"] = kp
        out[f"hw_{name}"] = np.array([height, width], np.int64)
        out[f"windows_{name}"] = wins[:, 0]
        out[f"k3d_{name}"] = k3
    kw = recorded["kwargs"]
    assert (kw["num_frame"], kw["num_joints"], kw["in_chans"], kw["embed_dim_ratio"], kw["depth"], kw["num_heads"], kw["mlp_ratio"],
            kw["qkv_bias"]) == (81, 17, 2, 32, 4, 8, 2.0, True), kw
    np.savez_compressed(os.path.join(OUT, "poseformer_pre.npz"), **out)
    print("wrote poseformer_pre.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
