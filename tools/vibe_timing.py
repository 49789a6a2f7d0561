#!/usr/bin/env python
"""Times of the SMPL stage (DESIGN_LOG.md 5m): per-stage device milliseconds of the VIBE path -- crop, backbone, GRU, regressor, SMPL --
for a synthetic track (default 256 present frames of a 640 x 480 clip held on the device), by HIP events on the context's stream
(`Context.timer_start` / `timer_stop` around each stage's launches; the stages run one after the other, so the figures add up).

usage: python tools/vibe_timing.py [--out FILE] [--frames 256] [--reps 3] [--numerics exact split]     (needs an MI355X; synthetic weights)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("POSEPIPE_SYNTHETIC_WEIGHTS", "1")

from posepipeline_amd import _lib as L                                    # noqa: E402
from posepipeline_amd import ops                                          # noqa: E402
from posepipeline_amd.models import vibe as vm                            # noqa: E402
from posepipeline_amd.wrappers import vibe as W                           # noqa: E402


def time_track(ctx, numerics, n, reps, height=480, width=640, chunk=32):
    rng = np.random.default_rng(0)
    model = W.VibeModel(ctx=ctx, numerics=numerics)
    frames = rng.integers(0, 256, (chunk, height, width, 3), dtype=np.uint8)
    boxes = np.stack([rng.uniform(100, 300, n), rng.uniform(50, 150, n), rng.uniform(80, 200, n), rng.uniform(150, 300, n)], axis=1)
    _, mats = W.crop_matrices(boxes)
    frames_dev = ctx.malloc(frames.nbytes)
    padded = -(-n // vm.SEQ) * vm.SEQ
    feat_dev = ctx.malloc(padded * vm.FEAT * 4)
    in_ptr, out_ptr = model.backbone.buffer("input")[0], model.backbone.buffer("features")[0]
    best = None
    try:
        ctx.h2d(frames_dev, frames)
        ctx.h2d(feat_dev, np.zeros((padded, vm.FEAT), np.float32))
        for _ in range(reps + 1):                                   # the first pass warms up
            ms = {"crop": 0.0, "backbone": 0.0}
            for i0 in range(0, n, W.BACKBONE_BATCH):
                k = min(W.BACKBONE_BATCH, n - i0)
                idx = np.arange(k, dtype=np.int32) % chunk
                ctx.timer_start()
                ops.warp_affine_normalize_each(ctx, frames_dev, idx, mats[i0:i0 + k], (W.CROP_SIZE, W.CROP_SIZE), model.lut, W.CHAN_MAP,
                                               out_dev=in_ptr, frames_dev_shape=(chunk, height, width))
                ms["crop"] += ctx.timer_stop()
                ctx.timer_start()
                model.backbone.run(k)
                ctx.d2d(feat_dev + i0 * vm.FEAT * 4, out_ptr, k * vm.FEAT * 4)
                ms["backbone"] += ctx.timer_stop()
            model.run_head(feat_dev, n, want_verts=False, timed=True)
            ms.update(zip(("gru", "regressor", "smpl"), (float(v) for v in model.stage_ms)))
            if best is None or sum(ms.values()) < sum(best.values()):
                best = ms
    finally:
        ctx.free(frames_dev)
        ctx.free(feat_dev)
        numerics_built = model.head.numerics
        model.close()
    total = sum(best.values())
    return {"track": f"{n} present frames, {width}x{height}", "numerics": numerics_built, "sequences": padded // vm.SEQ,
            "ms": {k: round(v, 3) for k, v in best.items()}, "ms_total": round(total, 3), "frames_per_s_device": round(n / total * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numerics", nargs="+", default=["exact", "split"])
    a = ap.parse_args()
    ctx = L.Context(0)
    rows = []
    for numerics in a.numerics:
        rows.append(time_track(ctx, numerics, a.frames, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
