#!/usr/bin/env python
"""Throughput of the SkeletonAction stage (PoseC3D) at full size on one GPU, with synthetic weights: windows per second and the stage
split (targets, front, gather, trunk, head), in both numerics, with the front-stage de-duplication on and off in ALTERNATING runs on
the same device, and a sweep of the clips per pass.  One JSON line per measurement.

    python tools/posec3d_timing.py [--windows 8] [--repeats 3] [--sweep 1,2,4,10,20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from posepipeline_amd import _lib  # noqa: E402
from posepipeline_amd.models import posec3d as pm  # noqa: E402
from posepipeline_amd.wrappers import mmaction as W  # noqa: E402


def track(n, seed=0):
    rng = np.random.default_rng(seed)
    kp = np.zeros((n, 17, 3), np.float32)
    base = np.stack([rng.uniform(500, 900, 17), rng.uniform(200, 900, 17)], axis=1)
    for t in range(n):
        kp[t, :, :2] = base + rng.normal(0, 4, (17, 2)) + t * np.array([3.0, 1.0])
        kp[t, :, 2] = rng.uniform(0.3, 1.0, 17)
    return kp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sweep", default="1,2,4,10,20")
    ap.add_argument("--numerics", default="exact,split")
    args = ap.parse_args()
    spec = pm.PoseC3DSpec()
    sd = pm.synth_params(pm.posec3d_param_shapes(spec), 11)
    kp, shape = track(49 + args.windows), (1080, 1920)
    ctx = _lib.Context(0)
    progs = pm.build_programs(spec, sd)[0]
    flop = ((progs["front"].flops + progs["frame"].flops) * spec.clip_len + progs["clip"].flops) * 2 * W.NUM_CLIPS
    print(json.dumps(dict(what="sizes", flop_per_window_plain=flop, activation_bytes_per_clip=pm.activation_bytes_per_clip(spec, progs),
                          clips_per_pass_default=pm.clips_per_pass(spec, 2 * W.NUM_CLIPS, progs),
                          front_bytes_per_frame=pm.front_bytes_per_frame(progs), args=vars(args))), flush=True)

    def measure(model, tag):
        model.timing = False
        model.scores(kp[:51], shape)                                   # warm-up: one window
        rates = []
        for _ in range(args.repeats):
            model.scores(kp, shape)
            rates.append(model.last_timing["windows"] / model.last_timing["total_s"])
        model.timing = True
        model.scores(kp, shape)
        t = model.last_timing
        stages = {k: round(t[k] / t["windows"], 3) for k in ("targets", "front", "gather", "trunk", "head")}
        print(json.dumps(dict(tag, windows_per_s=[round(r, 2) for r in rates], best=round(max(rates), 2), stage_ms_per_window=stages,
                              clips_per_pass=model.clips_per_pass)), flush=True)
        return max(rates)

    for numerics in args.numerics.split(","):
        models = {d: W.SkeletonActionModel(ctx=ctx, numerics=numerics, state_dict=sd, spec=spec, dedup=d) for d in (True, False)}
        for rnd in range(2):                                           # alternating: on, off, on, off
            for d in (True, False):
                measure(models[d], dict(what="dedup", numerics=models[d].net.numerics, dedup=d, round=rnd))
        for m in models.values():
            m.close()
        for cpp in [int(v) for v in args.sweep.split(",") if v]:
            m = W.SkeletonActionModel(ctx=ctx, numerics=numerics, state_dict=sd, spec=spec, dedup=True, clips_per_pass=cpp)
            measure(m, dict(what="clips_per_pass", numerics=m.net.numerics, dedup=True))
            m.close()
    ctx.close()


if __name__ == "__main__":
    main()
