#!/usr/bin/env python
"""Device times of the PoseFormer lifter (DESIGN_LOG.md 5k): per numerics and channel padding, a 300-frame and a 3 000-frame clip split
into spatial kernel / gather / temporal program / mean + head (HIP events inside pp_poseformer_lift), the temporal program's
conv_kinds, and the spatial stage in the reference's form -- recomputed for every window, 81 frames per window -- next to the
once-per-frame form the lifter runs.

usage: python tools/poseformer_timing.py [--out FILE] [--reps 9] [--max-windows 64]     (needs an MI355X; synthetic weights)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from posepipeline_amd import _lib as L                                    # noqa: E402
from posepipeline_amd.models import poseformer as M                       # noqa: E402
from posepipeline_amd.wrappers import poseformer as W                     # noqa: E402


def spatial_ms(ctx, d_params, n_frames, reps):
    """the spatial kernel alone over n_frames frames resident on the device: HIP-event milliseconds, best of `reps` after a warm-up"""
    x = np.random.default_rng(1).uniform(0, 1, (n_frames, 17, 2)).astype(np.float32)
    d_x, d_f = ctx.malloc(x.nbytes), ctx.malloc(n_frames * 544 * 4)
    try:
        ctx.h2d(d_x, x)
        times = []
        for r in range(reps + 1):
            ctx.timer_start()
            L.check(ctx.lib.pp_poseformer_spatial(ctx.handle, L.ptr(d_params), L.ptr(d_x), n_frames, L.PP_MEM_DEVICE, L.ptr(d_f)), "pp_poseformer_spatial")
            times.append(ctx.timer_stop())
        return min(times[1:])
    finally:
        ctx.free(d_x)
        ctx.free(d_f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--max-windows", type=int, default=64)
    ap.add_argument("--frames", type=int, nargs="+", default=[300, 3000])
    a = ap.parse_args()
    ctx = L.Context(0)
    spec = M.PoseFormerSpec()
    sd = M.synth_params(M.poseformer_param_shapes(spec), seed=11)
    rng = np.random.default_rng(0)
    clips = {n: rng.uniform(0, 1, (n, 17, 2)).astype(np.float32) for n in a.frames}
    rows = []
    # the four forms side by side: all built and warmed up first, then timed in ALTERNATION (one call of each per round), so that a
    # drift of the clock or of the shared host hits every form alike; per form the spread over the rounds is reported with the minimum
    forms = [(numerics, pad) for numerics in ("exact", "split") for pad in (0, 128)]
    lifters = {f: W.PoseFormerLifter(max_windows=a.max_windows, numerics=f[0], ctx=ctx, state_dict=sd, channel_pad=f[1]) for f in forms}
    for n, x in clips.items():
        for lf in lifters.values():
            lf.lift(x)                                       # warm-up of every shape the timed calls use
        runs = {f: [] for f in forms}
        for _ in range(a.reps):
            for f in forms:
                lifters[f].lift(x, timed=True)
                runs[f].append(lifters[f].stage_ms.copy())
        for f in forms:
            lf, r = lifters[f], np.array(runs[f])
            tot = r.sum(axis=1)
            best = r[int(tot.argmin())]
            kinds = lf.net.conv_kinds()
            rows.append({"numerics": lf.net.numerics, "split_kind": lf.net.split_kind, "channel_pad": f[1], "frames": n, "windows": n - 80,
                         "ms_spatial": float(best[0]), "ms_gather": float(best[1]), "ms_temporal": float(best[2]),
                         "ms_mean_head": float(best[3]), "ms_total": float(tot.min()), "ms_total_median": float(np.median(tot)),
                         "ms_total_max": float(tot.max()), "rounds": a.reps, "conv_kinds": kinds[kinds > 0].tolist()})
            print(json.dumps(rows[-1]), flush=True)
    for lf in lifters.values():
        lf.close()
    # the spatial stage in the reference's form: every window evaluates its 81 frames again
    block = M.spatial_param_block(spec, sd)
    d_params = ctx.malloc(block.nbytes)
    ctx.h2d(d_params, block)
    for n in a.frames:
        rows.append({"spatial_only_frames": n, "ms_once_per_frame": spatial_ms(ctx, d_params, n, a.reps),
                     "ms_per_window_form": spatial_ms(ctx, d_params, 81 * (n - 80), a.reps), "frames_per_window_form": 81 * (n - 80)})
        print(json.dumps(rows[-1]), flush=True)
    ctx.free(d_params)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
