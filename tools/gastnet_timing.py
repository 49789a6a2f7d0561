#!/usr/bin/env python
"""Times of the GAST-Net lifter (DESIGN_LOG.md 5p): `GastNetLifter.lift` on a clip of 1 000 valid frames (the rf = 27 model, chunks of
256 frames, flip augmentation: two samples per chunk) with its per-stage milliseconds -- upload and program are device times (HIP
events around the copies and around the program's launches, summed over the chunks), post is the host's share (download, flip merge;
wall) -- and `Net.profile` of one chunk by op type, lanes off, so that the two new ops stand beside the convolutions.

With `--persons P --step N` (DESIGN_LOG.md 5q) it times the streamed cascade's lifting step instead: P tracks that each gain N valid
frames per call, so every call lifts P segments of N + 2 pad frames (the new frames and their halo).  Per chunk length 8 / 16 / 32 / 64
it prints the milliseconds per call of the one-call device path (`GastNetLifter.lift_many`: pp_gastnet_lift_many) beside the
per-person host path (`camera_to_world(lift(x))` in a loop over the persons) on the same lifter, in the same run, after checking
that both give the same bytes.

usage: python tools/gastnet_timing.py [--out FILE] [--frames 1000] [--numerics exact split]     (needs an MI355X; synthetic weights)
       python tools/gastnet_timing.py --persons 4 --step 8 [--chunks 8 16 32 64] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("POSEPIPE_SYNTHETIC_WEIGHTS", "1")

from posepipeline_amd import _lib as L                                    # noqa: E402
from posepipeline_amd.wrappers import gastnet as W                        # noqa: E402

OP_NAMES = {L.PP_OP_CONV: "conv", L.PP_OP_GRAPH_MIX: "graph_mix", L.PP_OP_JOINT_ATTN: "joint_attn"}


def streaming_step(a):
    """--persons P --step N: ms per call of lift_many against lift in a loop, per chunk length"""
    from posepipeline_amd.models import gastnet as gn
    rng = np.random.default_rng(0)
    rows = []
    ctx = L.Context(0)
    for numerics in a.numerics:
        for chunk in a.chunks:
            spec = gn.GastNetSpec(chunk=chunk)
            n = a.step + 2 * spec.pad
            items = -(-n // chunk)
            xs = [rng.uniform(-1, 1, (n, 17, 2)).astype(np.float32) for _ in range(a.persons)]
            lf = W.GastNetLifter(ctx=ctx, numerics=numerics, spec=spec, max_batch=2 * a.persons * items)
            many = lf.lift_many(xs)                                      # warm-up of both paths, and the same bytes from both
            loop = [W.camera_to_world(lf.lift(x)) for x in xs]
            assert all(np.array_equal(m, h) for m, h in zip(many, loop)), "lift_many differs from the host chain"
            t_many, t_loop = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                lf.lift_many(xs)
                t_many.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                for x in xs:
                    W.camera_to_world(lf.lift(x))
                t_loop.append((time.perf_counter() - t0) * 1e3)
            rows.append({"lifter": "GastNetLifter rf=27 channels=128", "numerics": lf.net.numerics, "persons": a.persons, "step": a.step,
                         "frames_per_segment": n, "chunk": chunk, "items_per_person": items, "max_batch": lf.net.max_batch,
                         "lift_many_ms_per_call": round(float(np.median(t_many)), 3), "lift_many_ms_min": round(min(t_many), 3),
                         "lift_loop_ms_per_call": round(float(np.median(t_loop)), 3), "lift_loop_ms_min": round(min(t_loop), 3)})
            print(json.dumps(rows[-1]), flush=True)
            lf.close()
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numerics", nargs="+", default=["exact", "split"])
    ap.add_argument("--persons", type=int, default=None, help="with --step: time the streamed cascade's lifting step")
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 16, 32, 64])
    a = ap.parse_args()
    if (a.persons is None) != (a.step is None):
        ap.error("--persons and --step go together")
    if a.persons is not None:
        rows = streaming_step(a)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        return
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (a.frames, 17, 2)).astype(np.float32)
    rows = []
    ctx = L.Context(0)
    for numerics in a.numerics:
        lf = W.GastNetLifter(ctx=ctx, numerics=numerics)
        lf.lift(x)                                                       # warm-up
        walls, stages = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            lf.lift(x)
            walls.append((time.perf_counter() - t0) * 1e3)
            lf.lift(x, timed=True)
            stages.append(dict(lf.stage_ms))
        best = min(stages, key=lambda s: s["program"])
        prog = lf.net.prog
        lf.net.set_lanes(False)
        ms = np.array([lf.net.profile(2) for _ in range(a.reps + 1)])[1:].min(axis=0)
        by_type = {}
        for op, m in zip(prog.ops, ms):
            name = OP_NAMES.get(int(op.type), str(int(op.type)))
            by_type[name] = by_type.get(name, 0.0) + float(m)
        kinds = lf.net.conv_kinds()
        rows.append({"lifter": "GastNetLifter rf=27 channels=128", "numerics": lf.net.numerics, "split_kind": lf.net.split_kind,
                     "frames": a.frames, "chunk": lf.spec.chunk, "chunks": -(-a.frames // lf.spec.chunk), "wall_ms": min(walls),
                     "frames_per_s": a.frames / min(walls) * 1e3, "stage_ms": {k: round(v, 3) for k, v in best.items()},
                     "chunk_profile_ms_by_op": {k: round(v, 3) for k, v in by_type.items()}, "chunk_profile_ms_total": round(float(ms.sum()), 3),
                     "ops": len(prog.ops), "convs_split": int((kinds == 2).sum()), "convs_f32": int((kinds == 1).sum()),
                     "gflop_per_chunk": round(2 * prog.flops * 1e-9, 2)})
        print(json.dumps(rows[-1]), flush=True)
        lf.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
