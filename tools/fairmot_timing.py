#!/usr/bin/env python
"""Times of the FairMOT stage (DESIGN_LOG.md 5l): frames per second of `fairmot_bounding_boxes` on a 1080p clip with per-stage wall
milliseconds, `Net.profile` per op of the 608 x 1088 DLA-34 program at batch 1 and at the wrapper's batch, and for every DCN shape the
time of PP_OP_DCN3X3 beside an ordinary 3x3 PP_OP_CONV of the same shape in the same net numerics (the yardstick: the same
multiply-adds without sampling), with the achieved FLOP rate from 2 * 9 * cin * cout * h * w.

usage: python tools/fairmot_timing.py [--out FILE] [--frames 16] [--numerics exact split]     (needs an MI355X; synthetic weights)
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("POSEPIPE_SYNTHETIC_WEIGHTS", "1")

from posepipeline_amd import _lib as L                                    # noqa: E402
from posepipeline_amd import video                                        # noqa: E402
from posepipeline_amd.models import dla                                   # noqa: E402
from posepipeline_amd.program import Net, ProgramBuilder                  # noqa: E402
from posepipeline_amd.wrappers import fairmot as W                        # noqa: E402

DCN_SHAPES = [(512, 256, 19, 34), (256, 256, 38, 68), (256, 128, 38, 68), (256, 64, 38, 68), (128, 128, 76, 136), (128, 64, 76, 136),
              (64, 64, 152, 272)]


def dcn_vs_conv(ctx, numerics, batch, reps):
    rows = []
    rng = np.random.default_rng(0)
    for cin, cout, h, w in DCN_SHAPES:
        pb = ProgramBuilder()
        x = pb.buf(h, w, cin, name="x")
        wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
        om = pb.conv(x, (rng.standard_normal((27, cin, 3, 3)) * 0.05).astype(np.float32), np.zeros(27, np.float32), pad=1, name="offset_mask")
        pb.mark_output(pb.dcn3x3(x, om, wt, np.zeros(cout, np.float32), relu=L.PP_RELU_LAST, name="dcn"), "y")
        pb.mark_output(pb.conv(x, wt, np.zeros(cout, np.float32), pad=1, relu=L.PP_RELU_LAST, name="conv"), "c")
        prog = pb.build()
        net = Net(ctx, prog, batch, numerics=numerics)
        net.set_lanes(False)
        ctx.h2d(net.buffer("x")[0], rng.standard_normal((batch, h, w, cin)).astype(np.float32))
        ms = np.array([net.profile(batch) for _ in range(reps + 1)])[1:].min(axis=0)
        t = dict(zip(prog.op_names, ms.tolist()))
        flop = 2.0 * 9 * cin * cout * h * w * batch
        rows.append({"shape": f"{cin}->{cout} at {h}x{w}", "batch": batch, "numerics": net.numerics, "conv_kind": int(net.conv_kinds()[prog.op_names.index("conv")]),
                     "ms_dcn": t["dcn"], "ms_conv": t["conv"], "ms_offset_mask": t["offset_mask"], "dcn_over_conv": t["dcn"] / t["conv"],
                     "dcn_tflops": flop / t["dcn"] * 1e-9, "conv_tflops": flop / t["conv"] * 1e-9})
        print(json.dumps(rows[-1]), flush=True)
        net.close()
    return rows


def net_profile(ctx, sd, numerics, batch, reps):
    prog = dla.build_dla34_program(sd, 608, 1088)
    net = Net(ctx, prog, batch, numerics=numerics)
    net.set_lanes(False)
    ms = np.array([net.profile(batch) for _ in range(reps + 1)])[1:].min(axis=0)
    by_type = {}
    for op, m in zip(prog.ops, ms):
        by_type[int(op.type)] = by_type.get(int(op.type), 0.0) + float(m)
    row = {"program": "dla34 608x1088", "numerics": net.numerics, "batch": batch, "ms_total": float(ms.sum()), "ms_by_op_type": by_type,
           "gflop_per_frame": prog.flops * 1e-9, "arena_mb_per_frame": dla.activation_bytes_per_frame(prog) / 1e6,
           "ops": [{"name": n, "ms": float(m)} for n, m in zip(prog.op_names, ms)]}
    print(json.dumps({k: v for k, v in row.items() if k != "ops"}), flush=True)
    net.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numerics", nargs="+", default=["exact", "split"])
    a = ap.parse_args()
    rows = []
    rng = np.random.default_rng(0)
    clip = rng.integers(0, 256, (a.frames, 1080, 1920, 3), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "clip.ppvid")
        video.write_ppvid(path, clip, 30.0)
        W.fairmot_bounding_boxes(path)                           # warm-up: builds the net
        t0 = time.perf_counter()
        tracks = W.fairmot_bounding_boxes(path)
        dt = time.perf_counter() - t0
    rows.append({"wrapper": "fairmot_bounding_boxes 1080p", "frames": len(tracks), "batch": W.BATCH, "fps": len(tracks) / dt,
                 "stage_ms": dict(W.last_timing), "boxes": int(sum(len(f) for f in tracks))})
    print(json.dumps(rows[-1]), flush=True)
    ctx, det = next(iter(W._cache.values()))
    sd = dla.get_state_dict()
    for numerics in a.numerics:
        for batch in (1, W.BATCH):
            rows.append(net_profile(ctx, sd, numerics, batch, a.reps))
        rows += dcn_vs_conv(ctx, numerics, 1, a.reps)
        rows += dcn_vs_conv(ctx, numerics, W.BATCH, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
