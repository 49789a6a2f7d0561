#!/usr/bin/env python
"""Times of the TraDeS stage (DESIGN_LOG.md 5o): frames per second of `trades_bounding_boxes` on a 1080p clip with per-stage wall
milliseconds (pre, program A, CVA, render, program B, decode, tracker), program B's per-frame latency with its launch count, and
`pp_trades_cva` at 60 x 108 (the 864 x 480 input) per frame pair beside two yardsticks:
  (a) the cost volume's 2 * 6480 * 6480 * 128 = 10.7 GFLOP at the float32-input MFMA rate measured on this chip (155 TFLOP/s);
  (b) a torch evaluation of the upstream formulation on the same device: matmul, two maxima, two softmaxes, two expectations -- it
      writes and re-reads the 168 MB volume (recorded as missing where torch has no device);
  (c) a non-fused evaluation from this project's own kernels, a LOWER bound of any materialising formulation: the volume written by
      the float32-MFMA convolution kernel (a 1x1 convolution 128 -> 6480 whose weight is the previous frame's embeddings: the same
      product, stored) plus one device copy of the volume, which moves the bytes the two maxima passes would at least read.
The wrapper is timed twice: as it runs in production (frames per second) and with a synchronisation after every stage (the table).

usage: python tools/trades_timing.py [--out FILE] [--frames 16] [--numerics exact split]     (needs an MI355X; synthetic weights)
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
from posepipeline_amd import ops, video                                   # noqa: E402
from posepipeline_amd.models import trades as T                           # noqa: E402
from posepipeline_amd.program import Net                                  # noqa: E402
from posepipeline_amd.wrappers import trades as W                         # noqa: E402

F32_MFMA_TFLOPS = 155.0


def cva_timing(ctx, hc, wc, pairs, reps):
    rng = np.random.default_rng(0)
    emb = (rng.standard_normal((pairs + 1, hc, wc, 128)) * 0.2).astype(np.float32)
    nb = emb[0].nbytes
    d_emb = ctx.malloc(emb.nbytes)
    d_off = ctx.malloc(pairs * 4 * hc * wc * 2 * 4)
    ctx.h2d(d_emb, emb)
    ms = []
    for _ in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        ops.trades_cva_dev(ctx, d_emb + nb, d_emb, pairs, hc, wc, d_off)
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    off = np.empty((pairs, 2 * hc, 2 * wc, 2), np.float32)
    ctx.d2h(off, d_off)
    ctx.free(d_emb)
    ctx.free(d_off)
    row = {"shape": f"{hc}x{wc}", "pairs": pairs, "ms_per_pair_fused": min(ms[1:]) / pairs,
           "ms_per_pair_at_mfma_rate": 2.0 * (hc * wc) ** 2 * 128 / (F32_MFMA_TFLOPS * 1e9)}
    row.update(unfused_floor(ctx, emb, hc, wc, reps))
    try:
        import torch
        te = torch.from_numpy(emb).cuda()
        iq, jq = np.divmod(np.arange(hc * wc), wc)
        th = torch.from_numpy((2 * (np.arange(hc)[None, :] - iq[:, None])).astype(np.float32)).cuda()
        tw = torch.from_numpy((2 * (np.arange(wc)[None, :] - jq[:, None])).astype(np.float32)).cuda()

        def upstream(cur, prev):
            c = torch.matmul(cur.reshape(-1, 128), prev.reshape(-1, 128).t()).reshape(hc * wc, hc, wc)
            sh = torch.softmax(5 * c.max(dim=2)[0], dim=1)
            sw = torch.softmax(5 * c.max(dim=1)[0], dim=1)
            return torch.stack([(sw * tw).sum(1), (sh * th).sum(1)], -1)
        tms = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = [upstream(te[p + 1], te[p]) for p in range(pairs)]
            torch.cuda.synchronize()
            tms.append((time.perf_counter() - t0) * 1e3)
        ref = outs[0].cpu().numpy().reshape(hc, wc, 2)
        row["ms_per_pair_torch"] = min(tms[1:]) / pairs
        row["max_abs_diff_to_torch"] = float(np.abs(off[0][::2, ::2] - ref).max())
    except Exception as e:           # torch without a device: the yardstick is reported as missing, never replaced
        row["ms_per_pair_torch"] = None
        row["torch_error"] = repr(e)
    return row


def unfused_floor(ctx, emb, hc, wc, reps):
    """yardstick (c) for one pair: materialise c[q][key] with the project's float32 convolution kernel, then copy it once"""
    from posepipeline_amd.program import ProgramBuilder
    P = hc * wc
    pb = ProgramBuilder()
    x = pb.buf(hc, wc, 128, name="cur")
    pb.mark_output(pb.conv(x, emb[0].reshape(P, 128, 1, 1), None, name="volume"), "volume")
    net = Net(ctx, pb.build(), 1, numerics="exact")
    ctx.h2d(net.buffer("cur")[0], emb[1])
    vol, nbytes, _ = net.buffer("volume")
    copy = ctx.malloc(nbytes)
    ms_mm, ms_cp = [], []
    for _ in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        net.run(1)
        ctx.synchronize()
        t1 = time.perf_counter()
        ctx.d2d(copy, vol, nbytes)
        ctx.synchronize()
        ms_mm.append((t1 - t0) * 1e3)
        ms_cp.append((time.perf_counter() - t1) * 1e3)
    got = np.empty((1, hc, wc, P), np.float32)
    ctx.d2h(got, vol)
    ref = emb[1].reshape(P, 128).astype(np.float64) @ emb[0].reshape(P, 128).astype(np.float64).T
    ctx.free(copy)
    net.close()
    return {"volume_mb": nbytes / 1e6, "ms_materialise": min(ms_mm[1:]), "ms_copy_volume": min(ms_cp[1:]),
            "ms_per_pair_unfused_floor": min(ms_mm[1:]) + min(ms_cp[1:]), "volume_max_abs_err": float(np.abs(got.reshape(P, P) - ref).max())}


def program_b_latency(ctx, sd, numerics, reps):
    net = Net(ctx, T.build_program_b(sd, 120, 216), 1, numerics=numerics)
    rng = np.random.default_rng(1)
    for name in ("feat_cur", "feat_prev", "tracking_offset", "pre_hm"):
        _, _, dims = net.buffer(name)
        ctx.h2d(net.buffer(name)[0], rng.standard_normal(dims).astype(np.float32))
    ms = []
    for _ in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        net.run(1)
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    net.set_lanes(False)
    per_op = np.array([net.profile(1) for _ in range(reps + 1)])[1:].min(axis=0)
    out = {"numerics": net.numerics, "launches": len(net.prog.ops), "ms_wall": min(ms[1:]), "ms_sum_of_ops": float(per_op.sum()),
           "ops": dict(zip(net.prog.op_names, [round(float(v), 4) for v in per_op]))}
    net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numerics", nargs="+", default=["split"])
    args = ap.parse_args()
    result = {"cva": [], "program_b": [], "wrapper": []}
    ctx = L.Context(0)
    for pairs in (1, 4):
        result["cva"].append(cva_timing(ctx, 60, 108, pairs, args.reps))
        print(json.dumps(result["cva"][-1]), flush=True)
    sd = T.get_state_dict()
    for numerics in args.numerics:
        result["program_b"].append(program_b_latency(ctx, sd, numerics, args.reps))
        print(json.dumps(result["program_b"][-1]), flush=True)
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (args.frames, 1080, 1920, 3), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clip.ppvid")
        video.write_ppvid(path, frames, 30.0)
        for rep, staged in enumerate((False, False, True)):      # the first call builds the programs and loads the kernels
            W.STAGE_TIMING = staged
            tracks = W.trades_bounding_boxes(path)
            t = dict(W.last_timing)
            row = {"call": rep, "stage_synchronised": staged, "frames": t["frames"], "fps": t["frames"] / t["total"] * 1e3,
                   "detections": sum(len(f) for f in tracks)}
            if staged:
                row["ms_per_frame"] = {k: t[k] / t["frames"] for k in W.STAGES}
            result["wrapper"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
