#!/usr/bin/env python
"""Records tests/golden/trades_e2e.npz: the TraDeS chain of tests/trades_ref.py (pre-processing -> float64 network -> decode ->
TrackerRef) on two seeded 8-frame clips, landscape 64 x 96 and portrait 96 x 64 (so that the 480 x 864 swap runs), at the full
network size, together with the same chain with every network layer in float32.  Per frame: the ids, boxes (source pixels) and scores of
both chains; per clip the margins the test relies on:
  score_margin   the smallest |score - 0.5| over every decoded peak of every frame, either chain (out_thresh = new_thresh = pre_thresh)
  score_dev      the largest |score32 - score64| over the peaks both chains decoded
  gap_margin     the smallest of: best-to-second-best gap of every greedy row, and |dist - area| of every (detection, track) gate [px^2]
  gap_dev        the largest |dist32 - dist64| + |area32 - area64| over the same entries
The script asserts that both margins clear FACTOR = 4 times their deviation and that the two chains agree on ids and membership in every
frame -- no frame is left out; a seed that fails is not recorded.  Takes about ten minutes on 8 cores (a float64 trunk pass at
480 x 864 is 12 s).

usage: python tests/golden/make_goldens_trades.py [--seed-landscape 0] [--seed-portrait 3] [--frames 8] [--cache DIR]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import preprocess as OP                                  # noqa: E402
from posepipeline_amd.models import trades as T                       # noqa: E402
from tests import fairmot_ref as F                                    # noqa: E402
from tests import trades_ref as R                                     # noqa: E402

FACTOR = 4.0


def record(sd, name, h, w, seed, n_frames, out, cache_dir=None):
    frames = F.rectangles_clip(n_frames, h, w, seed=seed)
    cache = {}
    cache_file = os.path.join(cache_dir, f"trades_trunk_{name}_{seed}_{n_frames}.npz") if cache_dir else None
    if cache_file and os.path.exists(cache_file):           # the trunk does not depend on the heads being tuned: keep it between runs
        z = np.load(cache_file)
        cache = {(f, dt): (z[f"feat_{f}_{dt}"], z[f"emb_{f}_{dt}"]) for f in range(n_frames) for dt in ("float64", "float32")}
    r64, p64, t64 = R.chain(sd, frames, np.float64, OP, T.MEAN, T.STD, trunk_cache=cache)
    r32, p32, t32 = R.chain(sd, frames, np.float32, OP, T.MEAN, T.STD, trunk_cache=cache)
    if cache_file and not os.path.exists(cache_file):
        np.savez(cache_file, **{f"{k}_{f}_{dt}": v[i] for (f, dt), v in cache.items() for i, k in enumerate(("feat", "emb"))})
    print(name, "ids per frame:", [[i for i, _, _ in fr] for fr in r64], flush=True)
    assert [[i for i, _, _ in fr] for fr in r64] == [[i for i, _, _ in fr] for fr in r32], "the float32 chain numbers the tracks differently"
    score_margin = min(abs(s - 0.5) for p in p64 + p32 for s in p.values())
    score_dev = max(abs(a[i] - b[i]) for a, b in zip(p64, p32) for i in a if i in b)
    gaps, devs = [], []
    for l64, l32 in zip(t64.log, t32.log):
        assert l64["dist"].shape == l32["dist"].shape
        if l64["dist"].size:
            d64, d32 = l64["dist"].astype(np.float64), l32["dist"].astype(np.float64)
            devs.append(np.abs(d64 - d32).max() + max(np.abs(l64[k].astype(np.float64) - l32[k]).max() for k in ("track_area", "det_area")))
            for lg in (l64, l32):
                d = lg["dist"].astype(np.float64)
                gaps.append(np.abs(d - lg["track_area"][None, :]).min())
                gaps.append(np.abs(d - lg["det_area"][:, None]).min())
                for row in lg["rows"]:
                    ok = np.sort(row[row < 1e16])
                    if len(ok) >= 2:
                        gaps.append(ok[1] - ok[0])
    for f, lg in enumerate(t64.log):
        if lg["dist"].size:
            print(f"  frame {f}: dist {np.round(lg['dist'], 1).tolist()} track areas {np.round(lg['track_area'], 1).tolist()}", flush=True)
    gap_margin, gap_dev = float(min(gaps)), float(max(devs))
    print(f"{name}: score margin {score_margin:.3e} vs deviation {score_dev:.3e}; gap margin {gap_margin:.3e} vs deviation {gap_dev:.3e}", flush=True)
    assert score_margin > FACTOR * score_dev and gap_margin > FACTOR * gap_dev, "choose another seed"
    n_boxes = sum(len(fr) for fr in r64)
    persisting = len({i for fr in r64 for i, _, _ in fr}) < n_boxes
    assert n_boxes > 0 and persisting, "no detection clears 0.5, or none keeps its id"
    out[f"{name}_seed"], out[f"{name}_frames"], out[f"{name}_size"] = seed, n_frames, np.array([h, w])
    out[f"{name}_score_margin"], out[f"{name}_score_dev"] = score_margin, score_dev
    out[f"{name}_gap_margin"], out[f"{name}_gap_dev"] = gap_margin, gap_dev
    for f in range(n_frames):
        out[f"{name}_ids{f}"] = np.array([i for i, _, _ in r64[f]], np.int64)
        for tag, rows in (("64", r64), ("32", r32)):
            out[f"{name}_bbox{tag}_{f}"] = np.array([b for _, b, _ in rows[f]], np.float64).reshape(-1, 4)
            out[f"{name}_score{tag}_{f}"] = np.array([s for _, _, s in rows[f]], np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed-landscape", type=int, default=0)
    ap.add_argument("--seed-portrait", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--cache", help="directory that keeps the trunk outputs between runs (not part of the repository)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "trades_e2e.npz"))
    args = ap.parse_args()
    sd = T.synth_trades_state_dict(T.trades_param_shapes(), 11)
    out = {}
    record(sd, "landscape", 64, 96, args.seed_landscape, args.frames, out, args.cache)
    record(sd, "portrait", 96, 64, args.seed_portrait, args.frames, out, args.cache)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
