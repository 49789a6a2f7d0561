#!/usr/bin/env python
"""Golden vectors of the hand-box stage, by RUNNING the reference's own `make_bbox_from_keypoints`.

Runs only where a checkout of the reference (peabody124/PosePipeline) exists; tests/golden/hand_bbox.npz, which it writes
next to this script, is committed and is what tests/test_hand_stage.py reads.  Nothing here copies reference source:
pose_pipeline/wrappers/hand_bbox.py is loaded by file path (with empty stand-ins for the `cv2` and `datajoint` imports at its
top, and a `pose_pipeline` module that has the `Video` attribute it imports), called on seeded inputs, and inputs + outputs
are stored.

Inputs: Halpe-136 tracks (T, 136, 3) float64.  Uniformly random keypoints are useless -- almost every hand would fall back to
the fixed box -- so each hand is 21 points clustered within ~80 px of a centre well inside a 1920x1080 frame, plus the edge
cases the contract has: right-only / left-only fallback (a hand hanging over the top or left edge), an absent person's all-zero
row, and a hand within 60 px of an edge whose POINTS are all inside the frame.  The mix is asserted on the reference's OUTPUT
before anything is written.

usage: python tests/golden/make_goldens_hand.py <reference checkout>      (deterministic; rewrites hand_bbox.npz)
"""
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
FALLBACK = np.array([0.0, 0.0, 2040.0, 1500.0])


def load_reference(ref):
    for name in ("cv2", "datajoint"):
        sys.modules.setdefault(name, types.ModuleType(name))
    pp = types.ModuleType("pose_pipeline")
    pp.Video = object
    sys.modules["pose_pipeline"] = pp
    spec = importlib.util.spec_from_file_location("ref_hand_bbox", os.path.join(ref, "pose_pipeline", "wrappers", "hand_bbox.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hand(rng, centre, spread=80.0):
    return np.asarray(centre, np.float64) + rng.uniform(-spread, spread, (21, 2))


def make_track(rng, n=32, width=120):
    kp = np.zeros((n, 136, 3), np.float64)
    kp[:, :94, :2] = 500.0              # body / face / feet joints and the scores are not read by the hand boxes: constants keep
    kp[:, :, 2] = 0.9                   # the fixture small
    for t in range(n):
        kp[t, 94:115, :2] = hand(rng, rng.uniform((300, 300), (1600, 800)))       # left hand
        kp[t, 115:136, :2] = hand(rng, rng.uniform((300, 300), (1600, 800)))      # right hand
    kp[3, 115:136, :2] = hand(rng, (30.0, 500.0))       # right hand over the left edge: right-only fallback
    kp[4, 94:115, :2] = hand(rng, (700.0, 20.0))        # left hand over the top edge: left-only fallback
    kp[5] = 0.0                                         # person absent in this frame: both boxes fall back
    kp[6, 115:136, :2] = hand(rng, (70.0, 600.0), 40.0)     # every point inside the frame, but x_min - width / 2 < 0: falls back
    kp[7, 94:115, :2] = hand(rng, (150.0, 145.0), 80.0)     # near the top-left corner: keeps its own box at the default size
    kp[8, 115:136, :2] = np.round(hand(rng, (900.0, 500.0)))    # integer coordinates
    kp[8, 115, :2] = (width / 2, 700.0)                         # x_min - width / 2 == 0 exactly: not negative, no fallback
    return kp


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(20240521)
    out = {}
    for name, kw in (("a", {}), ("b", {"width": 90, "height": 150})):
        kp = make_track(rng, width=kw.get("width", 120))
        boxes = ref.make_bbox_from_keypoints(kp, **kw)
        assert isinstance(boxes, list) and len(boxes) == len(kp) and all(len(b) == 2 for b in boxes)
        arr = np.array(boxes)
        assert arr.shape == (len(kp), 2, 4) and arr.dtype == np.float64
        fb = (arr == FALLBACK).all(axis=2)                      # [frame][right, left]
        assert (~fb).all(axis=1).sum() >= len(kp) // 2, "at least half of the rows have both hands non-fallback"
        assert (fb[:, 0] & ~fb[:, 1]).any() and (~fb[:, 0] & fb[:, 1]).any(), "right-only and left-only fallback rows"
        assert fb[5].all() and not kp[5].any(), "the absent person's row"
        pts = kp[6, 115:136, :2]
        assert fb[6, 0] and (pts >= 0).all() and pts[:, 0].min() < min(60, kw.get("width", 120) / 2), "a hand within 60 px of the left edge"
        assert not fb[8, 0] and arr[8, 0, 0] == 0.0
        out[f"kp_{name}"] = kp
        out[f"boxes_{name}"] = arr
        out[f"wh_{name}"] = np.array([kw.get("width", 120), kw.get("height", 120)], np.int64)
    np.savez_compressed(os.path.join(OUT, "hand_bbox.npz"), **out)
    print("wrote hand_bbox.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
