"""Drop-in for pose_pipeline/wrappers/hand_bbox.py: the boxes the hand stage crops.

`make_bbox_from_keypoints` (reference :80-105, the "TopDown" method of the HandBbox table) turns the last 42 joints of a
Halpe-136 track (TopDownPerson with top_down_method=2, MMPoseHalpe) into one right-hand and one left-hand box per frame.
The contract is the reference's, quirks included: right hand = the last 21 joints, left = the 21 before them; a box is the
min / max of the hand's points -/+ half of (width, height); a hand with ANY negative box coordinate -- a hand near the top
or left edge as much as an absent person's all-zero row -- gets the fixed box [0, 0, 2040, 1500]; the result is a per-frame
list [right (4,), left (4,)] of xyxy float64.  Written here as array operations over the whole track (the reference loops
over frames); pinned against the reference's output by tests/golden/hand_bbox.npz.

`mmpose_hand_det` (the "RTMDet" method) is not built: RTMDet is another model family.
"""
from __future__ import annotations

import numpy as np

FALLBACK_BOX = (0.0, 0.0, 2040.0, 1500.0)


def mmpose_hand_det(key, method='RTMDet'):
    raise NotImplementedError(f"hand detection method {method!r} (RTMDet-nano hand detector) is not built; "
                              "use the HandBbox method 'TopDown' (boxes from Halpe keypoints)")


def make_bbox_from_keypoints(keypoints=[], width=120, height=120):
    kp = np.asarray(keypoints)
    n = kp.shape[0]
    hands = kp[:, -42:, :2].reshape(n, 2, 21, 2)               # [frame][left, right][joint][x, y]
    xs, ys = hands[..., 0], hands[..., 1]
    # min(p - w/2) == min(p) - w/2 bit for bit (rounding is monotonic), in the track's own dtype as the reference computes it
    boxes = np.stack([xs.min(axis=2) - width / 2, ys.min(axis=2) - height / 2,
                      xs.max(axis=2) + width / 2, ys.max(axis=2) + height / 2], axis=2).astype(np.float64)
    boxes[(boxes < 0).any(axis=2)] = FALLBACK_BOX
    return [[boxes[i, 1].copy(), boxes[i, 0].copy()] for i in range(n)]
