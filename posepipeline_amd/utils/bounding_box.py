"""Box arithmetic of the SMPL stage: pose_pipeline/utils/bounding_box.py:7-29 and :56-98, the same float64 operations.

`fix_bb_aspect_ratio` makes a TLWH box the wanted aspect ratio around its centre and dilates it; the two `convert_*` functions
(adopted by the reference from VIBE's demo_utils) take the weak-perspective camera and the normalised 2-D joints of a square crop
back to the original image.  Kept quirk: both read `h = bbox[:, 2]`, the box WIDTH -- the boxes are square by then.

The crop itself (`crop_image_bbox`, `get_person_dataloader`) runs on the device: wrappers/vibe.py.
"""
from __future__ import annotations

import numpy as np


def fix_bb_aspect_ratio(bbox, dilate=1.2, ratio=1.0):
    """bbox (4,) TLWH -> (4,) TLWH with width / height = ratio, containing the box, scaled by `dilate` about its centre"""
    bbox = np.asarray(bbox)
    center = bbox[:2] + bbox[2:] / 2.0
    w, h = bbox[2], bbox[3]
    # a box narrower than the ratio grows in width, any other in height (:22-26)
    size = np.array([h * ratio, h]) if w / h < ratio else np.array([w, w / ratio])
    size = size * dilate
    return np.concatenate([center - size / 2, size], axis=0)


def _square_box_frame(bbox):
    """centre (cx, cy) and side of the (square) boxes [n][4] TLWH; the side is column 2, as the reference reads it"""
    bbox = np.asarray(bbox)
    return bbox[:, 0] + bbox[:, 2] / 2, bbox[:, 1] + bbox[:, 3] / 2, bbox[:, 2]


def convert_crop_cam_to_orig_img(cam, bbox, img_width, img_height):
    """weak-perspective camera (s, tx, ty) [n][3] of the crop -> (sx, sy, tx, ty) [n][4] of the original image"""
    cam = np.asarray(cam)
    cx, cy, side = _square_box_frame(bbox)
    hw, hh = img_width / 2.0, img_height / 2.0
    sx = cam[:, 0] * (1.0 / (img_width / side))
    sy = cam[:, 0] * (1.0 / (img_height / side))
    tx = ((cx - hw) / hw / sx) + cam[:, 1]
    ty = ((cy - hh) / hh / sy) + cam[:, 2]
    return np.stack([sx, sy, tx, ty]).T


def convert_crop_coords_to_orig_img(bbox, keypoints, crop_size):
    """joints [n][k][2] in [-1, 1] of the crop -> pixels of the original image (a new array; the reference also returns a new one)"""
    cx, cy, side = _square_box_frame(bbox)
    keypoints = 0.5 * crop_size * (np.asarray(keypoints) + 1.0)          # to crop pixels
    keypoints *= side[..., None, None] / crop_size                        # to the box's scale
    keypoints[:, :, 0] = (cx - side / 2)[..., None] + keypoints[:, :, 0]
    keypoints[:, :, 1] = (cy - side / 2)[..., None] + keypoints[:, :, 1]
    return keypoints
