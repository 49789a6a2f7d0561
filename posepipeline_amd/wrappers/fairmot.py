"""Drop-in for pose_pipeline/wrappers/fairmot.py:64-141 `fairmot_bounding_boxes`.

Same signature and the same return structure: one list per decoded frame of
    {"track_id": int, "tlbr": ndarray(4,) x1y1x2y2, "tlhw": ndarray(4,) [x, y, w, h], "confidence": float}
(the key really is spelled `tlhw` and holds x, y, w, h, :126-132).  The reference runs FairMOT's `JDETracker.update` once per frame:
one DLA-34 pass gives boxes and 128-d identity embeddings, no second ReID network.  Upstream needs the CUDA-only DCNv2 extension
(DCNv2_PATH next to FAIRMOT_PATH); here the clip is streamed to the device in batches (streaming.FrameStreamer), pre-processing,
the network (models/dla.py: PP_OP_DCN3X3 / PP_OP_DWDECONV of csrc/fairmot.hip) and the decode run batched on the GPU, and the strictly
sequential association (tracking.JDETracker) runs on the host.

Reference behaviour kept (FairMOT and DCNv2 are not vendored: everything below is restated and UNPINNED):
  * EVERY FRAME IS FIRST RESIZED TO 1920 x 1080, whatever the source size: upstream `LoadVideo` hard-codes self.w, self.h = 1920, 1080
    (cv2.resize, INTER_LINEAR).  That is why the reference multiplies by xscale = width / 1920 and yscale = height / 1080
    (:101-103, :131-132).  All tracker arithmetic happens in that 1920 x 1080 frame; boxes are rescaled only when the dicts are built.
  * Network size 1088 x 608 (w x h), or 608 x 1088 when the source has height > width (:82-83) -- the frame is still squeezed to
    1920 x 1080 first, then letterboxed (INTER_AREA, border 127.5 -> 128), RGB / 255, no mean / std.
  * The min_box_area and "vertical" filters are dead code (`if True:`, :123): every activated track is reported.
  * BaseTrack._count = 0 per call (:106): ids start at 1 in every call.
  * Settings that matter at inference: K = 500, conf_thres = 0.2, down_ratio = 4, ltrb = True, reg_offset = True, reid_dim = 128,
    track_buffer = 30, head_conv = 256, heads hm 1 / wh 4 / id 128 / reg 2; nms_thres, mean and std are not used at inference.
    The tracker's frame rate is LoadVideo's int(round(fps)).
  * Decoded boxes go back to the 1920 x 1080 frame by CenterNet's transform_preds: c = (960, 540), s = max(wp / hp * 1080, 1920),
    output size (wp / 4, hp / 4); the matrix is built CenterNet's way (float32 triangles, third point by rotation,
    cv2.getAffineTransform = a float64 6 x 6 solve), applied in float64 and stored as float32; then score > 0.2.

Checkpoint: fairmot/fairmot_dla34.pth under MODEL_DATA_DIR (keys and shapes checked, a `module.` prefix dropped);
POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded parameters (models/dla.synth_dla34_state_dict).

BATCH = 4 frames per pass: the activation arena of the 608 x 1088 program is 343 MB per frame (models/dla.activation_bytes_per_frame;
base_layer and level0 alone are 16 channels at full resolution, 42 MB each, a 256-channel head map another 42 MB), so 4 frames keep
the arena at 1.4 GB and the small maps still fill the chip (the smallest DCN map, 19 x 34, gives 11 tiles per frame, 44 per pass).
"""
from __future__ import annotations

import time

import numpy as np

from .. import _lib, ops
from ..models import dla
from ..program import Net
from ..tracking import JDETracker
from ..video import open_video

BATCH = 4
K = 500
CONF_THRES = 0.2
TRACK_BUFFER = 30
FRAME_W, FRAME_H = 1920, 1080          # LoadVideo's hard-coded size
_cache: dict = {}
last_timing: dict = {}                 # per-stage wall milliseconds of the most recent call


def _third_point(a, b):
    d = a - b
    return b + np.array([-d[1], d[0]], np.float32)


def transform_matrix(hp: int, wp: int) -> np.ndarray:
    """CenterNet get_affine_transform(c, s, 0, (wp / 4, hp / 4), inv=1) for the 1920 x 1080 frame -> 2 x 3 float64"""
    c = np.array([FRAME_W / 2.0, FRAME_H / 2.0], np.float32)
    s = max(float(wp) / float(hp) * FRAME_H, FRAME_W) * 1.0
    scale = np.array([s, s], np.float32)
    dst_w, dst_h = wp // dla.DOWN_RATIO, hp // dla.DOWN_RATIO
    src_dir = np.array([0.0, scale[0] * -0.5])                       # get_dir(..., rot_rad = 0)
    dst_dir = np.array([0, dst_w * -0.5], np.float32)
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0] = c
    src[1] = c + src_dir
    dst[0] = [dst_w * 0.5, dst_h * 0.5]
    dst[1] = np.array([dst_w * 0.5, dst_h * 0.5], np.float32) + dst_dir
    src[2] = _third_point(src[0], src[1])
    dst[2] = _third_point(dst[0], dst[1])
    # cv2.getAffineTransform(dst, src): the 6 x 6 system in float64
    a = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        a[2 * i, 0:3] = [dst[i, 0], dst[i, 1], 1.0]
        a[2 * i + 1, 3:6] = [dst[i, 0], dst[i, 1], 1.0]
        b[2 * i], b[2 * i + 1] = src[i, 0], src[i, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def transform_preds(coords, trans) -> np.ndarray:
    """CenterNet affine_transform of float32 points [n][2] with the float64 matrix -> float64 [n][2]"""
    pts = np.concatenate([np.asarray(coords, np.float32), np.ones((len(coords), 1), np.float32)], 1)
    return pts.astype(np.float64) @ trans.T


def post_process(dets, hp, wp):
    """[K][5] float32 boxes in heat-map cells -> float32 boxes in the 1920 x 1080 frame (both corners through transform_preds)"""
    trans = transform_matrix(hp, wp)
    out = np.asarray(dets, np.float32).copy()
    out[:, 0:2] = transform_preds(out[:, 0:2], trans).astype(np.float32)
    out[:, 2:4] = transform_preds(out[:, 2:4], trans).astype(np.float32)
    return out


class FairMOTDetector:
    """pre-processing -> DLA-34 -> decode for chunks of frames of one source size"""

    def __init__(self, ctx, sd, src_h, src_w, max_frames=BATCH, numerics=None):
        self.ctx, self.src = ctx, (int(src_h), int(src_w))
        self.hp, self.wp = ops.fairmot_input_size(src_h, src_w)[:2]
        self.prog = dla.build_dla34_program(sd, self.hp, self.wp)
        self.net = Net(ctx, self.prog, max_batch=max_frames, numerics=numerics)
        self.max_frames = max_frames
        self.ms = dict(pre=0.0, net=0.0, decode=0.0)

    def run(self, frames, frames_dev=None):
        """-> per frame (dets [m][5] float32 x1 y1 x2 y2 score in the 1920 x 1080 frame, score > 0.2, descending; feats [m][128])"""
        din = self.net.buffer("input")[0]
        t0 = time.perf_counter()
        if frames_dev is not None:
            ptr, n = frames_dev
            ops.fairmot_preprocess(self.ctx, int(ptr), din, frames_dev_shape=(n,) + self.src)
        else:
            n = len(frames)
            ops.fairmot_preprocess(self.ctx, frames, din)
        assert 0 < n <= self.max_frames
        t1 = time.perf_counter()
        self.net.run(n)
        self.ctx.synchronize()
        t2 = time.perf_counter()
        h, w = self.hp // dla.DOWN_RATIO, self.wp // dla.DOWN_RATIO
        dets, feats, _ = ops.fairmot_decode(self.ctx, *[self.net.buffer(k)[0] for k in ("hm", "wh", "reg", "id")], n, h, w, min(K, h * w))
        out = []
        for f in range(n):
            d = post_process(dets[f], self.hp, self.wp)
            keep = d[:, 4] > np.float32(CONF_THRES)
            out.append((d[keep], feats[f][keep]))
        t3 = time.perf_counter()
        for k, v in (("pre", t1 - t0), ("net", t2 - t1), ("decode", t3 - t2)):
            self.ms[k] += v * 1e3
        return out


def _detector(src_h, src_w, device=0):
    key = (src_h, src_w, device)
    if key not in _cache:
        ctx = _lib.Context(device)
        _cache[key] = (ctx, FairMOTDetector(ctx, dla.get_state_dict(), src_h, src_w))
    return _cache[key]


def fairmot_bounding_boxes(file_path):
    from ..streaming import FrameStreamer
    cap = open_video(file_path)
    video_length = int(cap.num_frames)
    width, height = int(cap.width), int(cap.height)
    tracks = []
    if video_length <= 0:
        cap.release()
        return tracks
    ctx, det = _detector(height, width)
    det.ms = dict(pre=0.0, net=0.0, decode=0.0)
    to_source = np.array([width / FRAME_W, height / FRAME_H] * 2)       # the reference's xscale, yscale (:101-103)
    tracker = JDETracker(frame_rate=int(round(cap.fps)), conf_thres=CONF_THRES, track_buffer=TRACK_BUFFER)      # ids from 1 in every call
    host_ms = 0.0
    t_all = time.perf_counter()
    streamer = FrameStreamer(ctx, cap, min(BATCH, video_length), max_frames=video_length)
    try:
        for dev_ptr, n, _first in streamer:
            per_frame = det.run(None, frames_dev=(dev_ptr, n))
            streamer.release()
            t0 = time.perf_counter()
            for dets, feats in per_frame:
                rows = []
                for track_id, tlwh, score in tracker.step(dets, feats):
                    box = tlwh * to_source                       # x, y, w, h in source pixels
                    rows.append({"track_id": int(track_id), "tlbr": np.r_[box[:2], box[:2] + box[2:]], "tlhw": box,
                                 "confidence": float(score)})
                tracks.append(rows)
            host_ms += (time.perf_counter() - t0) * 1e3
    finally:
        streamer.close()
        cap.release()
    last_timing.clear()
    last_timing.update(det.ms, tracker=host_ms, total=(time.perf_counter() - t_all) * 1e3, frames=len(tracks))
    return tracks
