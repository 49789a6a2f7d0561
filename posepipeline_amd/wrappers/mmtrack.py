"""Drop-in for pose_pipeline/wrappers/mmtrack.py:8-62 `mmtrack_bounding_boxes`.

Same signature and the same return structure: one list per decoded frame of
    {"track_id": int, "tlbr": ndarray(4,) x1y1x2y2, "tlhw": ndarray(4,) [x1, y1, w, h], "confidence": float}
(the key really is spelled `tlhw`, :50-60).  The reference calls `mmtrack.apis.inference_mot` once per
frame; here the clip is streamed to the device in batches, the detector runs batched on the GPU and the strictly
sequential association runs on the host.

Built:
  "deepsort"   mot/deepsort/deepsort_faster-rcnn_fpn_4e_mot17-private-half.py, the configuration the reference selects
               (wrappers/mmtrack.py:16-19): Faster-RCNN R50-FPN (pp_detector) + mmtrack SortTracker WITH its ReID
               appearance branch -- ResNet-50 ReID model on 256x128 crops of the detector's input tensor
               (models/reid_r50.py), Kalman gating, appearance then IoU assignment (tracking.SortReidTracker; the
               NaN-gated assignment is given an explicit reading there).  POSEPIPE_MMTRACK_REID=0 drops the appearance
               branch (= the sort_faster-rcnn configuration of the same directory, pp_tracker mode 1);
  "bytetrack"  YOLOX-X (models/yolox.py) + mmtrack ByteTracker (tracking.ByteTracker) of
               mot/bytetrack/bytetrack_yolox_x_crowdhuman_mot17-private.py -- restated from mmdet / mmtrack 0.x, unpinned.
  "tracktor"   mot/tracktor/tracktor_faster-rcnn_r50_fpn_4e_mot17-private-half.py, the reference wrapper's DEFAULT method (:8, :12-15):
               the same Faster-RCNN R50-FPN (checkpoint of the -private config) and ResNet-50 ReID model, and mmtrack's
               TracktorTracker (tracking.TracktorTracker): tracks are propagated by regressing their boxes through the detector's RoI
               head on the next frame (Detector.regress, on the FPN maps the chunk's detector pass left on the device), after
               camera-motion compensation -- cv2.findTransformECC(MOTION_EUCLIDEAN, 100 iterations, eps 1e-5) between consecutive
               network-input tensors, here ONE device call per chunk over all its frame pairs (csrc/ecc.hip; the gray plane of the
               chunk's last frame stays on the device for the pair across the chunk boundary).  The map is estimated between the
               network-input tensors and applied to boxes in source pixels, as the configuration does with rescale=True.  A frame
               pair on which ECC fails (NaN correlation, non-positive lambda denominator) raises RuntimeError naming the frame; the
               reference dies in cv2.error there.  Restated from mmtrack 0.x / OpenCV, unpinned.
qdtrack uses another model family and raises NotImplementedError.  Unknown names raise Exception like the reference (:28-29).
"""
from __future__ import annotations

import numpy as np

import os

import time

from .. import _lib, ops, weights
from ..models import faster_rcnn as fr
from ..tracking import ByteTracker, SortReidTracker, Tracker, TracktorTracker
from ..video import open_video

BATCH = 16
BATCH_YOLOX = 4          # 800 x 1440 inputs: 1.4 GB of activations per frame
_KNOWN = ("tracktor", "deepsort", "bytetrack", "qdtrack")
_cache: dict = {}
ECC_ITERS, ECC_EPS = 100, 1e-5      # CameraMotionCompensation(num_iters, stop_eps) of the tracktor config (:47-50)
last_timing: dict = {}              # tracktor: per-stage wall milliseconds and ECC iteration counts of the most recent call


def _detector(src_h, src_w, device=0, method="deepsort"):
    key = (src_h, src_w, device, method)
    if key not in _cache:
        ctx = _lib.Context(device)
        if method == "bytetrack":
            from ..models import yolox
            # init_cfg of mot/bytetrack/*-private-half.py:16-20: the COCO YOLOX-X checkpoint of mmdetection
            rel = "mmtracking/checkpoints/yolox_x_8x8_300e_coco_20211126_140254-1ef88d67.pth"
            sd = weights.get_state_dict(rel, yolox.yolox_param_shapes(), seed=6)
            if not os.path.exists(os.path.join(weights.model_data_dir(), rel)):
                yolox.seed_synthetic_head(sd)           # seeded weights: keep the candidate count realistic
            _cache[key] = (ctx, yolox.YoloXDetector(ctx, sd, src_h, src_w, max_frames=BATCH_YOLOX))
        elif method == "tracktor":
            from ..models import reid_r50
            # the -private config's overrides (:6-9 detector, :11-14 reid)
            sd = weights.get_state_dict("mmtracking/checkpoints/faster-rcnn_r50_fpn_4e_mot17-ffa52ae7.pth",
                                        fr.faster_rcnn_param_shapes(), seed=2)
            det = fr.Detector(ctx, sd, src_h, src_w, max_frames=BATCH)
            rsd = weights.get_state_dict("mmtracking/checkpoints/reid_r50_6e_mot17-4bf6b63d.pth", reid_r50.reid_param_shapes(), seed=7)
            det.reid = reid_r50.ReidEncoder(ctx, rsd, det)
            _cache[key] = (ctx, det)
        else:
            sd = weights.get_state_dict("mmtracking/checkpoints/faster-rcnn_r50_fpn_4e_mot17-half-64ee2ed4.pth",
                                        fr.faster_rcnn_param_shapes(), seed=2)
            det = fr.Detector(ctx, sd, src_h, src_w, max_frames=BATCH)
            if method == "deepsort" and os.environ.get("POSEPIPE_MMTRACK_REID", "1") != "0":
                from ..models import reid_r50
                # init_cfg of the config's reid section (:39-42)
                rsd = weights.get_state_dict("mmtracking/checkpoints/tracktor_reid_r50_iter25245-a452f51f.pth",
                                             reid_r50.reid_param_shapes(), seed=7)
                det.reid = reid_r50.ReidEncoder(ctx, rsd, det)
            _cache[key] = (ctx, det)
    return _cache[key]


def _rows_to_dicts(track_results):
    return [
        {
            "track_id": int(x[0]),
            "tlbr": x[1:5],
            "tlhw": np.array([x[1], x[2], x[3] - x[1], x[4] - x[2]]),
            "confidence": x[5],
        }
        for x in track_results
    ]


def _tracktor(ctx, det, cap, video_length):
    """method "tracktor": per chunk ONE detector pass, ONE gray conversion and ONE ECC call over all consecutive frame pairs, then
    TracktorTracker.step frame by frame with Detector.regress / ReidEncoder.encode on the chunk's resident tensors"""
    from ..streaming import FrameStreamer
    reid, tracker = det.reid, TracktorTracker()
    in_ptr, _, (hp, wp, _c) = det.net_a.buffer("input")
    plane = hp * wp * 4
    gray = ctx.malloc((BATCH + 1) * plane)          # slot 0: the previous chunk's last frame; 1..n: this chunk's frames
    tm = dict(detector=0.0, ecc=0.0, regress=0.0, reid=0.0, host=0.0, ecc_iters=[])
    tracks = []

    def clocked(key, fn):
        def run(*a):
            t0 = time.perf_counter()
            out = fn(*a)
            tm[key] += (time.perf_counter() - t0) * 1e3
            return out
        return run

    streamer = FrameStreamer(ctx, cap, min(BATCH, video_length), max_frames=video_length)
    try:
        for dev_ptr, n, first in streamer:
            t0 = time.perf_counter()
            per_frame = det.run(None, frames_dev=(dev_ptr, n))
            streamer.release()                      # everything below reads the detector's own buffers
            t1 = time.perf_counter()
            ops.gray_from_nhwc4(ctx, in_ptr, n, hp, wp, gray + plane)
            pairs = [(k, k + 1) for k in range(0 if first else 1, n)]       # (template = previous frame, input = this frame)
            warps = {}
            if pairs:
                warp, _rho, iters, status = ops.ecc_euclidean(ctx, gray, n + 1, hp, wp, pairs, ECC_ITERS, ECC_EPS)
                for (_, k), m, st in zip(pairs, warp, status):
                    if st != _lib.PP_ECC_OK:
                        raise RuntimeError(f"camera-motion compensation failed on frame {first + k - 1}: ECC status {int(st)} "
                                           f"({'NaN correlation' if st == _lib.PP_ECC_NAN else 'non-positive lambda denominator'})")
                    warps[k - 1] = m
                tm["ecc_iters"] += [int(i) for i in iters]
            ctx.d2d(gray, gray + n * plane, plane)
            t2 = time.perf_counter()
            tm["detector"] += (t1 - t0) * 1e3
            tm["ecc"] += (t2 - t1) * 1e3
            empty = np.zeros((0, 4), np.float32)
            for k, rows in enumerate(per_frame):
                regress = clocked("regress", lambda b, k=k: det.regress(k, b))
                embed = clocked("reid", lambda b, k=k: reid.encode([b if j == k else empty for j in range(n)])[k])
                t3 = time.perf_counter()
                tracks.append(_rows_to_dicts(list(tracker.step(first + k, rows, regress, embed, warps.get(k)))))
                tm["host"] += (time.perf_counter() - t3) * 1e3
    finally:
        streamer.close()
        cap.release()
        ctx.synchronize()
        ctx.free(gray)
    tm["host"] -= tm["regress"] + tm["reid"]
    last_timing.clear()
    last_timing.update(tm, frames=len(tracks))
    return tracks


def mmtrack_bounding_boxes(file_path, method="tracktor"):
    if method not in _KNOWN:
        raise Exception(f"Unknown config file for MMTrack method {method}")
    if method not in ("tracktor", "deepsort", "bytetrack"):
        raise NotImplementedError(f"MMTrack method {method!r}: only the Faster-RCNN + Tracktor / SORT and YOLOX + ByteTrack families "
                                  "are built (see module docstring)")

    from ..streaming import FrameStreamer
    cap = open_video(file_path)
    video_length = int(cap.num_frames)
    ctx, det = _detector(cap.height, cap.width, method=method)
    if method == "tracktor":
        if video_length <= 0:
            cap.release()
            return []
        return _tracktor(ctx, det, cap, video_length)
    byte = method == "bytetrack"
    reid = getattr(det, "reid", None)
    tracker = ByteTracker() if byte else SortReidTracker() if reid is not None else Tracker(mode=1, match_iou_thr=0.5, obj_score_thr=0.5)
    batch = BATCH_YOLOX if byte else BATCH

    tracks = []
    if video_length <= 0:
        cap.release()
        return tracks
    # the clip is read once and streamed to the device `batch` frames at a time (the reference: one cap.read() and one
    # blocking upload per frame, :38-45); a read failure simply ends the stream (:41-42)
    streamer = FrameStreamer(ctx, cap, min(batch, video_length), max_frames=video_length)
    try:      # an error in a stage must not leak the reader thread, the page-locked staging buffers and the open video
        for dev_ptr, n, _first in streamer:
            per_frame = det.run(None, frames_dev=(dev_ptr, n))          # [n][5] float32: x1 y1 x2 y2 score
            if reid is not None:
                # appearance embeddings of the detections the tracker keeps, from the detector's resident input tensor
                per_frame = [rows[tracker.keep(rows)] for rows in per_frame]
                embeds = reid.encode(per_frame)
            streamer.release()
            for k, rows in enumerate(per_frame):
                if reid is not None:
                    track_results = list(tracker.step(rows, embeds[k]))                          # [id, x1, y1, x2, y2, score]
                elif byte:
                    track_results = list(tracker.step(rows))
                else:
                    ids, _, info = tracker.step(rows[:, :4].astype(np.float64), rows[:, 4].astype(np.float64))
                    track_results = [np.concatenate([[np.float32(i)], rows[j]]).astype(np.float32) for i, j in zip(ids, info[:, 1])]
                tracks.append(_rows_to_dicts(track_results))
    finally:
        streamer.close()
        cap.release()
    return tracks
