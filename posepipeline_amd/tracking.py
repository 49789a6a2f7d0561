"""Host-side tracking stage: thin wrappers over pp_tracker_* plus the PersonBbox selection/smoothing.

Mirrors, for the cascade's tracking stage,
  * pose_pipeline/wrappers/deep_sort_yolov4/deep_sort/tracker.py (the in-tree DeepSORT, mode 0) and
    mmtrack's SortTracker as wired by wrappers/mmtrack.py:45 (mode 1) -- both in C++ behind the C ABI;
  * pose_pipeline/pipeline.py:656-687 `PersonBbox.make`: pick the frame's box iff exactly one of
    `keep_tracks` is present, then pandas `bfill(limit=2)` / `ffill(limit=2)` over missing rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def linear_sum_assignment(cost):
    """scipy.optimize.linear_sum_assignment restated in C++ (tie-breaking included)."""
    cost = np.ascontiguousarray(cost, np.float64)
    nr, nc = cost.shape
    n = min(nr, nc)
    rows = np.zeros(max(n, 1), np.int32)
    cols = np.zeros(max(n, 1), np.int32)
    k = C.c_int32()
    L.check(L.load_library().pp_linear_sum_assignment(L.ptr(cost), nr, nc, L.ptr(rows), L.ptr(cols), C.byref(k)),
            "pp_linear_sum_assignment")
    return rows[: k.value].astype(np.int64), cols[: k.value].astype(np.int64)


class Tracker:
    """mode 0: in-tree DeepSORT (needs appearance features); mode 1: mmtrack SORT without ReID."""

    def __init__(self, mode=0, feat_dim=128, max_iou_distance=0.7, max_cosine_distance=0.3, max_age=30, n_init=3,
                 match_iou_thr=0.5, obj_score_thr=0.5):
        self.lib = L.load_library()
        self.mode = mode
        self.feat_dim = feat_dim if mode == 0 else 0
        h = C.c_void_p()
        a, b = (max_iou_distance, max_cosine_distance) if mode == 0 else (match_iou_thr, obj_score_thr)
        L.check(self.lib.pp_tracker_create(mode, self.feat_dim, a, b, max_age, n_init, C.byref(h)), "pp_tracker_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pp_tracker_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, tlwh, conf, feats=None, cap=1024):
        """-> (track_id int64 [n], tlwh float64 [n][4], info int32 [n][4])"""
        tlwh = np.ascontiguousarray(tlwh, np.float64).reshape(-1, 4)
        conf = np.ascontiguousarray(conf, np.float64).reshape(-1)
        n = tlwh.shape[0]
        f = None
        if self.mode == 0:
            f = np.ascontiguousarray(feats, np.float64).reshape(n, self.feat_dim)
        ids = np.zeros(cap, np.int64)
        out = np.zeros((cap, 4), np.float64)
        info = np.zeros((cap, 4), np.int32)
        k = C.c_int32()
        L.check(self.lib.pp_tracker_step(self.handle, L.ptr(tlwh), L.ptr(conf), L.ptr(f), n, cap, L.ptr(ids), L.ptr(out),
                                         L.ptr(info), C.byref(k)), "pp_tracker_step")
        k = k.value
        self._last_ids = set(int(i) for i in ids[:k])
        return ids[:k].copy(), out[:k].copy(), info[:k].copy()

    def live_ids(self) -> set:
        """ids that can still be reported by a later frame.  Both built modes report every track they keep: mode 0 emits
        all of tracker.tracks per frame (parser.py:76-86), mode 1 (no ReID) can only re-associate tracks seen in the
        previous frame -- so the live set is the id set of the last step."""
        return getattr(self, "_last_ids", set())

    def dump(self, cap=1024):
        ids = np.zeros(cap, np.int64)
        st = np.zeros((cap, 4), np.int32)
        mean = np.zeros((cap, 8))
        cov = np.zeros((cap, 64))
        k = C.c_int32()
        L.check(self.lib.pp_tracker_dump(self.handle, cap, L.ptr(ids), L.ptr(st), L.ptr(mean), L.ptr(cov), C.byref(k)),
                "pp_tracker_dump")
        k = k.value
        return ids[:k], st[:k], mean[:k], cov[:k].reshape(k, 8, 8)


def person_bbox(tracks, keep_tracks, limit=2):
    """PersonBbox.make (pipeline.py:656-687) without pandas.

    tracks: list (frames) of lists of dicts with "track_id" and "tlhw" (= x, y, w, h).
    Returns (bbox [N][4] float64 with NaN rows, present [N] bool)."""
    n = len(tracks)
    bbox = np.zeros((n, 4), np.float64)
    present = np.zeros(n, bool)
    keep = set(int(k) for k in np.atleast_1d(keep_tracks))
    for i, fr in enumerate(tracks):
        valid = [t for t in fr if int(t["track_id"]) in keep]
        if len(valid) == 1:
            present[i] = True
            bbox[i] = np.asarray(valid[0]["tlhw"], np.float64)
    out = bbox.copy()
    out[~present] = np.nan
    missing = ~present
    # bfill(limit): a NaN row takes the next valid row if it is among the `limit` NaNs directly before it
    filled = out.copy()
    nxt = -1
    run = 0
    fill_b = np.zeros(n, bool)
    for i in range(n - 1, -1, -1):
        if not missing[i]:
            nxt, run = i, 0
        else:
            run += 1
            if nxt >= 0 and run <= limit:
                filled[i] = out[nxt]
                fill_b[i] = True
    still = missing & ~fill_b
    res = filled.copy()
    prv = -1
    run = 0
    for i in range(n):
        if not still[i]:
            prv, run = i, 0
        else:
            run += 1
            if prv >= 0 and run <= limit:
                res[i] = filled[prv]
    return res, ~np.isnan(res).any(axis=1)


# ---- mmtrack ByteTracker (method "bytetrack" of wrappers/mmtrack.py) ------------------------------------------
def _iou_f32(a, b, eps=1e-6):
    """mmdet bbox_overlaps(mode='iou') in float32: a [n][4], b [m][4] -> [n][m]"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = np.clip(np.minimum(a[:, None, 2:], b[None, :, 2:]) - np.maximum(a[:, None, :2], b[None, :, :2]), 0, None)
    overlap = wh[..., 0] * wh[..., 1]
    union = np.maximum(area_a[:, None] + area_b[None, :] - overlap, np.float32(eps))
    return overlap / union


class ByteTracker:
    """mmtrack ByteTracker as configured by 3rdparty/mmtracking/mot/bytetrack/bytetrack_yolox_x_crowdhuman_mot17-private-half.py:21-28
    (obj_score_thrs .6 / .1, init_track_thr .7, weight_iou_with_det_scores, match_iou_thrs .1 / .5 / .3, num_frames_retain 30).
    Kalman filter: pp_kalman_* (the C++ restatement pinned on the in-tree deep_sort filter, which mmtrack's KalmanFilter
    copies); assignment: `lap.lapjv(extend_cost=True, cost_limit)` = the optimum of the cost matrix extended with
    dummy rows / columns at cost_limit / 2, solved with pp_linear_sum_assignment.  mmtrack is not vendored: unpinned."""

    def __init__(self, high=0.6, low=0.1, init_track_thr=0.7, weight_iou_with_det_scores=True, match_iou_high=0.1,
                 match_iou_low=0.5, match_iou_tentative=0.3, num_frames_retain=30, num_tentatives=3):
        self.lib = L.load_library()
        self.high, self.low, self.init_thr = np.float32(high), np.float32(low), np.float32(init_track_thr)
        self.weight, self.thr = weight_iou_with_det_scores, (match_iou_high, match_iou_low, match_iou_tentative)
        self.retain, self.num_tentatives = num_frames_retain, num_tentatives
        self.tracks: dict = {}      # id -> [mean8, cov64, last_frame, hits, tentative]
        self.num_tracks = 0
        self.frame_id = -1

    def live_ids(self) -> set:
        return set(int(i) for i in self.tracks)

    # Kalman steps through the C ABI
    def _kf(self, fn, mean, cov, z=None):
        if z is None:
            L.check(getattr(self.lib, fn)(L.ptr(mean), L.ptr(cov)), fn)
        else:
            zz = np.ascontiguousarray(z, np.float64)
            L.check(getattr(self.lib, fn)(L.ptr(mean), L.ptr(cov), L.ptr(zz)), fn)

    @staticmethod
    def _cxcyah(box):
        b = box.astype(np.float32)
        w, h = b[2] - b[0], b[3] - b[1]
        return np.array([(b[2] + b[0]) / np.float32(2), (b[3] + b[1]) / np.float32(2), w / h, h], np.float64)

    def _track_boxes(self, ids):
        m = np.array([self.tracks[i][0][:4] for i in ids], np.float64).astype(np.float32).reshape(-1, 4)
        w = m[:, 2] * m[:, 3]
        two = np.float32(2)
        return np.stack([m[:, 0] - w / two, m[:, 1] - m[:, 3] / two, m[:, 0] + w / two, m[:, 1] + m[:, 3] / two], -1)

    def _assign(self, ids, dets, weight, thr):
        n, m = len(ids), len(dets)
        row, col = np.full(n, -1, np.int64), np.full(m, -1, np.int64)
        if n == 0 or m == 0:
            return row, col
        ious = _iou_f32(self._track_boxes(ids), dets[:, :4])
        if weight:
            ious = ious * dets[:, 4][None]
        dists = (np.float32(1) - ious).astype(np.float64)
        ext = np.full((n + m, n + m), (1 - thr) / 2.0)
        ext[n:, m:] = 0.0
        ext[:n, :m] = dists
        r, c = linear_sum_assignment(ext)
        for i, j in zip(r, c):
            if i < n and j < m:
                row[i], col[j] = j, i
        return row, col

    def step(self, dets):
        """dets [n][5] float32 (x1, y1, x2, y2, score) -> [m][6] float32 rows (id, x1, y1, x2, y2, score)"""
        self.frame_id += 1
        fid = self.frame_id
        dets = np.asarray(dets, np.float32).reshape(-1, 5)
        if not self.tracks or len(dets) == 0:
            out = dets[dets[:, 4] > self.init_thr]
            ids = np.arange(self.num_tracks, self.num_tracks + len(out), dtype=np.int64)
            self.num_tracks += len(out)
        else:
            first = dets[:, 4] > self.high
            second = (~first) & (dets[:, 4] > self.low)
            d1, d2 = dets[first], dets[second]
            confirmed = [i for i, t in self.tracks.items() if not t[4]]
            unconfirmed = [i for i, t in self.tracks.items() if t[4]]
            for i in confirmed:
                t = self.tracks[i]
                if t[2] != fid - 1:
                    t[0][7] = 0.0                       # lost in the previous frame: no vertical velocity
                self._kf("pp_kalman_predict", t[0], t[1])
            row1, col1 = self._assign(confirmed, d1, self.weight, self.thr[0])
            id1 = np.array([confirmed[r] if r > -1 else -1 for r in col1], np.int64)
            hit = id1 > -1
            u_b, u_i = d1[~hit], id1[~hit].copy()
            _, colt = self._assign(unconfirmed, u_b, self.weight, self.thr[2])
            for j, r in enumerate(colt):
                if r > -1:
                    u_i[j] = unconfirmed[r]
            rest = [i for k, i in enumerate(confirmed) if row1[k] == -1 and self.tracks[i][2] == fid - 1]
            _, col2 = self._assign(rest, d2, False, self.thr[1])
            id2 = np.array([rest[r] if r > -1 else -1 for r in col2], np.int64)
            keep2 = id2 > -1
            out = np.concatenate([d1[hit], u_b, d2[keep2]])
            ids = np.concatenate([id1[hit], u_i, id2[keep2]])
            new = ids == -1
            ids[new] = np.arange(self.num_tracks, self.num_tracks + int(new.sum()))
            self.num_tracks += int(new.sum())
        for i, b in zip(ids, out):
            i = int(i)
            z = self._cxcyah(b[:4])
            if i in self.tracks:
                t = self.tracks[i]
                self._kf("pp_kalman_update", t[0], t[1], z)
                t[2], t[3] = fid, t[3] + 1
                if t[4] and t[3] >= self.num_tentatives:
                    t[4] = False
            else:
                mean, cov = np.zeros(8), np.zeros(64)
                L.check(self.lib.pp_kalman_initiate(L.ptr(z), L.ptr(mean), L.ptr(cov)), "pp_kalman_initiate")
                self.tracks[i] = [mean, cov, fid, 1, fid != 0]
        for i in [i for i, t in self.tracks.items() if fid - t[2] >= self.retain or (t[4] and t[2] != fid)]:
            del self.tracks[i]
        if len(out) == 0:
            return np.zeros((0, 6), np.float32)
        return np.concatenate([ids[:, None].astype(np.float32), out], axis=1).astype(np.float32)


# ---- mmtrack SortTracker WITH its ReID branch (method "deepsort" of wrappers/mmtrack.py) ---------------------------------
REID_GATED = 1e6      # surrogate cost of a Kalman-gated (track, detection) pair in the appearance assignment, see below


def reid_cdist(a, b):
    """torch.cdist(a, b) (p = 2) of float32 rows, defined here as: float64 sum of squared float32 differences, sqrt,
    rounded to float32"""
    d = a.astype(np.float32)[:, None, :].astype(np.float64) - b.astype(np.float32)[None, :, :].astype(np.float64)
    return np.sqrt((d * d).sum(-1)).astype(np.float32)


class SortReidTracker:
    """mmtrack 0.x `SortTracker.track` as configured by 3rdparty/mmtracking/mot/deepsort/
    deepsort_faster-rcnn_fpn_4e_mot17-private-half.py:43-54 (obj_score_thr .5, reid num_samples 10 / match_score_thr 2.0,
    match_iou_thr .5, num_tentatives 2, num_frames_retain 100; motion = KalmanFilter(center_only=False)):

      frame with no track yet (or no kept detection): every kept detection starts a track (tentative until it has
      `num_tentatives` boxes; a tentative track that misses a frame is dropped), ids from a running counter starting at 0;
      otherwise: Kalman-predict EVERY track and gate it against every detection (chi-square 0.95, 4 dof);
        1. appearance: confirmed tracks (any age up to num_frames_retain) vs detections, Euclidean distance between the mean
           of the track's last <= 10 embeddings and the detection's embedding, gated pairs excluded, Hungarian, accept
           distance <= 2.0;
        2. IoU: tracks updated in the previous frame and not matched yet vs the unmatched detections, cost 1 - IoU of the
           last OBSERVED box (float32), Hungarian, accept cost < 0.5;
      unmatched detections start new tracks; matched tracks get a Kalman update with the detection.

    The gated pairs: mmtrack writes NaN into the distance matrix before scipy.optimize.linear_sum_assignment, which current
    scipy rejects ("matrix contains invalid numeric entries") and old scipy resolved by unspecified NaN comparisons.  The
    well-defined reading implemented here (and in oracle/reid_mm.py): a gated pair costs REID_GATED = 1e6 in the assignment
    -- so the optimum uses as few gated pairs as possible -- and is never accepted.
    Kalman filter / Hungarian: the C++ restatements behind pp_kalman_* / pp_linear_sum_assignment (fixture-pinned on the
    in-tree deep_sort filter, which mmtrack's KalmanFilter copies).  mmtrack is not vendored: PARITY UNPINNED."""

    CHI2INV95_4 = 9.4877

    def __init__(self, obj_score_thr=0.5, match_iou_thr=0.5, match_score_thr=2.0, num_samples=10, num_tentatives=2,
                 num_frames_retain=100):
        self.lib = L.load_library()
        self.obj_score_thr, self.match_iou_thr, self.match_score_thr = np.float32(obj_score_thr), match_iou_thr, match_score_thr
        self.num_samples, self.num_tentatives, self.retain = num_samples, num_tentatives, num_frames_retain
        self.tracks: dict = {}      # id -> dict(mean, cov, box, last, n, tentative, embeds); insertion-ordered like mmtrack's
        self.num_tracks = 0
        self.frame_id = -1

    def live_ids(self) -> set:
        return set(self.tracks)

    def keep(self, dets):
        """mask of the detections the tracker uses (score > obj_score_thr): only these need an embedding"""
        return np.asarray(dets, np.float32).reshape(-1, 5)[:, 4] > self.obj_score_thr

    def _kf(self, fn, *args):
        L.check(getattr(self.lib, fn)(*[L.ptr(a) for a in args]), fn)

    def step(self, dets, embeds):
        """dets [n][5] float32 (x1, y1, x2, y2, score), ALREADY filtered with keep(); embeds [n][d] float32
        -> rows [n][6] float32 (id, x1, y1, x2, y2, score)"""
        self.frame_id += 1
        fid = self.frame_id
        dets = np.asarray(dets, np.float32).reshape(-1, 5)
        n = len(dets)
        embeds = np.asarray(embeds, np.float32).reshape(n, -1) if n else np.zeros((0, 1), np.float32)
        zs = np.stack([ByteTracker._cxcyah(d[:4]) for d in dets]) if n else np.zeros((0, 4))
        ids = np.full(n, -1, np.int64)
        if self.tracks and n:
            order = list(self.tracks)
            gate = np.zeros((len(order), n))
            for r, i in enumerate(order):
                t = self.tracks[i]
                self._kf("pp_kalman_predict", t["mean"], t["cov"])
                out = np.zeros(n)
                L.check(self.lib.pp_kalman_gating_distance(L.ptr(t["mean"]), L.ptr(t["cov"]), L.ptr(np.ascontiguousarray(zs)), n, L.ptr(out)),
                        "pp_kalman_gating_distance")
                gate[r] = out
            gated = gate > self.CHI2INV95_4
            confirmed = [i for i in order if not self.tracks[i]["tentative"]]
            if confirmed:
                means = []
                for i in confirmed:
                    e = self.tracks[i]["embeds"][-self.num_samples:]
                    acc = np.zeros_like(e[0])
                    for v in e:
                        acc = (acc + v).astype(np.float32)
                    means.append((acc / np.float32(len(e))).astype(np.float32))
                dist = reid_cdist(np.stack(means), embeds)
                g = gated[[order.index(i) for i in confirmed]]
                cost = np.where(g, REID_GATED, dist.astype(np.float64))
                rows, cols = linear_sum_assignment(cost)
                for r, c in zip(rows, cols):
                    if not g[r, c] and dist[r, c] <= self.match_score_thr:
                        ids[c] = confirmed[r]
            active = [i for i in order if i not in set(ids.tolist()) and self.tracks[i]["last"] == fid - 1]
            if active:
                free = np.flatnonzero(ids == -1)
                if len(free):
                    tb = np.stack([self.tracks[i]["box"] for i in active])
                    dists = (np.float32(1) - _iou_f32(tb, dets[free, :4])).astype(np.float64)
                    rows, cols = linear_sum_assignment(dists)
                    for r, c in zip(rows, cols):
                        if dists[r, c] < 1 - self.match_iou_thr:
                            ids[free[c]] = active[r]
        new = ids == -1
        ids[new] = np.arange(self.num_tracks, self.num_tracks + int(new.sum()))
        self.num_tracks += int(new.sum())
        for i, d, z, e in zip(ids.tolist(), dets, zs, embeds):
            if i in self.tracks:
                t = self.tracks[i]
                self._kf("pp_kalman_update", t["mean"], t["cov"], np.ascontiguousarray(z))
                t["box"], t["last"], t["n"] = d[:4].copy(), fid, t["n"] + 1
                t["embeds"] = (t["embeds"] + [e.copy()])[-self.num_samples:]
                if t["tentative"] and t["n"] >= self.num_tentatives:
                    t["tentative"] = False
            else:
                mean, cov = np.zeros(8), np.zeros(64)
                L.check(self.lib.pp_kalman_initiate(L.ptr(np.ascontiguousarray(z)), L.ptr(mean), L.ptr(cov)), "pp_kalman_initiate")
                self.tracks[i] = dict(mean=mean, cov=cov, box=d[:4].copy(), last=fid, n=1, tentative=True, embeds=[e.copy()])
        for i in [i for i, t in self.tracks.items() if fid - t["last"] >= self.retain or (t["tentative"] and t["last"] != fid)]:
            del self.tracks[i]
        return np.concatenate([ids[:, None].astype(np.float32), dets], axis=1).astype(np.float32) if n else np.zeros((0, 6), np.float32)


# ---- mmtrack TracktorTracker (method "tracktor" of wrappers/mmtrack.py) ---------------------------------------------------
def _nms_f32(boxes, scores, iou_thr):
    """mmcv `nms` on the host (float32, x1y1x2y2, area = w * h, suppress where inter > thr * union, stable descending score
    order): kept indices.  The few boxes of a frame's tracks; the detector's own NMS is the device kernel (nms.hip)."""
    b, s = np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(scores, np.float32).reshape(-1)
    order = np.argsort(-s, kind="stable")
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    thr, dead, keep = np.float32(iou_thr), np.zeros(len(b), bool), []
    for i in range(len(b)):
        if dead[i]:
            continue
        keep.append(int(order[i]))
        w = np.maximum(np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]), np.float32(0))
        h = np.maximum(np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]), np.float32(0))
        inter = w * h
        dead[i + 1:] |= inter > thr * ((area[i] + area[i + 1:]) - inter)
    return keep


def warp_boxes_f32(boxes, warp):
    """CameraMotionCompensation.warp_bboxes: the tl and br corners of [n][4] float32 boxes through the 2 x 3 map, in float32
    ((m00 x + m01 y) + m02; cv2.findTransformECC returns a float32 matrix, so the map is rounded to float32 first)"""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    m = np.asarray(warp, np.float64).reshape(2, 3).astype(np.float32)
    out = np.empty_like(b)
    for k in (0, 2):
        out[:, k] = (m[0, 0] * b[:, k] + m[0, 1] * b[:, k + 1]) + m[0, 2]
        out[:, k + 1] = (m[1, 0] * b[:, k] + m[1, 1] * b[:, k + 1]) + m[1, 2]
    return out


class TracktorTracker:
    """mmtrack 0.x `TracktorTracker.track` (+ BaseTracker's memo, CameraMotionCompensation.warp_bboxes) as configured by
    3rdparty/mmtracking/mot/tracktor/tracktor_faster-rcnn_r50_fpn_4e_mot17-private-half.py:43-62: obj_score_thr .5, regression
    (obj_score_thr .5, nms IoU .6, match_iou_thr .3), reid (obj_score_thr .5, img_scale (256, 128), match_score_thr 2.0,
    match_iou_thr .2), momentums None, num_frames_retain 10; motion = camera-motion compensation only (no linear motion model, so
    one box per track is warped).  Per frame:

      detections with score > .5 are kept.  No track yet: each starts a track (ids from a running counter) and is embedded.
      Otherwise  1. every track's last box is warped with the frame's ECC map (warp_boxes_f32);
                 2. the boxes of the tracks seen in the PREVIOUS frame are regressed through the detector's RoI head on this frame;
                    NMS (IoU .6) over those with score > 0, result in descending score order; score > .5 survives: propagated;
                 3. detections whose IoU with any propagated box is >= .3 are dropped;
                 4. propagated boxes and remaining detections are embedded; every track that was NOT propagated is a candidate for
                    the remaining detections: cost = Euclidean distance of the mean of its last <= 10 embeddings to the detection's,
                    1e6 where the IoU of its (warped) last box with the detection is < .2; Hungarian; cost <= 2.0 hands the id over;
                 5. the rest start new tracks, in detector order.
      Rows out: propagated first, then detections, [id, x1, y1, x2, y2, score].  Every row updates (or starts) its track with box,
      score, embedding and frame; tracks not seen for 10 frames are dropped.  frame_id 0 resets the tracker.

    The three device-side pieces come in as arguments, so the flow runs without a GPU:
      regress(boxes [n][4] float32) -> (boxes [n][4], scores [n])     Detector.regress on the current frame
      embed(boxes [n][4] float32)   -> [n][d] float32                  ReidEncoder.encode on the current frame
      warp                          2 x 3 map of the frame (pp_ecc_euclidean); only read when there are tracks
    The map is estimated between the detector's INPUT tensors (normalised, resized, padded) and applied to boxes in SOURCE pixels:
    that is how the configuration behaves with rescale=True.  mmtrack is not vendored: restated from memory, PARITY UNPINNED
    (tests/tracktor_ref.py holds the loop-by-loop transcription this class is tested against)."""

    def __init__(self, obj_score_thr=0.5, regress_score_thr=0.5, regress_nms_iou=0.6, regress_match_iou=0.3, reid_match_score=2.0,
                 reid_match_iou=0.2, num_samples=10, num_frames_retain=10):
        self.lib = L.load_library()
        self.obj_score_thr, self.reg_thr, self.reg_nms = np.float32(obj_score_thr), np.float32(regress_score_thr), regress_nms_iou
        self.reg_iou, self.reid_score, self.reid_iou = np.float32(regress_match_iou), reid_match_score, np.float32(reid_match_iou)
        self.num_samples, self.retain = num_samples, num_frames_retain
        self.reset()

    def reset(self):
        self.tracks: dict = {}      # id -> dict(box, score, last, embeds); insertion-ordered like mmtrack's memo
        self.num_tracks = 0

    def live_ids(self) -> set:
        return set(self.tracks)

    def step(self, frame_id, dets, regress, embed, warp=None):
        """dets [n][5] float32 (x1, y1, x2, y2, score) -> rows [m][6] float32 (id, x1, y1, x2, y2, score)"""
        if frame_id == 0:
            self.reset()
        dets = np.asarray(dets, np.float32).reshape(-1, 5)
        dets = dets[dets[:, 4] > self.obj_score_thr]
        if not self.tracks:
            boxes, scores = dets[:, :4], dets[:, 4]
            ids = np.arange(self.num_tracks, self.num_tracks + len(dets), dtype=np.int64)
        else:
            order = list(self.tracks)
            warped = warp_boxes_f32(np.stack([self.tracks[i]["box"] for i in order]), warp)
            for i, b in zip(order, warped):
                self.tracks[i]["box"] = b
            prev = [i for i in order if self.tracks[i]["last"] == frame_id - 1]
            p_ids, p_boxes, p_scores = np.zeros(0, np.int64), np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
            if prev:
                rb, rs = regress(np.stack([self.tracks[i]["box"] for i in prev]))
                rb, rs = np.asarray(rb, np.float32).reshape(-1, 4), np.asarray(rs, np.float32).reshape(-1)
                valid = np.flatnonzero(rs > np.float32(0))
                keep = valid[_nms_f32(rb[valid], rs[valid], self.reg_nms)] if len(valid) else valid
                keep = keep[rs[keep] > self.reg_thr]
                p_ids, p_boxes, p_scores = np.asarray(prev, np.int64)[keep], rb[keep], rs[keep]
            if len(p_ids) and len(dets):
                dets = dets[~(_iou_f32(p_boxes, dets[:, :4]) >= self.reg_iou).any(axis=0)]
            d_ids = np.full(len(dets), -1, np.int64)
            boxes, scores = np.concatenate([p_boxes, dets[:, :4]]), np.concatenate([p_scores, dets[:, 4]])
        embeds = np.asarray(embed(boxes), np.float32).reshape(len(boxes), -1) if len(boxes) else np.zeros((0, 1), np.float32)
        if self.tracks:
            cand = [i for i in order if i not in set(p_ids.tolist())]
            if cand and len(dets):
                means = []
                for i in cand:
                    e = self.tracks[i]["embeds"][-self.num_samples:]
                    acc = np.zeros_like(e[0])
                    for v in e:
                        acc = (acc + v).astype(np.float32)
                    means.append((acc / np.float32(len(e))).astype(np.float32))
                cost = reid_cdist(np.stack(means), embeds[len(p_ids):]).astype(np.float64)
                cost[_iou_f32(np.stack([self.tracks[i]["box"] for i in cand]), dets[:, :4]) < self.reid_iou] = REID_GATED
                for r, c in zip(*linear_sum_assignment(cost)):
                    if cost[r, c] <= self.reid_score:
                        d_ids[c] = cand[r]
            new = d_ids == -1
            d_ids[new] = np.arange(self.num_tracks, self.num_tracks + int(new.sum()))
            ids = np.concatenate([p_ids, d_ids])
        self.num_tracks = max(self.num_tracks, int(ids.max()) + 1) if len(ids) else self.num_tracks
        for i, b, s, e in zip(ids.tolist(), boxes, scores, embeds):
            t = self.tracks.setdefault(i, dict(embeds=[]))
            t["box"], t["score"], t["last"] = b.copy(), s, frame_id
            t["embeds"] = (t["embeds"] + [e.copy()])[-self.num_samples:]
        for i in [i for i, t in self.tracks.items() if frame_id - t["last"] >= self.retain]:
            del self.tracks[i]
        if len(ids) == 0:
            return np.zeros((0, 6), np.float32)
        return np.concatenate([ids[:, None].astype(np.float32), boxes, scores[:, None]], axis=1).astype(np.float32)


# ---- FairMOT JDETracker (wrappers/fairmot.py) -------------------------------------------------------------------------------------
class _STrack:
    """one track of JDETracker (upstream STrack): state 0 New, 1 Tracked, 2 Lost, 3 Removed"""
    __slots__ = ("tlwh0", "score", "mean", "cov", "is_activated", "state", "track_id", "frame_id", "start_frame", "tracklet_len",
                 "curr_feat", "smooth_feat")

    def __init__(self, tlwh, score, feat):
        self.tlwh0 = np.asarray(tlwh, np.float64)
        self.score = float(score)
        self.mean = self.cov = None
        self.is_activated = False
        self.state, self.track_id, self.frame_id, self.start_frame, self.tracklet_len = 0, 0, 0, 0, 0
        self.smooth_feat = None
        self.update_features(feat)

    def update_features(self, feat, alpha=0.9):
        feat = np.asarray(feat, np.float64)
        feat = feat / np.linalg.norm(feat)
        self.curr_feat = feat
        if self.smooth_feat is None:
            self.smooth_feat = feat
        else:
            self.smooth_feat = alpha * self.smooth_feat + (1 - alpha) * feat
        self.smooth_feat = self.smooth_feat / np.linalg.norm(self.smooth_feat)

    @property
    def tlwh(self):
        if self.mean is None:
            return self.tlwh0.copy()
        ret = self.mean[:4].copy()
        ret[2] *= ret[3]
        ret[:2] -= ret[2:] / 2
        return ret

    @property
    def tlbr(self):
        ret = self.tlwh
        ret[2:] += ret[:2]
        return ret

    def xyah(self):
        ret = self.tlwh
        ret[:2] += ret[2:] / 2
        ret[2] /= ret[3]
        return np.ascontiguousarray(ret)


def jde_iou_distance(a_tlbr, b_tlbr):
    """1 - IoU with cython_bbox's convention: float64, + 1 on widths, heights and intersections"""
    a = np.asarray(a_tlbr, np.float64).reshape(-1, 4)
    b = np.asarray(b_tlbr, np.float64).reshape(-1, 4)
    cost = np.ones((len(a), len(b)))
    if cost.size == 0:
        return cost
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    iw = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]) + 1
    ih = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]) + 1
    ok = (iw > 0) & (ih > 0)
    inter = np.where(ok, iw * ih, 0.0)
    return 1.0 - np.where(ok, inter / (area_a[:, None] + area_b[None, :] - inter), 0.0)


def lapjv_assign(cost, thresh):
    """`lap.lapjv(cost, extend_cost=True, cost_limit=thresh)` read as ByteTracker._assign reads it: the optimum of the cost matrix
    extended with dummy rows / columns at thresh / 2 (entries may be +inf).  -> (matches [(row, col)], unmatched rows, unmatched cols)"""
    cost = np.asarray(cost, np.float64)
    n, m = cost.shape
    if n == 0 or m == 0:
        return [], list(range(n)), list(range(m))
    ext = np.full((n + m, n + m), thresh / 2.0)
    ext[n:, m:] = 0.0
    ext[:n, :m] = cost
    r, c = linear_sum_assignment(ext)
    matches = [(int(i), int(j)) for i, j in zip(r, c) if i < n and j < m]
    mr, mc = {i for i, _ in matches}, {j for _, j in matches}
    return matches, [i for i in range(n) if i not in mr], [j for j in range(m) if j not in mc]


class JDETracker:
    """FairMOT's `JDETracker.update` with `STrack` (src/lib/tracker/multitracker.py) on the host, after the detections are decoded:
    appearance association with Kalman gating (`fuse_motion`, lambda 0.98), IoU association of the rest, unconfirmed tracks, new
    tracks, expiry of lost tracks after max_time_lost = int(fps / 30 * track_buffer) frames, duplicate removal.  Ids start at 1 in
    every instance (the reference wrapper resets BaseTrack._count per call).  Float64 throughout.  Kalman filter: pp_kalman_*
    (the same xyah filter); assignment: lapjv_assign.  Quirks kept: a lost track that expires stays one more frame in the lost
    list (upstream subtracts the removed list before extending it), and a new track is activated at once only in frame 1.
    A re-activated track takes the matched detection's score (the score reported is the last matched detection's).
    Restated from memory of the published code: UNPINNED."""

    CHI2INV95_4 = 9.4877

    def __init__(self, frame_rate=30, conf_thres=0.2, track_buffer=30):
        self.lib = L.load_library()
        self.tracked, self.lost, self.removed = [], [], []
        self.frame_id = 0
        self.det_thresh = conf_thres
        self.max_time_lost = int(frame_rate / 30.0 * track_buffer)
        self._count = 0

    def live_ids(self) -> set:
        return {t.track_id for t in self.tracked + self.lost}

    def _kf(self, fn, *args):
        L.check(getattr(self.lib, fn)(*[L.ptr(a) for a in args]), fn)

    def _kf_update(self, t, det):
        self._kf("pp_kalman_update", t.mean, t.cov, det.xyah())

    def _update(self, t, det):
        t.frame_id = self.frame_id
        t.tracklet_len += 1
        self._kf_update(t, det)
        t.state, t.is_activated, t.score = 1, True, det.score
        t.update_features(det.curr_feat)

    def _re_activate(self, t, det):
        self._kf_update(t, det)
        t.update_features(det.curr_feat)
        t.tracklet_len, t.state, t.is_activated, t.frame_id, t.score = 0, 1, True, self.frame_id, det.score

    def _activate(self, t):
        self._count += 1
        t.track_id = self._count
        z = t.xyah()
        t.mean, t.cov = np.zeros(8), np.zeros(64)
        self._kf("pp_kalman_initiate", z, t.mean, t.cov)
        t.tracklet_len, t.state = 0, 1
        if self.frame_id == 1:
            t.is_activated = True
        t.frame_id = t.start_frame = self.frame_id

    def _embedding_gated(self, pool, dets):
        cost = np.zeros((len(pool), len(dets)))
        if cost.size == 0:
            return cost
        df = np.stack([d.curr_feat for d in dets])
        tf = np.stack([t.smooth_feat for t in pool])
        num = tf @ df.T
        den = np.linalg.norm(tf, axis=1)[:, None] * np.linalg.norm(df, axis=1)[None, :]
        cost = np.maximum(0.0, 1.0 - num / den)
        zs = np.ascontiguousarray(np.stack([d.xyah() for d in dets]))
        for r, t in enumerate(pool):
            g = np.zeros(len(dets))
            L.check(self.lib.pp_kalman_gating_distance(L.ptr(t.mean), L.ptr(t.cov), L.ptr(zs), len(dets), L.ptr(g)), "pp_kalman_gating_distance")
            cost[r, g > self.CHI2INV95_4] = np.inf
            cost[r] = 0.98 * cost[r] + 0.02 * g
        return cost

    @staticmethod
    def _joint(a, b):
        ids = {t.track_id for t in a}
        res = list(a)
        for t in b:
            if t.track_id not in ids:
                ids.add(t.track_id)
                res.append(t)
        return res

    @staticmethod
    def _sub(a, b):
        ids = {t.track_id for t in b}
        return [t for t in a if t.track_id not in ids]

    def step(self, dets, feats):
        """dets [n][5] float (x1, y1, x2, y2, score) already filtered by score > conf_thres, feats [n][d]
        -> [(track_id, tlwh float64 [4], score)] of the activated tracked tracks"""
        self.frame_id += 1
        dets = np.asarray(dets, np.float64).reshape(-1, 5)
        feats = np.asarray(feats, np.float64).reshape(len(dets), -1)
        activated, refind, lost, removed = [], [], [], []
        detections = [_STrack(np.r_[d[:2], d[2:4] - d[:2]], d[4], f) for d, f in zip(dets, feats)]
        unconfirmed = [t for t in self.tracked if not t.is_activated]
        tracked = [t for t in self.tracked if t.is_activated]
        pool = self._joint(tracked, self.lost)
        for t in pool:                                   # multi_predict
            if t.state != 1:
                t.mean[7] = 0.0
            self._kf("pp_kalman_predict", t.mean, t.cov)

        def take(matches, tracks, dets_):
            for it, idet in matches:
                t, d = tracks[it], dets_[idet]
                if t.state == 1:
                    self._update(t, d)
                    activated.append(t)
                else:
                    self._re_activate(t, d)
                    refind.append(t)
        # appearance, gated by motion
        matches, u_track, u_det = lapjv_assign(self._embedding_gated(pool, detections), 0.4)
        take(matches, pool, detections)
        # IoU for the rest
        detections = [detections[i] for i in u_det]
        r_tracked = [pool[i] for i in u_track if pool[i].state == 1]
        matches, u_track, u_det = lapjv_assign(jde_iou_distance([t.tlbr for t in r_tracked], [d.tlbr for d in detections]), 0.5)
        take(matches, r_tracked, detections)
        for it in u_track:
            t = r_tracked[it]
            if t.state != 2:
                t.state = 2
                lost.append(t)
        # unconfirmed tracks: usually tracks with only one beginning frame
        detections = [detections[i] for i in u_det]
        matches, u_unc, u_det = lapjv_assign(jde_iou_distance([t.tlbr for t in unconfirmed], [d.tlbr for d in detections]), 0.7)
        for it, idet in matches:
            self._update(unconfirmed[it], detections[idet])
            activated.append(unconfirmed[it])
        for it in u_unc:
            unconfirmed[it].state = 3
            removed.append(unconfirmed[it])
        for i in u_det:
            t = detections[i]
            if t.score < self.det_thresh:
                continue
            self._activate(t)
            activated.append(t)
        for t in self.lost:
            if self.frame_id - t.frame_id > self.max_time_lost:
                t.state = 3
                removed.append(t)
        self.tracked = [t for t in self.tracked if t.state == 1]
        self.tracked = self._joint(self.tracked, activated)
        self.tracked = self._joint(self.tracked, refind)
        self.lost = self._sub(self.lost, self.tracked)
        self.lost.extend(lost)
        self.lost = self._sub(self.lost, self.removed)
        self.removed.extend(removed)
        # remove_duplicate_stracks
        pd = jde_iou_distance([t.tlbr for t in self.tracked], [t.tlbr for t in self.lost])
        dupa, dupb = set(), set()
        for p, q in zip(*np.where(pd < 0.15)):
            tp = self.tracked[p].frame_id - self.tracked[p].start_frame
            tq = self.lost[q].frame_id - self.lost[q].start_frame
            if tp > tq:
                dupb.add(int(q))
            else:
                dupa.add(int(p))
        self.tracked = [t for i, t in enumerate(self.tracked) if i not in dupa]
        self.lost = [t for i, t in enumerate(self.lost) if i not in dupb]
        return [(t.track_id, t.tlwh, t.score) for t in self.tracked if t.is_activated]


# ---- TraDeS / CenterTrack tracker (wrappers/trades.py) -------------------------------------------------------------------------------
class TradesTracker:
    """CenterTrack's `Tracker.step` with the reference wrapper's settings (max_age = -1, hungarian = False, public_det = False, one
    class), on the host after the detections are decoded.  For detections d (in score order) and tracks t: dist = ||t.ct - (d.ct +
    d.tracking)||^2 in float32; a pair is invalid (+ 1e18) when dist > area(t.bbox) or dist > area(d.bbox); greedy assignment: each
    detection in turn takes its argmin over the tracks, accepted if < 1e16, and that track's column is then blocked.  A matched
    detection inherits the track's id, an unmatched one with score > new_thresh gets the next id (ids start at 1 in every instance),
    unmatched tracks are dropped.  The returned list (matched first, then new, each in detection order) is the next frame's tracks.
    The first frame goes through the same step with no tracks.  Restated from memory of the published code: UNPINNED."""

    def __init__(self, new_thresh=0.5):
        self.new_thresh = new_thresh
        self.id_count = 0
        self.tracks: list = []

    @staticmethod
    def _area(items):
        return np.array([(t["bbox"][2] - t["bbox"][0]) * (t["bbox"][3] - t["bbox"][1]) for t in items], np.float32)

    def step(self, results):
        """results: dicts with "score", "ct" [2], "tracking" [2], "bbox" [4] (source pixels), score descending -> the same dicts with
        "tracking_id", "age" and "active" added"""
        n, m = len(results), len(self.tracks)
        dets = np.array([np.asarray(d["ct"], np.float32) + np.asarray(d["tracking"], np.float32) for d in results], np.float32).reshape(n, 2)
        tracks = np.array([t["ct"] for t in self.tracks], np.float32).reshape(m, 2)
        dist = ((tracks.reshape(1, m, 2) - dets.reshape(n, 1, 2)) ** 2).sum(axis=2)
        invalid = (dist > self._area(self.tracks).reshape(1, m)) | (dist > self._area(results).reshape(n, 1))
        dist = dist + invalid * 1e18
        matches = []
        if m > 0:
            for i in range(n):
                j = int(dist[i].argmin())
                if dist[i, j] < 1e16:
                    dist[:, j] = 1e18
                    matches.append((i, j))
        ret = []
        for i, j in matches:
            d = results[i]
            d["tracking_id"], d["age"], d["active"] = self.tracks[j]["tracking_id"], 1, self.tracks[j]["active"] + 1
            ret.append(d)
        taken = {i for i, _ in matches}
        for i in range(n):
            d = results[i]
            if i not in taken and d["score"] > self.new_thresh:
                self.id_count += 1
                d["tracking_id"], d["age"], d["active"] = self.id_count, 1, 1
                ret.append(d)
        self.tracks = ret
        return ret
