"""CPU statements of the Tracktor configuration (method "tracktor" of wrappers/mmtrack.py) for tests/test_tracktor.py and
tests/test_gpu_tracktor.py.  TEST INFRASTRUCTURE ONLY.

  ecc_euclidean       cv2.findTransformECC(MOTION_EUCLIDEAN, no mask, gaussFiltSize 1) in float64 numpy, written from the text in
                      posepipeline_amd/csrc/ecc.hip's header (two passes per iteration: means first, then the zero-mean images --
                      not the kernel's single pass of raw sums)
  TracktorRef         mmtrack 0.x TracktorTracker.track + BaseTracker memo + CameraMotionCompensation.warp_bboxes with the values of
                      3rdparty/mmtracking/mot/tracktor/tracktor_faster-rcnn_r50_fpn_4e_mot17-private-half.py:43-62, one Python loop
                      per step of the flow
  regress_ref         roi_head.simple_test_bboxes(rescale=True) on given boxes, composed from oracle.detector
  reference_chain     the wrapper end to end on the CPU
OpenCV / mmtrack are neither vendored nor installed: PARITY UNPINNED.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

from oracle import boxes as obox
from oracle import detector as odet
from oracle import reid_mm as orm
from oracle.tracking import bbox_overlaps

f32 = np.float32
ECC_OK, ECC_NAN, ECC_DIVERGED = 0, 1, 2


# ---- ECC --------------------------------------------------------------------------------------------------------------
def _reflect101_gradients(img):
    p = np.pad(img, 1, mode="reflect")                     # numpy 'reflect' = REFLECT_101 (the edge pixel is not repeated)
    gx = 0.5 * p[1:-1, 2:] - 0.5 * p[1:-1, :-2]
    gy = 0.5 * p[2:, 1:-1] - 0.5 * p[:-2, 1:-1]
    return gx, gy


def _fixed_coords(M, h, w, round_delta, shift):
    xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    ax = np.rint(M[0, 0] * xs * 1024).astype(np.int64)
    bx = np.rint(M[1, 0] * xs * 1024).astype(np.int64)
    x0 = np.rint((M[0, 1] * ys + M[0, 2]) * 1024).astype(np.int64) + round_delta
    y0 = np.rint((M[1, 1] * ys + M[1, 2]) * 1024).astype(np.int64) + round_delta
    return (x0[:, None] + ax[None, :]) >> shift, (y0[:, None] + bx[None, :]) >> shift


def warp_bilinear(planes, M):
    """dst(x, y) = src(M (x, y, 1)) of each [h][w] float64 plane: warpAffine's fixed-point coordinates, constant border 0"""
    h, w = planes[0].shape
    X, Y = _fixed_coords(M, h, w, 16, 5)
    sx, sy, a, b = X >> 5, Y >> 5, (X & 31) / 32.0, (Y & 31) / 32.0
    out = [np.zeros((h, w)) for _ in planes]
    for dy, dx, wt in ((0, 0, (1 - a) * (1 - b)), (0, 1, a * (1 - b)), (1, 0, (1 - a) * b), (1, 1, a * b)):
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
        for o, p in zip(out, planes):
            o += wt * np.where(ok, p[yc, xc], 0.0)
    return out


def warp_mask(M, h, w):
    X, Y = _fixed_coords(M, h, w, 512, 10)
    return (X >= 0) & (X < w) & (Y >= 0) & (Y < h)


def ecc_euclidean(template, image, num_iters=100, stop_eps=1e-5):
    """-> (M [2][3] float64, rho, iterations, status).  The images are used as float64 whatever their dtype: feed float32 arrays for the
    'float32 images' evaluation."""
    T, I = np.asarray(template, np.float64), np.asarray(image, np.float64)
    h, w = T.shape
    gx, gy = _reflect101_gradients(I)
    Xg, Yg = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    M = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    rho, last_rho, it = -1.0, -stop_eps, 0
    i = 1
    while i <= num_iters and abs(rho - last_rho) >= stop_eps:
        Iw, gxw, gyw = warp_bilinear([I, gx, gy], M)
        mask = warp_mask(M, h, w)
        n = int(mask.sum())
        with np.errstate(all="ignore"):
            # means taken about the mask's first pixel: the same number up to rounding, and exactly the value of a constant image
            pI, pT = (Iw[mask][0], T[mask][0]) if n else (0.0, 0.0)
            mI, mT = pI + (Iw[mask] - pI).sum() / n if n else np.nan, pT + (T[mask] - pT).sum() / n if n else np.nan
            Izm = np.where(mask, Iw - mI, Iw)
            Tzm = np.where(mask, T - mT, 0.0)
            img_norm = np.sqrt((Izm[mask] ** 2).sum())
            tmp_norm = np.sqrt((Tzm[mask] ** 2).sum())
            c, s = M[0, 0], M[1, 0]
            J = np.stack([gxw * (-Xg * s - Yg * c) + gyw * (Xg * c - Yg * s), gxw, gyw]).reshape(3, -1)
            H = J @ J.T
            corr = float((Tzm * Izm).sum())
            ip, tp = J @ Izm.reshape(-1), J @ Tzm.reshape(-1)
            last_rho, rho = rho, corr / (img_norm * tmp_norm)
        it = i
        if np.isnan(rho):
            return M, rho, it, ECC_NAN
        Hinv = np.linalg.inv(H)
        a = Hinv @ ip
        lam_d = corr - tp @ a
        if not lam_d > 0:
            return M, rho, it, ECC_DIVERGED
        lam = (img_norm * img_norm - ip @ a) / lam_d
        dp = Hinv @ (lam * tp - ip)
        theta = np.arcsin(M[1, 0]) + dp[0]
        M = np.array([[np.cos(theta), -np.sin(theta), M[0, 2] + dp[1]], [np.sin(theta), np.cos(theta), M[1, 2] + dp[2]]])
        i += 1
    return M, rho, it, ECC_OK


def sinusoid_image(h, w, seed, motion=None, n_waves=24):
    """float64 [h][w] image of `n_waves` random sinusoids (wave numbers 0.2 - 0.4 rad / px in random directions, amplitudes
    0.5 - 1); with motion = (theta, tx, ty) the SAME image evaluated at M (x, y, 1), M = [[cos, -sin, tx], [sin, cos, ty]] -- i.e.
    template(x, y) = image(M (x, y, 1)) holds for image = sinusoid_image(h, w, seed) and template = sinusoid_image(h, w, seed,
    motion): ECC recovers M.  The band was picked on the CPU from the float64 reference alone: lower wave numbers leave too little
    gradient on a 50 x 70 image, higher ones cost bilinear-interpolation error (tests/test_tracktor.py holds the figures)."""
    rng = np.random.default_rng(seed)
    mag, ang = rng.uniform(0.2, 0.4, n_waves), rng.uniform(0, 2 * np.pi, n_waves)
    k = np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    ph, amp = rng.uniform(0, 2 * np.pi, n_waves), rng.uniform(0.5, 1.0, n_waves)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    if motion is not None:
        th, tx, ty = motion
        x, y = np.cos(th) * x - np.sin(th) * y + tx, np.sin(th) * x + np.cos(th) * y + ty
    return sum(a * np.sin(kx * x + ky * y + p) for (kx, ky), p, a in zip(k, ph, amp))


ECC_MOTIONS = ((0.004, 1.3, -0.7), (-0.01, -2.6, 1.9), (0.02, 4.2, 3.1))        # (theta rad, tx, ty)
ECC_SHAPES = ((96, 128), (50, 70))                                               # the second: no multiple of any tile
ECC_SEED = 40


def ecc_test_pairs(h, w):
    """the (template, image) pairs of the ECC tests, float64: one per motion"""
    return [(sinusoid_image(h, w, ECC_SEED + k, m), sinusoid_image(h, w, ECC_SEED + k)) for k, m in enumerate(ECC_MOTIONS)]


def motion_matrix(motion):
    th, tx, ty = motion
    return np.array([[np.cos(th), -np.sin(th), tx], [np.sin(th), np.cos(th), ty]])


def gray_f32(x_hwc):
    """cv2.cvtColor(COLOR_RGB2GRAY) of a float32 image, channels 0, 1, 2 = R, G, B"""
    x = np.asarray(x_hwc, f32)
    return ((f32(0.299) * x[..., 0] + f32(0.587) * x[..., 1]).astype(f32) + f32(0.114) * x[..., 2]).astype(f32)


def gray_f64(x_hwc):
    x = np.asarray(x_hwc, np.float64)
    return (float(f32(0.299)) * x[..., 0] + float(f32(0.587)) * x[..., 1]) + float(f32(0.114)) * x[..., 2]


# ---- the tracker, loop by loop ------------------------------------------------------------------------------------------------
class TracktorRef:
    """A literal transcription of the flow; `trace` records per frame what each branch did (the tests assert on it)."""

    def __init__(self):
        self.tracks = {}          # id -> dict(box, score, embeds, frame), insertion-ordered
        self.num_tracks = 0
        self.trace = []

    def step(self, frame_id, dets, regress, embed, warp):
        if frame_id == 0:
            self.tracks, self.num_tracks = {}, 0
        tr = dict(propagated=[], killed_score=[], killed_nms=[], suppressed=0, reid=[], gated=[], dropped=[], new=[])
        self.trace.append(tr)
        dets = np.asarray(dets, f32).reshape(-1, 5)
        kept = [d for d in dets if d[4] > f32(0.5)]
        rows = []
        if not self.tracks:
            emb = embed(np.array([d[:4] for d in kept], f32).reshape(-1, 4)) if kept else []
            for d, e in zip(kept, emb):
                rows.append((self.num_tracks, d[:4].copy(), d[4], np.asarray(e, f32)))
                tr["new"].append(self.num_tracks)
                self.num_tracks += 1
        else:
            M = np.asarray(warp, np.float64).reshape(2, 3).astype(f32)
            for t in self.tracks.values():                      # camera-motion compensation of every track's last box
                b = t["box"]
                t["box"] = np.array([f32(f32(M[0, 0] * b[0]) + f32(M[0, 1] * b[1])) + M[0, 2], f32(f32(M[1, 0] * b[0]) + f32(M[1, 1] * b[1])) + M[1, 2],
                                     f32(f32(M[0, 0] * b[2]) + f32(M[0, 1] * b[3])) + M[0, 2], f32(f32(M[1, 0] * b[2]) + f32(M[1, 1] * b[3])) + M[1, 2]], f32)
            prop_ids = [i for i, t in self.tracks.items() if t["frame"] == frame_id - 1]
            prop = []
            if prop_ids:
                rb, rs = regress(np.stack([self.tracks[i]["box"] for i in prop_ids]).astype(f32))
                rb, rs = np.asarray(rb, f32).reshape(-1, 4), np.asarray(rs, f32).reshape(-1)
                valid = [k for k in range(len(prop_ids)) if rs[k] > f32(0)]
                keep = obox.nms_mmcv(rb[valid], rs[valid], 0.6) if valid else []
                for k in range(len(prop_ids)):
                    if k in valid and valid.index(k) not in keep:
                        tr["killed_nms"].append(prop_ids[k])
                for j in keep:
                    k = valid[j]
                    if rs[k] > f32(0.5):
                        prop.append((prop_ids[k], rb[k], rs[k]))
                        tr["propagated"].append(prop_ids[k])
                    else:
                        tr["killed_score"].append(prop_ids[k])
                tr["killed_score"] += [prop_ids[k] for k in range(len(prop_ids)) if k not in valid]
            rest = []
            for d in kept:                                      # detections that do not overlap a propagated track
                hit = False
                for _, pb, _ in prop:
                    if bbox_overlaps(pb[None], d[None, :4])[0, 0] >= f32(0.3):
                        hit = True
                if hit:
                    tr["suppressed"] += 1
                else:
                    rest.append(d)
            all_boxes = np.array([p[1] for p in prop] + [d[:4] for d in rest], f32).reshape(-1, 4)
            emb = np.asarray(embed(all_boxes), f32).reshape(len(all_boxes), -1) if len(all_boxes) else np.zeros((0, 1), f32)
            prop_e, rest_e = emb[:len(prop)], emb[len(prop):]
            ids = [-1] * len(rest)
            cand = [i for i in self.tracks if i not in [p[0] for p in prop]]
            if cand and rest:
                cost = np.zeros((len(cand), len(rest)))
                for r, i in enumerate(cand):
                    e = self.tracks[i]["embeds"][-10:]
                    acc = np.zeros_like(e[0])
                    for v in e:
                        acc = (acc + v).astype(f32)
                    mean = (acc / f32(len(e))).astype(f32)
                    for c, d in enumerate(rest):
                        cost[r, c] = orm.cdist(mean[None], rest_e[c][None])[0, 0]
                        if bbox_overlaps(self.tracks[i]["box"][None], d[None, :4])[0, 0] < f32(0.2):
                            if cost[r, c] <= 2.0 and i not in tr["gated"]:
                                tr["gated"].append(i)           # the appearance alone would have accepted it
                            cost[r, c] = 1e6
                row, col = linear_sum_assignment(cost)
                for r, c in zip(row, col):
                    if cost[r, c] <= 2.0:
                        ids[c] = cand[r]
                        tr["reid"].append(cand[r])
            for c in range(len(rest)):
                if ids[c] < 0:
                    ids[c] = self.num_tracks
                    tr["new"].append(self.num_tracks)
                    self.num_tracks += 1
            for (i, b, s), e in zip(prop, prop_e):
                rows.append((i, b, s, e))
            for i, d, e in zip(ids, rest, rest_e):
                rows.append((i, d[:4].copy(), d[4], e))
        for i, b, s, e in rows:
            if i in self.tracks:
                t = self.tracks[i]
                t["box"], t["score"], t["frame"] = np.asarray(b, f32).copy(), s, frame_id
                t["embeds"].append(np.asarray(e, f32).copy())
            else:
                self.tracks[i] = dict(box=np.asarray(b, f32).copy(), score=s, frame=frame_id, embeds=[np.asarray(e, f32).copy()])
        for i in list(self.tracks):
            if frame_id - self.tracks[i]["frame"] >= 10:
                tr["dropped"].append(i)
                del self.tracks[i]
        return np.array([[i, *b, s] for i, b, s, _ in rows], f32).reshape(-1, 6)


# ---- RoI-head regression of given boxes ------------------------------------------------------------------------------------------
def regress_ref(model, feats, boxes_src, scale_factor):
    """boxes_src [n][4] float32 source pixels on ONE frame's FPN maps `feats` (odet.detect(..., want_intermediates=True)['feats'])
    -> (boxes [n][4] source pixels, scores [n])"""
    sf = np.asarray(scale_factor, f32)
    rois = (np.asarray(boxes_src, f32).reshape(-1, 4) * sf[None, :]).astype(f32)
    roi_feats, _ = odet.extract_roi_feats(feats[:4], rois)
    cls, reg = model.roi_head(roi_feats)
    out = odet.delta2bbox(rois, reg, stds=(0.1, 0.1, 0.2, 0.2))
    return (out / sf[None, :]).astype(f32), odet.softmax_fg(cls)


def reference_frames(model, frames_bgr):
    """the detector half of the chain, once per clip: per frame (dets, intermediates)"""
    out = []
    for f in frames_bgr:
        dets, mid = odet.detect(model, f[:, :, ::-1], want_intermediates=True)
        nw, nh = odet.rescale_size(f.shape[1], f.shape[0], (1088, 1088))
        mid["img_hw"] = (nh, nw)                             # the resized, un-padded input: what the ReID crops are clamped to
        out.append((dets, mid))
    return out


def reference_chain(model, reid, per_frame, gray):
    """per_frame: reference_frames(...); gray: gray_f32 or gray_f64 (what the chain's ECC is fed).
    -> (rows per frame, the tracker (its .trace), warps per frame, ECC iterations per frame)"""
    trk = TracktorRef()
    rows, warps, iters = [], [None], [0]
    for f, (dets, mid) in enumerate(per_frame):
        warp = None
        if f > 0:
            warp, _, it, status = ecc_euclidean(gray(per_frame[f - 1][1]["x"]), gray(mid["x"]))
            assert status == ECC_OK, (f, status)
            warps.append(warp)
            iters.append(it)
        regress = lambda b, mid=mid: regress_ref(model, mid["feats"], b, mid["scale_factor"])       # noqa: E731
        embed = lambda b, mid=mid: reid.forward(orm.crop_imgs(mid["x"], b, mid["scale_factor"], mid["img_hw"])) if len(b) else \
            np.zeros((0, 128), f32)                                                                      # noqa: E731
        rows.append(trk.step(f, dets, regress, embed, warp))
    return rows, trk, warps, iters
