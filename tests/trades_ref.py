"""numpy restatements of the TraDeS stage (models/trades.py, csrc/trades.hip, tracking.TradesTracker), written from the published
method and independently of the product code; every arithmetic step takes a dtype so that the tests can measure the deviation of a
float32 evaluation from float64 (the project's tolerance rule).  The DLA-34 trunk, conv2d and dcn3x3 are tests/fairmot_ref.py's."""
import math

import numpy as np

from tests import fairmot_ref as F

f32 = np.float32


# ---- cost-volume association ----------------------------------------------------------------------------------------------------------
def softmax(x, axis, dtype):
    x = x.astype(dtype)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return (e / e.sum(axis=axis, keepdims=True)).astype(dtype)


def cva(cur, prev, dtype=np.float64, temperature=5):
    """cur, prev [hc][wc][d] -> (tracking_offset [2 hc][2 wc][2] (w, h), soft_h [P][hc], soft_w [P][wc], ch [P][hc], cw [P][wc])"""
    hc, wc, d = cur.shape
    c = (cur.reshape(-1, d).astype(dtype) @ prev.reshape(-1, d).astype(dtype).T).reshape(hc * wc, hc, wc)
    ch, cw = c.max(axis=2), c.max(axis=1)
    sh, sw = softmax(dtype(temperature) * ch, 1, dtype), softmax(dtype(temperature) * cw, 1, dtype)
    iq, jq = np.divmod(np.arange(hc * wc), wc)
    th = (2 * (np.arange(hc)[None, :] - iq[:, None])).astype(dtype)
    tw = (2 * (np.arange(wc)[None, :] - jq[:, None])).astype(dtype)
    off = np.stack([(sw * tw).sum(1), (sh * th).sum(1)], -1).reshape(hc, wc, 2)
    return np.repeat(np.repeat(off, 2, 0), 2, 1), sh, sw, ch, cw


def entropy(p):
    return -(p * np.log(np.maximum(p, 1e-300))).sum(-1)


# ---- pre-heat-map ------------------------------------------------------------------------------------------------------------------------
def gaussian_radius(det_size, min_overlap=0.7):
    height, width = det_size
    cands = []
    for a, b, c in ((1, height + width, width * height * (1 - min_overlap) / (1 + min_overlap)),
                    (4, 2 * (height + width), (1 - min_overlap) * width * height),
                    (4 * min_overlap, -2 * min_overlap * (height + width), (min_overlap - 1) * width * height)):
        cands.append((b + math.sqrt(b * b - 4 * a * c)) / 2)
    return min(cands)


def radius_centre(box):
    """box: float32 x1 y1 x2 y2 in network-input pixels -> (cx, cy, r) ints or None"""
    box = np.asarray(box, f32)
    h, w = box[3] - box[1], box[2] - box[0]
    if not (h > 0 and w > 0):
        return None
    r = max(0, int(gaussian_radius((math.ceil(h), math.ceil(w)))))
    ct = np.array([(box[0] + box[2]) / 2, (box[1] + box[3]) / 2], f32)
    return int(ct[0]), int(ct[1]), r


def render_prehm(boxes, hp, wp, dtype=np.float64):
    """boxes int [m][3] (cx, cy, r) -> draw_umich_gaussian of each on a zero map (elementwise max), then AvgPool2d(4, 4): [hp / 4][wp / 4]"""
    hm = np.zeros((hp, wp), dtype)
    for cx, cy, r in np.asarray(boxes, np.int64).reshape(-1, 3):
        d = 2 * r + 1
        sigma = dtype(d) / dtype(6)
        y, x = np.ogrid[-r:r + 1, -r:r + 1]
        g = np.exp(-(x * x + y * y).astype(dtype) / (dtype(2) * sigma * sigma)).astype(dtype)
        g[g < np.finfo(np.float64).eps * g.max()] = 0
        left, right = min(cx, r), min(wp - cx, r + 1)
        top, bottom = min(cy, r), min(hp - cy, r + 1)
        m = hm[cy - top:cy + bottom, cx - left:cx + right]
        np.maximum(m, g[r - top:r + bottom, r - left:r + right], out=m)
    return hm.reshape(hp // 4, 4, wp // 4, 4).transpose(0, 2, 1, 3).reshape(hp // 4, wp // 4, 16).sum(-1) / dtype(16)


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
def decode(hm, reg, ltrb, trk, K):
    """head maps of ONE frame [h][w][c] float32 -> (dets [K][9] float32 = ct, amodal bbox about the integer peak, tracking, score; inds [K])"""
    h, w = hm.shape[:2]
    s = F.sigmoid(hm.reshape(h, w), f32)
    pad = np.full((h + 2, w + 2), -np.inf, f32)
    pad[1:-1, 1:-1] = s
    mx = np.max([pad[i:i + h, j:j + w] for i in range(3) for j in range(3)], axis=0)
    peaks = np.flatnonzero((s == mx).reshape(-1))
    order = sorted(peaks.tolist(), key=lambda p: (-float(s.reshape(-1)[p]), p))[:K]
    dets = np.zeros((K, 9), f32)
    inds = np.full(K, -1, np.int64)
    regf, lf, tf = reg.reshape(-1, 2).astype(f32), ltrb.reshape(-1, 4).astype(f32), trk.reshape(-1, 2).astype(f32)
    for r, p in enumerate(order):
        y, x = divmod(p, w)
        dets[r] = (f32(x) + regf[p, 0], f32(y) + regf[p, 1], f32(x) + lf[p, 0], f32(y) + lf[p, 1], f32(x) + lf[p, 2], f32(y) + lf[p, 3],
                   tf[p, 0], tf[p, 1], s.reshape(-1)[p])
        inds[r] = p
    return dets, inds


# ---- tracker -----------------------------------------------------------------------------------------------------------------------------
class TrackerRef:
    """CenterTrack's Tracker.step, max_age = -1, greedy; also records the quantities the tests need to rule out ties and gates on
    their thresholds (`log`: per frame the distance matrix before invalidation, the two areas, and the greedy choices)"""

    def __init__(self, new_thresh=0.5):
        self.new_thresh, self.next_id, self.tracks, self.log = new_thresh, 0, [], []

    def step(self, results):
        n, m = len(results), len(self.tracks)
        dist = np.zeros((n, m), f32)
        for i, d in enumerate(results):
            p = np.asarray(d["ct"], f32) + np.asarray(d["tracking"], f32)
            for j, t in enumerate(self.tracks):
                q = np.asarray(t["ct"], f32) - p
                dist[i, j] = q[0] * q[0] + q[1] * q[1]
        area = lambda b: f32(b[2] - b[0]) * f32(b[3] - b[1])       # noqa: E731
        ta = np.array([area(t["bbox"]) for t in self.tracks], f32)
        da = np.array([area(d["bbox"]) for d in results], f32)
        cost = dist.astype(np.float64)
        for i in range(n):
            for j in range(m):
                if dist[i, j] > ta[j] or dist[i, j] > da[i]:
                    cost[i, j] += 1e18
        frame_log = dict(dist=dist.copy(), track_area=ta, det_area=da, rows=[])
        used, out, matched = set(), [], set()
        for i in range(n):
            if m == 0:
                break
            row = np.array([1e18 if j in used else cost[i, j] for j in range(m)])
            frame_log["rows"].append(row.copy())
            j = int(np.argmin(row))
            if row[j] < 1e16:
                used.add(j)
                matched.add(i)
                out.append((i, self.tracks[j]["id"]))
        ret = [dict(results[i], id=tid) for i, tid in out]
        for i in range(n):
            if i not in matched and results[i]["score"] > self.new_thresh:
                self.next_id += 1
                ret.append(dict(results[i], id=self.next_id))
        self.tracks = ret
        self.log.append(frame_log)
        return [(t["id"], t) for t in ret]


# ---- program B and the network ---------------------------------------------------------------------------------------------------------------
def program_b(sd, feat_cur, feat_prev, trk, pre_hm, dtype=np.float64):
    """-> dict(offset_mask [h][w][27] with unit-mask logits left out (only the 18 offsets), prop, enhanced, heads...)"""
    dt = dtype
    cur, prev = feat_cur.astype(dt), feat_prev.astype(dt)
    diff = cur - prev
    off_w9 = F.conv2d(np.concatenate([trk[..., 0:1].astype(dt), diff], -1), sd["conv_offset_w.weight"], sd["conv_offset_w.bias"], 1, 1, dt)
    off_h9 = F.conv2d(np.concatenate([trk[..., 1:2].astype(dt), diff], -1), sd["conv_offset_h.weight"], sd["conv_offset_h.bias"], 1, 1, dt)
    offsets = np.stack([off_h9, off_w9], -1).reshape(off_h9.shape[:2] + (18,))            # 2k = dy = h, 2k + 1 = dx = w
    om = np.concatenate([offsets, np.full(offsets.shape[:2] + (9,), 1e4, dt)], -1)         # sigmoid(1e4) = 1: the mask of ones
    gated = pre_hm.reshape(pre_hm.shape[:2] + (1,)).astype(dt) * prev
    prop = F.dcn3x3(gated, om, sd["dcn1_1.weight"], sd["dcn1_1.bias"], False, dt)
    la = F.conv2d(cur, sd["attention_cur.weight"], sd["attention_cur.bias"], 1, 1, dt)
    lb = F.conv2d(prop, sd["attention_prev.weight"], sd["attention_prev.bias"], 1, 1, dt)
    a = softmax(np.concatenate([la, lb], -1), -1, dt)
    enh = a[..., 0:1] * cur + a[..., 1:2] * prop
    out = dict(offsets=offsets, gated=gated, diff=diff, prop=prop, enhanced=enh, attention=a)
    for head in ("hm", "reg", "wh", "ltrb_amodal"):
        t = np.maximum(F.conv2d(enh, sd[head + ".0.weight"], sd[head + ".0.bias"], 1, 1, dt), 0)
        out[head] = F.conv2d(t, sd[head + ".2.weight"], sd[head + ".2.bias"], 1, 0, dt)
    return out


class TrunkRef(F.Dla34Ref):
    """feat (64 channels, stride 4) and emb' (embedconv + MaxPool2d(2, 2)) of one frame"""

    def forward(self, x):
        sd = self.sd
        x = x[..., :3].astype(self.dt)
        x = self.convbn(x, "base.base_layer.0", "base.base_layer.1")
        y = [self.convbn(x, "base.level0.0", "base.level0.1")]
        y.append(self.convbn(y[0], "base.level1.0", "base.level1.1", 2))
        levels, ch = (1, 1, 1, 2, 2, 1), (16, 32, 64, 128, 256, 512)
        for lv in range(2, 6):
            y.append(self.tree(y[-1], f"base.level{lv}", levels[lv], ch[lv - 1], ch[lv], 2, lv >= 3))
        out = [y[-1]]
        for i in range(3):
            self.ida(y, f"dla_up.ida_{i}", len(y) - i - 2, len(y))
            out.insert(0, y[-1])
        z = out[:3]
        self.ida(z, "ida_up", 0, 3)
        feat = z[-1]
        e = np.maximum(F.conv2d(feat, sd["embedconv.0.weight"], sd["embedconv.0.bias"], 1, 1, self.dt), 0)
        e = np.maximum(F.conv2d(e, sd["embedconv.2.weight"], sd["embedconv.2.bias"], 1, 1, self.dt), 0)
        e = F.conv2d(e, sd["embedconv.4.weight"], sd["embedconv.4.bias"], 1, 0, self.dt)
        return feat, F.maxpool2(e)


# ---- the whole chain (tests/golden/make_goldens_trades.py) ---------------------------------------------------------------------------------
def input_size(src_h, src_w):
    return (864, 480) if src_h > src_w else (480, 864)


def affine(src_h, src_w, ow, oh, inv=False):
    """get_affine_transform(c = (w / 2, h / 2), s = max(h, w), 0, (ow, oh)) in closed form: a scale about the two centres"""
    s = ow / max(src_h, src_w)
    if inv:
        return np.array([[1 / s, 0, src_w / 2 - ow / 2 / s], [0, 1 / s, src_h / 2 - oh / 2 / s]])
    return np.array([[s, 0, ow / 2 - s * src_w / 2], [0, s, oh / 2 - s * src_h / 2]])


def _pt(p, m):
    return m @ np.r_[np.asarray(p, f32), f32(1)].astype(np.float64)


def prehm_boxes(tracks, m, hp, wp, pre_thresh=0.5):
    out = []
    for t in tracks:
        if t["score"] < pre_thresh:
            continue
        b = np.r_[_pt(t["bbox"][:2], m), _pt(t["bbox"][2:], m)].astype(f32)
        b[[0, 2]], b[[1, 3]] = np.clip(b[[0, 2]], 0, wp - 1), np.clip(b[[1, 3]], 0, hp - 1)
        rc = radius_centre(b)
        if rc is not None:
            out.append(rc)
    return np.array(out, np.int64).reshape(-1, 3)


def post_process(dets, minv, out_thresh=0.5):
    out = []
    for d in dets:
        if d[8] < out_thresh:
            break
        ct = _pt(d[0:2], minv).astype(f32)
        out.append({"score": float(d[8]), "ct": ct, "tracking": _pt(d[0:2] + d[6:8], minv).astype(f32) - ct,
                    "bbox": np.r_[_pt(d[2:4], minv), _pt(d[4:6], minv)].astype(f32)})
    return out


def preprocess(frame_bgr, oracle_pre, mean, std):
    """the reference wrapper's cvtColor(COLOR_RGB2BGR) on the decoded BGR frame, CenterTrack's fix_res warp, (x / 255 - mean) / std
    -> [hp][wp][3] float32 (oracle_pre = oracle.preprocess: its warpAffine and table are what the device kernel is held to)"""
    h, w = frame_bgr.shape[:2]
    hp, wp = input_size(h, w)
    img = oracle_pre.warp_affine_u8(np.ascontiguousarray(frame_bgr[:, :, ::-1]), affine(h, w, wp, hp), (wp, hp))
    lut = oracle_pre.normalize_lut(np.asarray(mean, f32), np.asarray(std, f32))
    return np.stack([lut[c][img[..., c]] for c in range(3)], -1).astype(f32)


def chain(sd, frames_bgr, dtype, oracle_pre, mean, std, K=100, trunk_cache=None):
    """pre-processing -> trunk -> CVA -> pre_hm -> program B -> decode -> post-processing -> TrackerRef, every network layer in `dtype`.
    -> (per frame [(id, bbox float32 [4], score)], per frame dict(scores of all decoded peaks by flat index), TrackerRef)"""
    h, w = frames_bgr.shape[1:3]
    hp, wp = input_size(h, w)
    m_in, m_inv = affine(h, w, wp, hp), affine(h, w, wp // 4, hp // 4, inv=True)
    trunk, tracker = TrunkRef(sd, dtype), TrackerRef(0.5)
    rows, peaks, prev = [], [], None
    for f, frame in enumerate(frames_bgr):
        key = (f, np.dtype(dtype).name)
        if trunk_cache is not None and key in trunk_cache:
            feat, emb = trunk_cache[key]
        else:
            feat, emb = trunk.forward(preprocess(frame, oracle_pre, mean, std))
            if trunk_cache is not None:
                trunk_cache[key] = (feat, emb)
        if prev is None:
            prev = (feat, emb)                       # frame 0's previous frame is itself
        trk = cva(emb, prev[1], dtype)[0]
        pre_hm = render_prehm(prehm_boxes(tracker.tracks, m_in, hp, wp), hp, wp, dtype)
        b = program_b(sd, feat, prev[0], trk, pre_hm, dtype)
        dets, inds = decode(b["hm"].astype(f32), b["reg"].astype(f32), b["ltrb_amodal"].astype(f32), trk.astype(f32), K)
        peaks.append({int(i): float(d[8]) for i, d in zip(inds, dets) if i >= 0})
        out = tracker.step(post_process(dets, m_inv))
        rows.append([(i, t["bbox"], t["score"]) for i, t in out])
        prev = (feat, emb)
    return rows, peaks, tracker
