"""NumPy restatement of the bottom-up stage's pre-processing rule, aggregation, heat-map parser, grouping and NMS.  TEST
INFRASTRUCTURE ONLY.

Written from the description of mmpose 0.x's bottom-up test path (BottomUpGetImgSize, flip_feature_maps / aggregate_stage_flip,
HeatmapParser.{nms, top_k, match, adjust, refine}, get_group_preds, oks_nms), not from the product code.  mmpose is not in the
reference tree, so this file is UNPINNED like what it checks.

`dtype` selects the arithmetic of the map side: float64 = the reference proper; float32 = the same statements rounded to float32
after every operation, the method as torch / numpy run it.  The gap between the two runs is the float32 error the tests scale
their bounds by.  Everything downstream of the maps (grouping, adjust, back-mapping, oks_nms) has ONE arithmetic, the one mmpose
uses (float32 rows, float64 where numpy promotes).
"""
from __future__ import annotations

import math

import numpy as np
from scipy.optimize import linear_sum_assignment

JOINT_ORDER = [0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16]
FLIP_INDEX = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
MAX_PEOPLE, DET_THR, TAG_THR, OKS_THR = 30, 0.1, 1.0, 0.9


# ---- section 2: the size rule ---------------------------------------------------------------------------------------------
def input_size(h, w, s=512):
    c64 = lambda v: int(math.ceil(v / 64.0) * 64)      # noqa: E731
    if w < h:
        wr, hr = s, c64(s / w * h)
        scale = np.array([w / 200.0, hr / wr * w / 200.0])
    else:
        wr, hr = c64(s / h * w), s
        scale = np.array([wr / hr * h / 200.0, h / 200.0])
    return wr, hr, np.array([round(w / 2.0), round(h / 2.0)], np.float64), scale


# ---- section 3: aggregation -------------------------------------------------------------------------------------------------
def _axis(n_in, n_out, align, dt):
    d = np.arange(n_out).astype(dt)
    if align:
        scale = dt(n_in - 1) / dt(n_out - 1) if n_out > 1 else dt(0)
        src = scale * d
    else:
        scale = dt(n_in) / dt(n_out)
        src = np.maximum(scale * (d + dt(0.5)) - dt(0.5), dt(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(dt)).astype(dt)
    return i0, i1, (dt(1) - l1).astype(dt), l1


def resize(x, hr, wr, align, dt):
    """F.interpolate(x [..][h][w], size=(hr, wr), mode='bilinear', align_corners=align) in dtype dt"""
    x = np.asarray(x).astype(dt)
    y0, y1, ly0, ly1 = _axis(x.shape[-2], hr, align, dt)
    x0, x1, lx0, lx1 = _axis(x.shape[-1], wr, align, dt)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    r0, r1 = x[..., y0, :], x[..., y1, :]
    out = ly0 * (lx0 * r0[..., x0] + lx1 * r0[..., x1]) + ly1 * (lx0 * r1[..., x0] + lx1 * r1[..., x1])
    assert out.dtype == dt
    return out


def aggregate(s0, s1, hr, wr, align, dt, flip_index=FLIP_INDEX):
    """s0 [2F][2K][h0][w0], s1 [2F][K][h1][w1] (samples F .. 2F-1 from the mirrored inputs) -> hm [F][K][hr][wr], tags [F][K][hr][wr][2]"""
    f, k = s0.shape[0] // 2, s1.shape[1]
    fi = np.asarray(flip_index)
    unflip = lambda m: m[..., ::-1][:, fi]      # noqa: E731  torch.flip(m, [3])[:, flip_index]
    h0, t0 = s0[:f, :k], s0[:f, k:]
    h0f, t0f = unflip(s0[f:, :k]), unflip(s0[f:, k:])
    h1, h1f = s1[:f], unflip(s1[f:])
    hm = np.zeros((f, k, hr, wr), dt)
    for m in (h0, h1, h0f, h1f):
        hm = hm + resize(m, hr, wr, align, dt)
    hm = hm / dt(4)
    tags = np.stack([resize(t0, hr, wr, align, dt), resize(t0f, hr, wr, align, dt)], axis=-1)
    assert hm.dtype == dt and tags.dtype == dt
    return hm, tags


# ---- section 3: candidates --------------------------------------------------------------------------------------------------
def nms_mask(hm):
    """pixel == max of its 5x5 neighbourhood (clipped to the map)"""
    h, w = hm.shape[-2:]
    pad = np.full(hm.shape[:-2] + (h + 4, w + 4), -np.inf, hm.dtype)
    pad[..., 2:-2, 2:-2] = hm
    mx = pad[..., 2:-2, 2:-2].copy()
    for dy in range(5):
        for dx in range(5):
            mx = np.maximum(mx, pad[..., dy:dy + h, dx:dx + w])
    return hm == mx


def top_k(hm, tags, m=MAX_PEOPLE):
    """hm [K][H][W], tags [K][H][W][2] of one frame -> dict(val [K][m], ind [K][m], x, y, tag [K][m][2], by, bx [K][m] bool).
    The survivors' map is hm * mask; the m largest, ties to the lower flat index."""
    k, h, w = hm.shape
    v = (hm * nms_mask(hm)).reshape(k, -1)
    ind = np.stack([np.lexsort((np.arange(h * w), -v[c]))[:m] for c in range(k)])
    val = np.take_along_axis(v, ind, axis=1)
    y, x = ind // w, ind % w
    c = np.arange(k)[:, None]
    by = hm[c, np.minimum(h - 1, y + 1), x] > hm[c, np.maximum(0, y - 1), x]
    bx = hm[c, y, np.minimum(w - 1, x + 1)] > hm[c, y, np.maximum(0, x - 1)]
    return dict(val=val, ind=ind, x=x, y=y, tag=tags[c, y, x], by=by, bx=bx)


# ---- section 4: grouping ----------------------------------------------------------------------------------------------------
def match_by_tag(val, x, y, tag, trace=None):
    """val, x, y [K][M], tag [K][M][2] -> persons [P][K][5] float32 (x, y, val, tag0, tag1) in the order the groups were opened.
    trace (list): every (unrounded distance) matrix the matching looked at."""
    k = val.shape[0]
    tag = np.asarray(tag, np.float32)
    default = np.zeros((k, 5), np.float32)
    joint_dict, tag_dict = {}, {}
    for i in range(k):
        idx = JOINT_ORDER[i]
        tags = tag[idx]
        joints = np.concatenate((np.stack([x[idx], y[idx]], 1).astype(np.int64), np.asarray(val[idx], np.float32)[:, None], tags), 1)
        mask = joints[:, 2] > DET_THR
        tags, joints = tags[mask], joints[mask]
        if joints.shape[0] == 0:
            continue
        if i == 0 or len(joint_dict) == 0:
            for t, j in zip(tags, joints):
                key = t[0]
                joint_dict.setdefault(key, np.copy(default))[idx] = j
                tag_dict[key] = [t]
        else:
            grouped_keys = list(joint_dict.keys())[:MAX_PEOPLE]
            grouped_tags = [np.mean(tag_dict[g], axis=0) for g in grouped_keys]
            diff = joints[:, None, 3:] - np.array(grouped_tags)[None, :, :]
            diff_normed = np.linalg.norm(diff, ord=2, axis=2)
            diff_saved = np.copy(diff_normed)
            if trace is not None:
                trace.append(diff_saved)
            diff_normed = np.round(diff_normed) * 100 - joints[:, 2:3]
            na, ng = diff.shape[:2]
            if na > ng:
                diff_normed = np.concatenate((diff_normed, np.zeros((na, na - ng), np.float32) + 1e10), axis=1)
            for row, col in zip(*linear_sum_assignment(diff_normed)):
                if row < na and col < ng and diff_saved[row][col] < TAG_THR:
                    key = grouped_keys[col]
                    joint_dict[key][idx] = joints[row]
                    tag_dict[key].append(tags[row])
                else:
                    key = tags[row][0]
                    joint_dict.setdefault(key, np.copy(default))[idx] = joints[row]
                    tag_dict[key] = [tags[row]]
    if not joint_dict:
        return np.zeros((0, k, 5), np.float32)
    return np.array([joint_dict[g] for g in joint_dict]).astype(np.float32)


def adjust(persons, hm):
    """+-0.25 towards the larger neighbour, + 0.5, for the joints with val > 0 (in place on a copy)"""
    out = persons.copy()
    h, w = hm.shape[-2:]
    for p in out:
        for c, j in enumerate(p):
            if j[2] > 0:
                xx, yy = int(j[0]), int(j[1])
                x, y = j[0], j[1]
                y += 0.25 if hm[c, min(h - 1, yy + 1), xx] > hm[c, max(0, yy - 1), xx] else -0.25
                x += 0.25 if hm[c, yy, min(w - 1, xx + 1)] > hm[c, yy, max(0, xx - 1)] else -0.25
                j[0], j[1] = x + 0.5, y + 0.5
    return out


def refine_person(hm, tags, person, dt, trace=None):
    """HeatmapParser.refine for one person [K][5]; hm [K][H][W], tags [K][H][W][2] in dtype dt"""
    k, h, w = hm.shape
    got = []
    for c in range(k):
        if person[c, 2] > 0:
            x, y = int(np.clip(int(person[c, 0]), 0, w - 1)), int(np.clip(int(person[c, 1]), 0, h - 1))
            got.append(tags[c, y, x])
    prev = np.mean(np.asarray(got, dt), axis=0).astype(dt)
    out = person.copy()
    filled = 0
    for c in range(k):
        d = (((tags[c] - prev[None, None, :]) ** 2).sum(axis=2) ** 0.5).astype(dt)
        norm = hm[c] - np.round(d)
        y, x = np.unravel_index(np.argmax(norm), norm.shape)
        val = hm[c, y, x]
        if trace is not None and person[c, 2] == 0:
            trace.append(dict(joint=c, d=d, hm=hm[c], y=int(y), x=int(x)))
        fx = x + 0.5 + (0.25 if hm[c, y, min(w - 1, x + 1)] > hm[c, y, max(0, x - 1)] else -0.25)
        fy = y + 0.5 + (0.25 if hm[c, min(h - 1, y + 1), x] > hm[c, max(0, y - 1), x] else -0.25)
        if val > 0 and person[c, 2] == 0:
            out[c, :3] = (fx, fy, val)
            filled += 1
    return out, filled


def get_group_preds(kpts, center, scale, wr, hr):
    out = np.array(kpts[..., :3], np.float32, copy=True)
    sc = np.asarray(scale, np.float64) * 200.0
    out[..., 0] = kpts[..., 0] * (sc[0] / wr) + center[0] - sc[0] * 0.5
    out[..., 1] = kpts[..., 1] * (sc[1] / hr) + center[1] - sc[1] * 0.5
    return out


def oks_iou(g, d, a_g, a_d):
    var = (SIGMAS * 2) ** 2
    ious = np.zeros(len(d), np.float32)
    for n in range(len(d)):
        dx, dy = d[n, 0::3] - g[0::3], d[n, 1::3] - g[1::3]
        e = (dx ** 2 + dy ** 2) / var / ((a_g + a_d[n]) / 2 + np.spacing(1)) / 2
        ious[n] = np.sum(np.exp(-e)) / len(e)
    return ious


def oks_nms(kpts, scores, thr=OKS_THR):
    if len(kpts) == 0:
        return []
    flat = np.array([kp.flatten() for kp in kpts])
    areas = np.array([(kp[:, 0].max() - kp[:, 0].min()) * (kp[:, 1].max() - kp[:, 1].min()) for kp in kpts])
    order = np.asarray(scores).argsort(kind="stable")[::-1]
    keep = []
    while len(order) > 0:
        i = order[0]
        keep.append(int(i))
        ovr = oks_iou(flat[i], flat[order[1:]], areas[i], areas[order[1:]])
        order = order[np.where(ovr <= thr)[0] + 1]
    return keep


def chain(s0, s1, hr, wr, center, scale, align=True, dt=np.float64, trace=None):
    """The whole post-processing of a chunk from its four low-resolution maps.  Returns one float32 (P, K, 3) array per frame.
    trace (dict): hm, tags, per frame the candidates / persons / scores / refine scans / distance matrices."""
    hm, tags = aggregate(s0, s1, hr, wr, align, dt)
    out, frames = [], []
    for f in range(hm.shape[0]):
        tk = top_k(hm[f], tags[f])
        dists, scans = [], []
        persons = match_by_tag(tk["val"], tk["x"], tk["y"], tk["tag"], trace=dists)
        adj = adjust(persons, hm[f])
        scores = [p[:, 2].mean() for p in adj]
        filled = 0
        ref = []
        for p in adj:
            r, n = refine_person(hm[f], tags[f], p, dt, trace=scans)
            ref.append(r)
            filled += n
        ref = np.array(ref, np.float32).reshape(-1, hm.shape[1], 5)
        pred = get_group_preds(ref, center, scale, wr, hr)
        keep = oks_nms(list(pred), scores)
        out.append(pred[keep] if keep else np.zeros((0, hm.shape[1], 3), np.float32))
        frames.append(dict(top=tk, persons=persons, adjusted=adj, scores=scores, refined=ref, filled=filled, dists=dists, scans=scans,
                           keep=keep))
    if trace is not None:
        trace.update(hm=hm, tags=tags, frames=frames)
    return out


# ---- section 2: the resize-align warp -----------------------------------------------------------------------------------------
def resize_align(frame, image_size):
    """BottomUpResizeAlign (scale 1, no UDP): frame [h][w][3] u8 -> (u8 [hr][wr][3], wr, hr, center, scale).  The three point pairs
    of get_affine_transform are float32, what is added up in front of them float64; the warp is the oracle's cv2.warpAffine."""
    from oracle import preprocess as opre
    h, w = frame.shape[:2]
    wr, hr, center, scale = input_size(h, w, image_size)
    scale_tmp = scale * 200.0
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0] = center
    src[1] = center + np.array([0.0, scale_tmp[0] * -0.5])
    dst[0] = [wr * 0.5, hr * 0.5]
    dst[1] = np.array([wr * 0.5, hr * 0.5]) + np.array([0.0, wr * -0.5])
    for p in (src, dst):
        d = p[0] - p[1]
        p[2] = p[1] + np.array([-d[1], d[0]], np.float32)
    trans = opre.get_affine_transform_cv(src, dst)
    return opre.warp_affine_u8(np.ascontiguousarray(frame), trans, (wr, hr)), wr, hr, center, scale


def network_input(frame_bgr, image_size, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """[3][hr][wr] float32: tensor channel c = channel c of the frame as read (the wrapper's BGR -> RGB and the loader's swap
    cancel, as in the top-down path), / 255, - mean[c], / std[c], each step in float32"""
    u8, wr, hr, center, scale = resize_align(frame_bgr, image_size)
    v = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    lut = ((v[None, :] - np.asarray(mean, np.float32)[:, None]).astype(np.float32) / np.asarray(std, np.float32)[:, None]).astype(np.float32)
    return np.stack([lut[c][u8[:, :, c]] for c in range(3)]), u8
