"""The bottom-up 2D stage: HigherHRNet-W48 + associative embedding, as `mmpose_bottom_up` runs it.

Replaces `inference_bottom_up_pose_model` of mmpose 0.x (pose_pipeline/wrappers/mmpose.py:113) with the test_cfg of the vendored
config 3rdparty/mmpose/config/bottom_up/higherhrnet/coco/higher_hrnet48_coco_512x512.py:109-125.  mmpose is not in the
reference tree: everything below that restates its code is UNPINNED (INTEGRATION.md lists the parts).

Where the work runs:
  device  resize-align warp + normalise + mirrored copy (pp_warp_affine_normalize), the network on 2F samples, flip / resize /
          average of the heat-maps, 5x5 NMS + top-30 per joint, the refine arg-max (csrc/bottomup.hip);
  host    grouping by tag (`match_by_tag`: sequential, 17 joints x <= 30 candidates, Hungarian through pp_linear_sum_assignment),
          the +-0.25 adjustment from the two comparison bits the device returns, the back-mapping and `oks_nms`.
The host never reads a map.
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import _lib as L
from . import ops

# normalisation of the val pipeline (higher_hrnet48_coco_512x512.py:158-162)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# test_cfg of the vendored config (:109-125) without num_joints
TEST_CFG = dict(max_num_people=30, scale_factor=[1], with_heatmaps=[True, True], with_ae=[True, False], project2image=True,
                nms_kernel=5, nms_padding=2, tag_per_joint=True, detection_threshold=0.1, tag_threshold=1, use_detection_val=True,
                ignore_too_much=False, adjust=True, refine=True, flip_test=True)
# HeatmapParser's joint order for COCO (restated)
JOINT_ORDER = (0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16)
# COCO keypoint sigmas (restated: the dataset_info `inference_bottom_up_pose_model` hands oks_nms)
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
OKS_NMS_THR = 0.9          # pose_nms_thr default of inference_bottom_up_pose_model
# test_cfg.get('align_corners', True) of BottomUp.forward_test: the vendored config does not set it
ALIGN_CORNERS = True


# ---- pre-processing rule (BottomUpGetImgSize, scale 1, no UDP) --------------------------------------------------------------
def input_size(h, w, image_size=512):
    """source h x w -> (wr, hr, center (2,) float64, scale (2,) float64 in units of 200 px)"""
    s = int(image_size)
    ceil64 = lambda v: int(math.ceil(v / 64.0)) * 64      # noqa: E731
    if w < h:
        wr, hr = s, ceil64(s / w * h)
        scale = (w / 200.0, hr / wr * w / 200.0)
    else:
        wr, hr = ceil64(s / h * w), s
        scale = (wr / hr * h / 200.0, h / 200.0)
    center = (float(round(w / 2.0)), float(round(h / 2.0)))
    return wr, hr, np.array(center, np.float64), np.array(scale, np.float64)


# ---- grouping (HeatmapParser._match_by_tag) ---------------------------------------------------------------------------------
def match_by_tag(cand, cfg=TEST_CFG, joint_order=JOINT_ORDER):
    """cand [K][M][C >= 5] float32: per joint and candidate (val, x, y, tag0, tag1, extra columns ...) as pp_bottomup_candidates
    returns them.  Returns persons [P][K][C] float32 in the same column layout (rows of undetected joints are zeros), in the
    order the groups were opened.  Groups are keyed by the float value of tag dimension 0 (equal keys merge: mmpose's quirk)."""
    from .tracking import linear_sum_assignment
    cand = np.asarray(cand, np.float32)
    k, _, ncol = cand.shape
    default = np.zeros((k, ncol), np.float32)
    joint_dict, tag_dict = {}, {}
    for i in range(k):
        idx = joint_order[i]
        rows = cand[idx]
        rows = rows[rows[:, 0].astype(np.float64) > cfg["detection_threshold"]]      # mmpose's rows are float64 here
        if rows.shape[0] == 0:
            continue
        tags = rows[:, 3:5]
        if i == 0 or len(joint_dict) == 0:
            for tag, row in zip(tags, rows):
                key = tag[0]
                joint_dict.setdefault(key, np.copy(default))[idx] = row
                tag_dict[key] = [tag]
            continue
        grouped_keys = list(joint_dict.keys())[:cfg["max_num_people"]]
        grouped_tags = [np.mean(tag_dict[g], axis=0) for g in grouped_keys]
        if cfg["ignore_too_much"] and len(grouped_keys) == cfg["max_num_people"]:
            continue
        # mmpose's `joints` is float64 (integer locations concatenated with float32 values); the group means are float32
        diff = tags.astype(np.float64)[:, None, :] - np.array(grouped_tags)[None, :, :]
        diff_normed = np.linalg.norm(diff, ord=2, axis=2)
        diff_saved = np.copy(diff_normed)
        if cfg["use_detection_val"]:
            diff_normed = np.round(diff_normed) * 100 - rows[:, 0:1].astype(np.float64)
        num_added, num_grouped = diff.shape[0], diff.shape[1]
        if num_added > num_grouped:
            diff_normed = np.concatenate((diff_normed, np.zeros((num_added, num_added - num_grouped), np.float32) + 1e10), axis=1)
        for row, col in zip(*linear_sum_assignment(diff_normed)):
            if row < num_added and col < num_grouped and diff_saved[row][col] < cfg["tag_threshold"]:
                key = grouped_keys[col]
                joint_dict[key][idx] = rows[row]
                tag_dict[key].append(tags[row])
            else:
                key = tags[row][0]
                joint_dict.setdefault(key, np.copy(default))[idx] = rows[row]
                tag_dict[key] = [tags[row]]
    if not joint_dict:
        return np.zeros((0, k, ncol), np.float32)
    return np.array([joint_dict[g] for g in joint_dict]).astype(np.float32)


def adjust(persons):
    """HeatmapParser.adjust from the comparison bits: persons [P][K][>= 7] (val, x, y, t0, t1, bit_y, bit_x) -> xy [P][K][2] float32:
    +-0.25 towards the larger neighbour, then + 0.5, for the joints with val > 0 (the others keep their zeros)"""
    p = np.asarray(persons, np.float32)
    xy = p[:, :, 1:3].copy()
    q = np.float32(0.25)
    on = p[:, :, 0] > 0
    xy[:, :, 0] = np.where(on, xy[:, :, 0] + np.where(p[:, :, 6] > 0, q, -q) + np.float32(0.5), xy[:, :, 0])
    xy[:, :, 1] = np.where(on, xy[:, :, 1] + np.where(p[:, :, 5] > 0, q, -q) + np.float32(0.5), xy[:, :, 1])
    return xy.astype(np.float32)


def get_group_preds(kpts, center, scale, wr, hr):
    """transform_preds of every person: kpts [P][K][3] float32 (x, y, val) in map pixels -> image pixels (float64 arithmetic
    stored to float32, the value column kept)"""
    out = np.array(kpts, np.float32, copy=True)
    sc = np.asarray(scale, np.float64) * 200.0
    out[..., 0] = out[..., 0].astype(np.float64) * (sc[0] / wr) + center[0] - sc[0] * 0.5
    out[..., 1] = out[..., 1].astype(np.float64) * (sc[1] / hr) + center[1] - sc[1] * 0.5
    return out


def oks_iou(g, d, a_g, a_d, sigmas=COCO_SIGMAS):
    vars_ = (np.asarray(sigmas, np.float64) * 2) ** 2
    xg, yg = g[0::3], g[1::3]
    ious = np.zeros(len(d), np.float32)
    for n in range(len(d)):
        dx, dy = d[n, 0::3] - xg, d[n, 1::3] - yg
        e = (dx ** 2 + dy ** 2) / vars_ / ((a_g + a_d[n]) / 2 + np.spacing(1)) / 2
        ious[n] = np.sum(np.exp(-e)) / len(e) if len(e) != 0 else 0.0
    return ious


def oks_nms(kpts, scores, thr=OKS_NMS_THR, sigmas=COCO_SIGMAS):
    """kpts [P][K][3] float32, scores [P]: indices kept, in descending score (vis_thr=None; area = the key points' bounding box)"""
    kpts = np.asarray(kpts, np.float32)
    if len(kpts) == 0:
        return np.zeros(0, np.int64)
    flat = kpts.reshape(len(kpts), -1)
    areas = (kpts[:, :, 0].max(axis=1) - kpts[:, :, 0].min(axis=1)) * (kpts[:, :, 1].max(axis=1) - kpts[:, :, 1].min(axis=1))
    order = np.asarray(scores).argsort(kind="stable")[::-1]
    keep = []
    while len(order) > 0:
        i = order[0]
        keep.append(i)
        ovr = oks_iou(flat[i], flat[order[1:]], areas[i], areas[order[1:]], sigmas)
        order = order[np.where(ovr <= thr)[0] + 1]
    return np.array(keep, np.int64)


# ---- the device side ----------------------------------------------------------------------------------------------------------
def warp_affine_normalize(ctx, frames, center, scale, out_wh, lut=None, chan_map=(0, 1, 2), flip=True, out_dev=None,
                          frames_dev_shape=None, want_u8=False):
    """BottomUpResizeAlign + ToTensor + NormalizeTensor (+ the mirrored copies) of every frame.  frames: numpy [F][H][W][3] u8
    (-> returns out [F or 2F][oh][ow][4] float32 and the u8 warp when asked) or a device pointer with frames_dev_shape = (F, H, W)
    and out_dev = the device pointer to write."""
    ow, oh = out_wh
    lut = ops.normalize_lut(MEAN, STD) if lut is None else np.ascontiguousarray(lut, np.float32)
    cm = np.asarray(chan_map, np.int32)
    c = np.ascontiguousarray(center, np.float64)
    s = np.ascontiguousarray(scale, np.float64)
    if isinstance(frames, np.ndarray):
        frames = np.ascontiguousarray(frames, np.uint8)
        f, h, w, _ = frames.shape
        out = np.empty((f * (2 if flip else 1), oh, ow, 4), np.float32)
        u8 = np.empty((f, oh, ow, 3), np.uint8) if want_u8 else None
        L.check(ctx.lib.pp_warp_affine_normalize(ctx.handle, L.ptr(frames), f, h, w, L.ptr(c), L.ptr(s), ow, oh, L.ptr(lut), L.ptr(cm),
                                                 int(bool(flip)), L.ptr(out), L.ptr(u8), L.PP_MEM_HOST), "pp_warp_affine_normalize")
        return (out, u8) if want_u8 else out
    f, h, w = frames_dev_shape
    L.check(ctx.lib.pp_warp_affine_normalize(ctx.handle, L.ptr(int(frames)), f, h, w, L.ptr(c), L.ptr(s), ow, oh, L.ptr(lut), L.ptr(cm),
                                             int(bool(flip)), L.ptr(int(out_dev)), None, L.PP_MEM_DEVICE), "pp_warp_affine_normalize")
    return None


class MapSet:
    """The two low-resolution outputs of one chunk on the device, s0 [2F][2K][h0][w0] and s1 [2F][K][h1][w1] (samples F .. 2F-1 from
    the mirrored inputs), and the aggregated heat-maps [F][K][hr][wr] behind the three post-processing calls.  s0 / s1: device
    pointers (borrowed) or numpy arrays (uploaded, owned)."""

    def __init__(self, ctx, s0, s1, n_frames, k, hw0, hw1, hr, wr, flip_perm, align_corners=ALIGN_CORNERS, hm_dev=None):
        self.ctx, self.f, self.k = ctx, int(n_frames), int(k)
        (self.h0, self.w0), (self.h1, self.w1), self.hr, self.wr = hw0, hw1, int(hr), int(wr)
        self.perm = np.ascontiguousarray(flip_perm, np.int32)
        assert self.perm.shape == (self.k,)
        self.align = int(bool(align_corners))
        self._own = []
        self.s0 = self._dev(s0, (2 * self.f, 2 * self.k, self.h0, self.w0))
        self.s1 = self._dev(s1, (2 * self.f, self.k, self.h1, self.w1))
        if hm_dev is None:
            hm_dev = ctx.malloc(max(self.f, 1) * self.k * self.hr * self.wr * 4)
            self._own.append(hm_dev)
        self.hm = int(hm_dev)

    def _dev(self, a, shape):
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, np.float32)
            assert a.shape == shape, (a.shape, shape)
            d = self.ctx.malloc(max(a.nbytes, 4))
            self._own.append(d)
            self.ctx.h2d(d, a)
            return d
        return int(a)

    def close(self):
        for d in self._own:
            self.ctx.free(d)
        self._own = []

    def aggregate(self):
        L.check(self.ctx.lib.pp_bottomup_aggregate(self.ctx.handle, L.ptr(self.s0), L.ptr(self.s1), self.f, self.k, self.h0, self.w0,
                                                   self.h1, self.w1, L.ptr(self.perm), self.hr, self.wr, self.align, L.ptr(self.hm)),
                "pp_bottomup_aggregate")

    def heatmaps(self):
        """the aggregated maps on the host (tests)"""
        out = np.empty((self.f, self.k, self.hr, self.wr), np.float32)
        self.ctx.d2h(out, self.hm)
        return out

    def candidates(self, max_people=TEST_CFG["max_num_people"]):
        """[F][K][max_people][8] float32 (val, x, y, tag0, tag1, bit_y, bit_x, flat index), see include/posepipe_hip.h"""
        cand = np.empty((self.f, self.k, int(max_people), 8), np.float32)
        L.check(self.ctx.lib.pp_bottomup_candidates(self.ctx.handle, L.ptr(self.hm), L.ptr(self.s0), self.f, self.k, self.h0, self.w0,
                                                    L.ptr(self.perm), self.hr, self.wr, self.align, int(max_people), L.ptr(cand)),
                "pp_bottomup_candidates")
        return cand

    def refine(self, person_frame, mean_tag, need):
        """[P][K][4] float32 (x, y, val, bits) of the joints with need != 0"""
        pf = np.ascontiguousarray(person_frame, np.int32)
        mt = np.ascontiguousarray(mean_tag, np.float32).reshape(len(pf), 2)
        nd = np.ascontiguousarray(need, np.int32).reshape(len(pf), self.k)
        out = np.zeros((len(pf), self.k, 4), np.float32)
        L.check(self.ctx.lib.pp_bottomup_refine(self.ctx.handle, L.ptr(self.hm), L.ptr(self.s0), self.f, self.k, self.h0, self.w0,
                                                L.ptr(self.perm), self.hr, self.wr, self.align, len(pf), L.ptr(pf), L.ptr(mt), L.ptr(nd),
                                                L.ptr(out)), "pp_bottomup_refine")
        return out


def parse_chunk(maps: MapSet, center, scale, cfg=TEST_CFG, timing=None, trace=None):
    """HeatmapParser.parse + get_group_preds + oks_nms for every frame of a chunk whose maps are aggregated.  Returns one float32
    (P, K, 3) array per frame (x_px, y_px, val), persons in descending score.  trace (a dict, tests): per-stage intermediates."""
    t = time.perf_counter()
    cand = maps.candidates(cfg["max_num_people"])
    t = _lap(timing, "candidates", t)
    persons = [match_by_tag(cand[f], cfg) for f in range(maps.f)]
    xy = [adjust(p) if cfg["adjust"] else p[:, :, 1:3].copy() for p in persons]
    scores = [p[:, :, 0].mean(axis=1) if len(p) else np.zeros(0, np.float32) for p in persons]
    kpts = [np.concatenate([c, p[:, :, 0:1]], axis=2).astype(np.float32) for c, p in zip(xy, persons)]
    t = _lap(timing, "group", t)
    filled = 0
    if cfg["refine"]:
        frame_of = np.concatenate([np.full(len(p), f, np.int32) for f, p in enumerate(persons)]) if persons else np.zeros(0, np.int32)
        if len(frame_of):
            allp = np.concatenate(persons)
            on = allp[:, :, 0] > 0
            mean_tag = np.stack([np.mean(pp[o][:, 3:5], axis=0) for pp, o in zip(allp, on)]).astype(np.float32)
            need = (allp[:, :, 0] == 0).astype(np.int32)
            if need.any():
                r = maps.refine(frame_of, mean_tag, need)
                q = np.float32(0.25)
                rx = r[:, :, 0] + np.float32(0.5) + np.where(r[:, :, 3].astype(np.int32) & 2, q, -q)
                ry = r[:, :, 1] + np.float32(0.5) + np.where(r[:, :, 3].astype(np.int32) & 1, q, -q)
                use = (need != 0) & (r[:, :, 2] > 0)
                filled = int(use.sum())
                off = 0
                for kp in kpts:
                    n = len(kp)
                    u = use[off:off + n]
                    kp[:, :, 0] = np.where(u, rx[off:off + n], kp[:, :, 0])
                    kp[:, :, 1] = np.where(u, ry[off:off + n], kp[:, :, 1])
                    kp[:, :, 2] = np.where(u, r[off:off + n, :, 2], kp[:, :, 2])
                    off += n
    t = _lap(timing, "refine", t)
    out = []
    for kp, sc in zip(kpts, scores):
        pred = get_group_preds(kp, center, scale, maps.wr, maps.hr)
        keep = oks_nms(pred, sc)
        out.append(pred[keep] if len(keep) else np.zeros((0, maps.k, 3), np.float32))
    _lap(timing, "nms", t)
    if trace is not None:
        trace.update(cand=cand, persons=persons, scores=scores, refined=filled, kpts=kpts)
    return out


def _lap(timing, name, t0):
    t1 = time.perf_counter()
    if timing is not None:
        timing[name] = timing.get(name, 0.0) + (t1 - t0)
    return t1


CHUNK = 8        # frames per program run: 16 network samples with the mirrored copies


class BottomUpStage:
    """The network + the post-processing for one spec, resident on one device.  The program depends on the padded input size,
    which depends on the clip's frame size: nets are built per (hp, wp) and kept."""

    def __init__(self, spec=None, device=0, max_frames=CHUNK, numerics=None, ctx=None, state_dict=None, chan_map=(0, 1, 2)):
        from .models import higherhrnet
        self.spec = higherhrnet.higher_hrnet48_coco_512x512() if spec is None else spec
        self.ctx = L.Context(device) if ctx is None else ctx
        self.max_frames, self.numerics, self.sd = int(max_frames), numerics, state_dict
        from .models.hrnet import flip_perm
        self.flip_perm = flip_perm(self.spec.num_joints)
        self.chan_map = tuple(chan_map)
        self.lut = ops.normalize_lut(MEAN, STD)
        self.nets: dict = {}
        self.hm_dev, self.hm_bytes = None, 0
        self.last_timing: dict = {}

    def state_dict(self):
        if self.sd is None:
            from . import weights
            from .models import higherhrnet
            self.sd = weights.get_state_dict(CHECKPOINT, higherhrnet.higherhrnet_param_shapes(self.spec), seed=1)
        return self.sd

    def net(self, hp, wp):
        if (hp, wp) not in self.nets:
            from .models import higherhrnet
            from .program import Net
            prog = higherhrnet.build_higherhrnet_program(self.spec, self.state_dict(), hp, wp)
            self.nets[(hp, wp)] = Net(self.ctx, prog, max_batch=2 * self.max_frames, numerics=self.numerics)
        return self.nets[(hp, wp)]

    def _hm(self, nbytes):
        if nbytes > self.hm_bytes:
            if self.hm_dev is not None:
                self.ctx.free(self.hm_dev)
            self.hm_dev, self.hm_bytes = self.ctx.malloc(nbytes), nbytes
        return self.hm_dev

    def run(self, frames, frames_dev_shape=None, trace=None):
        """frames: numpy [F][H][W][3] u8 BGR, or a device pointer with frames_dev_shape = (F, H, W).  Returns one float32
        (P, K, 3) array per frame."""
        timing = self.last_timing
        if isinstance(frames, np.ndarray):
            f, h, w = frames.shape[:3]
            fdev = self.ctx.malloc(frames.nbytes)
            self.ctx.h2d(fdev, np.ascontiguousarray(frames, np.uint8))
        else:
            (f, h, w), fdev = frames_dev_shape, int(frames)
        assert 0 < f <= self.max_frames, (f, self.max_frames)
        try:
            wr, hr, center, scale = input_size(h, w, self.spec.image_size)
            net = self.net(hr, wr)
            t = time.perf_counter()
            warp_affine_normalize(self.ctx, fdev, center, scale, (wr, hr), self.lut, self.chan_map, True, out_dev=net.buffer("input")[0],
                                  frames_dev_shape=(f, h, w))
            t = _lap(timing, "preprocess", t)
            net.run(2 * f)
            self.ctx.synchronize()
            _lap(timing, "network", t)
        finally:
            if isinstance(frames, np.ndarray):
                self.ctx.free(fdev)
        k = self.spec.num_joints
        return self.run_maps(net.buffer("output0")[0], net.buffer("output1")[0], f, (hr // 4, wr // 4), (hr // 2, wr // 2), (h, w), trace=trace)

    def run_maps(self, s0, s1, n_frames, hw0, hw1, src_hw, align_corners=ALIGN_CORNERS, trace=None):
        """The post-processing on the four low-resolution maps directly: s0 [2F][2K][h0][w0], s1 [2F][K][h1][w1] (plain samples,
        then the mirrored ones), numpy or device pointers; src_hw: the frame size the results are mapped back to."""
        timing = self.last_timing
        wr, hr, center, scale = input_size(src_hw[0], src_hw[1], self.spec.image_size)
        k = self.spec.num_joints
        maps = MapSet(self.ctx, s0, s1, n_frames, k, hw0, hw1, hr, wr, self.flip_perm, align_corners,
                      hm_dev=self._hm(n_frames * k * hr * wr * 4))
        try:
            t = time.perf_counter()
            maps.aggregate()
            _lap(timing, "aggregate", t)
            if trace is not None:
                trace["hm"] = maps.heatmaps()
            return parse_chunk(maps, center, scale, timing=timing, trace=trace)
        finally:
            maps.close()

    def close(self):
        for n in self.nets.values():
            n.close()
        self.nets = {}
        if self.hm_dev is not None and getattr(self.ctx, "handle", None):
            self.ctx.free(self.hm_dev)
        self.hm_dev, self.hm_bytes = None, 0


# the checkpoint `mmpose_bottom_up` first assigns (wrappers/mmpose.py:92), under MODEL_DATA_DIR
CHECKPOINT = "mmpose/checkpoints/higher_hrnet48_coco_512x512-60fedcbc_20200712.pth"
