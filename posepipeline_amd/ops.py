"""Thin Python wrappers over the stage entry points of the C ABI (host-numpy or device-pointer arguments)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

# torchvision to_tensor + normalize constants of the top-down test pipeline
# (3rdparty/mmpose/config/top_down/darkpose/coco/hrnet_w48_coco_384x288_dark.py:132-136)
TOPDOWN_MEAN = (0.485, 0.456, 0.406)
TOPDOWN_STD = (0.229, 0.224, 0.225)


def normalize_lut(mean=TOPDOWN_MEAN, std=TOPDOWN_STD) -> np.ndarray:
    """[3][256] fp32 table of ((v/255) - mean[c]) / std[c], each step rounded to float32."""
    v = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    m = np.asarray(mean, np.float32)[:, None]
    s = np.asarray(std, np.float32)[:, None]
    return np.ascontiguousarray(((v[None, :] - m).astype(np.float32) / s).astype(np.float32))


def crop_affine_normalize(ctx: L.Context, frames: np.ndarray, frame_idx, bboxes, out_wh=(288, 384), lut=None,
                          chan_map=(0, 1, 2), flip=True, want_crop_u8=False, udp=False):
    """frames [F][H][W][3] u8; bboxes [P][4] float64 TLWH (NaN row = absent).
    udp: TopDownAffine(use_udp=True) transform (ViTPose configs) instead of the 3-point affine.
    Returns dict(out=[P or 2P][out_h][out_w][4] fp32, center_scale=[P][4], valid=[P], crop_u8=...)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    f, h, w, c = frames.shape
    assert c == 3
    bboxes = np.ascontiguousarray(bboxes, dtype=np.float64).reshape(-1, 4)
    p = bboxes.shape[0]
    frame_idx = np.ascontiguousarray(frame_idx, dtype=np.int32)
    assert frame_idx.shape == (p,)
    lut = normalize_lut() if lut is None else np.ascontiguousarray(lut, np.float32)
    cm = np.asarray(chan_map, dtype=np.int32)
    ow, oh = out_wh
    out = np.empty((p * (2 if flip else 1), oh, ow, 4), dtype=np.float32)
    cs = np.zeros((p, 4), dtype=np.float32)
    valid = np.zeros((p,), dtype=np.int32)
    crop = np.empty((p, oh, ow, 3), dtype=np.uint8) if want_crop_u8 else None
    L.check(ctx.lib.pp_crop_affine_normalize(ctx.handle, L.ptr(frames), f, h, w, L.ptr(frame_idx), L.ptr(bboxes), p, ow, oh,
                                             L.ptr(lut), L.ptr(cm), int(bool(flip)) | (2 if udp else 0), L.ptr(out), L.ptr(cs), L.ptr(crop),
                                             L.ptr(valid), L.PP_MEM_HOST), "pp_crop_affine_normalize")
    return dict(out=out, center_scale=cs, valid=valid, crop_u8=crop)


def flip_merge_decode(ctx: L.Context, hm: np.ndarray, hm_flip, center_scale, flip_perm=None, shift_heatmap=True,
                      post="unbiased", blur_kernel=17, want_merged=False):
    """hm, hm_flip [N][K][H][W] fp32 (host).  Returns (kpts [N][K][3], merged or None)."""
    hm = np.ascontiguousarray(hm, np.float32)
    n, k, h, w = hm.shape
    hf = None if hm_flip is None else np.ascontiguousarray(hm_flip, np.float32)
    perm = None if flip_perm is None else np.ascontiguousarray(flip_perm, np.int32)
    cs = np.ascontiguousarray(center_scale, np.float32).reshape(n, 4)
    kp = np.empty((n, k, 3), dtype=np.float32)
    merged = np.empty_like(hm) if want_merged else None
    post_i = {"unbiased": 1, "default": 0, "udp": 2, None: -1}[post]   # "udp": UDP crop + DARK-UDP decode (ViTPose)
    L.check(ctx.lib.pp_flip_merge_decode(ctx.handle, L.ptr(hm), L.ptr(hf), n, k, h, w, L.ptr(perm), int(shift_heatmap),
                                         post_i, int(blur_kernel), L.ptr(cs), L.ptr(kp), L.ptr(merged), L.PP_MEM_HOST),
            "pp_flip_merge_decode")
    return kp, merged


def nms(ctx: L.Context, boxes, scores, thr, convention=0):
    """convention 0: float32 x1y1x2y2 (mmcv); 1: float64 tlwh (deep_sort); 2: float32 y1x1y2x2 (TensorFlow).
    Returns kept indices (int64)."""
    dt = np.float64 if convention == 1 else np.float32
    boxes = np.ascontiguousarray(boxes, dt).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, dt).reshape(-1)
    n = boxes.shape[0]
    keep = np.zeros(max(n, 1), np.int32)
    k = C.c_int32()
    L.check(ctx.lib.pp_nms(ctx.handle, L.ptr(boxes), L.ptr(scores), n, float(thr), convention, L.ptr(keep), C.byref(k),
                           L.PP_MEM_HOST), "pp_nms")
    return keep[: k.value].astype(np.int64)


class TopDown:
    """pp_topdown handle: crop/normalise -> backbone -> flip-merge + decode, parameters resident."""

    def __init__(self, net, num_joints=17, flip_perm=None, shift_heatmap=True, post="unbiased", blur_kernel=17,
                 lut=None, chan_map=(0, 1, 2), in_name="input", out_name="output"):
        self.net = net
        self.ctx = net.ctx
        self.k = int(num_joints)
        lut = normalize_lut() if lut is None else np.ascontiguousarray(lut, np.float32)
        cm = np.asarray(chan_map, np.int32)
        perm = None if flip_perm is None else np.ascontiguousarray(flip_perm, np.int32)
        post_i = {"unbiased": 1, "default": 0, "udp": 2, None: -1}[post]   # "udp": UDP crop + DARK-UDP decode (ViTPose)
        h = C.c_void_p()
        L.check(self.ctx.lib.pp_topdown_create(net.handle, net.prog.named[in_name], net.prog.named[out_name], self.k,
                                               L.ptr(perm), int(shift_heatmap), post_i, int(blur_kernel), L.ptr(lut),
                                               L.ptr(cm), C.byref(h)), "pp_topdown_create")
        self.handle = h
        self.flip = perm is not None

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None) and getattr(self.net, "handle", None):
                self.ctx.lib.pp_topdown_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, frames, frame_idx, bboxes, frames_dev_shape=None):
        """frames: numpy [F][H][W][3] u8, or a device pointer (int) with frames_dev_shape=(F,H,W).
        Returns (kpts [P][K][3] fp32, valid [P] int32)."""
        bboxes = np.ascontiguousarray(bboxes, np.float64).reshape(-1, 4)
        p = bboxes.shape[0]
        frame_idx = np.ascontiguousarray(frame_idx, np.int32)
        if isinstance(frames, np.ndarray):
            frames = np.ascontiguousarray(frames, np.uint8)
            f, h, w, _ = frames.shape
            fmem = L.PP_MEM_HOST
        else:
            f, h, w = frames_dev_shape
            fmem = L.PP_MEM_DEVICE
        kp = np.empty((p, self.k, 3), np.float32)
        valid = np.zeros((p,), np.int32)
        L.check(self.ctx.lib.pp_topdown_run(self.handle, L.ptr(frames), f, h, w, fmem, L.ptr(frame_idx), L.ptr(bboxes), p,
                                            L.ptr(kp), L.PP_MEM_HOST, L.ptr(valid)), "pp_topdown_run")
        return kp, valid

    def run_precropped(self, x, center_scale, n=None):
        """x: numpy [N][H][W][4] fp32 or device pointer (int, with n given).  Returns kpts [N][K][3]."""
        if isinstance(x, np.ndarray):
            x = np.ascontiguousarray(x, np.float32)
            n = x.shape[0]
            xmem = L.PP_MEM_HOST
        else:
            xmem = L.PP_MEM_DEVICE
        cs = np.ascontiguousarray(center_scale, np.float32).reshape(n, 4)
        kp = np.empty((n, self.k, 3), np.float32)
        L.check(self.ctx.lib.pp_topdown_run_precropped(self.handle, L.ptr(x), xmem, L.ptr(cs), n, L.ptr(kp),
                                                       L.PP_MEM_HOST), "pp_topdown_run_precropped")
        return kp

    def timing(self):
        """HIP-event stage times of the last run, ms: (pre, backbone, decode)."""
        ms = np.zeros(3, np.float32)
        L.check(self.ctx.lib.pp_topdown_timing(self.handle, L.ptr(ms)), "pp_topdown_timing")
        return tuple(float(v) for v in ms)


def gray_from_nhwc4(ctx: L.Context, src_dev: int, n: int, h: int, w: int, gray_dev: int, rgb=(0, 1, 2)):
    """cv2.COLOR_RGB2GRAY of a device [n][h][w][4] float32 tensor into device [n][h][w] (queued on the ctx stream)"""
    L.check(ctx.lib.pp_gray_from_nhwc4(ctx.handle, C.c_void_p(src_dev), n, h, w, rgb[0], rgb[1], rgb[2], C.c_void_p(gray_dev)),
            "pp_gray_from_nhwc4")


def ecc_euclidean(ctx: L.Context, gray_dev: int, n_images: int, h: int, w: int, pairs, num_iters=100, stop_eps=1e-5):
    """cv2.findTransformECC(MOTION_EUCLIDEAN) of every (template image, input image) pair of device [n_images][h][w] float32 gray
    images in one call (csrc/ecc.hip) -> (warp [n_pairs][2][3] float64, rho [n_pairs], iterations [n_pairs], status [n_pairs] PP_ECC_*)"""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    k = len(pairs)
    warp, rho = np.zeros((k, 2, 3), np.float64), np.zeros(k, np.float64)
    iters, status = np.zeros(k, np.int32), np.zeros(k, np.int32)
    L.check(ctx.lib.pp_ecc_euclidean(ctx.handle, C.c_void_p(gray_dev), n_images, h, w, L.ptr(pairs), k, int(num_iters), float(stop_eps),
                                     L.ptr(warp), L.ptr(rho), L.ptr(iters), L.ptr(status)), "pp_ecc_euclidean")
    return warp, rho, iters, status


def fairmot_input_size(src_h: int, src_w: int):
    """-> (hp, wp, nh, nw, top, left): FairMOT's network size for a source of this orientation and the letterbox of the 1920 x 1080
    image every frame is resized to first (pp_fairmot_input_size)"""
    v = [C.c_int32() for _ in range(6)]
    L.check(L.load_library().pp_fairmot_input_size(int(src_h), int(src_w), *[C.byref(x) for x in v]), "pp_fairmot_input_size")
    return tuple(int(x.value) for x in v)


def fairmot_preprocess(ctx: L.Context, frames, out_dev: int, frames_dev_shape=None):
    """frames: numpy [n][h][w][3] u8 BGR, or a device pointer (int) with frames_dev_shape = (n, h, w) -> device [n][hp][wp][4]
    float32 RGB / 255 at out_dev (pp_fairmot_preprocess).  Returns the geometry of fairmot_input_size."""
    if isinstance(frames, np.ndarray):
        frames = np.ascontiguousarray(frames, np.uint8)
        n, h, w, _ = frames.shape
        mem = L.PP_MEM_HOST
    else:
        n, h, w = frames_dev_shape
        mem = L.PP_MEM_DEVICE
    geo = fairmot_input_size(h, w)
    hp, wp, nh, nw, top, left = geo
    L.check(ctx.lib.pp_fairmot_preprocess(ctx.handle, L.ptr(frames), n, h, w, mem, hp, wp, nh, nw, top, left, C.c_void_p(out_dev)),
            "pp_fairmot_preprocess")
    return geo


def fairmot_decode(ctx: L.Context, hm_dev: int, wh_dev: int, reg_dev: int, id_dev: int, n: int, h: int, w: int, K: int, id_dim: int = 128):
    """pp_fairmot_decode on device head maps (NHWC) -> (dets [n][K][5] float32, feats [n][K][id_dim] float32, inds [n][K] int32)"""
    dets = np.zeros((n, K, 5), np.float32)
    feats = np.zeros((n, K, id_dim), np.float32)
    inds = np.zeros((n, K), np.int32)
    L.check(ctx.lib.pp_fairmot_decode(ctx.handle, C.c_void_p(hm_dev), C.c_void_p(wh_dev), C.c_void_p(reg_dev), C.c_void_p(id_dev), n, h, w,
                                      K, id_dim, L.ptr(dets), L.ptr(feats), L.ptr(inds), L.PP_MEM_HOST), "pp_fairmot_decode")
    return dets, feats, inds


# ---- TraDeS (trades.hip, fairmot.hip) ------------------------------------------------------------------------------------------------
def trades_cva(ctx: L.Context, emb_cur, emb_prev, want_soft=False):
    """pp_trades_cva on host arrays: emb_cur, emb_prev [n][hc][wc][128] float32 -> (tracking_offset [n][2 hc][2 wc][2] with channel 0 =
    off_w and 1 = off_h, soft_h [n][P][hc] or None, soft_w [n][P][wc] or None)"""
    emb_cur, emb_prev = (np.ascontiguousarray(e, np.float32) for e in (emb_cur, emb_prev))
    n, hc, wc, dim = emb_cur.shape
    assert emb_prev.shape == emb_cur.shape
    off = np.empty((n, 2 * hc, 2 * wc, 2), np.float32)
    sh = np.empty((n, hc * wc, hc), np.float32) if want_soft else None
    sw = np.empty((n, hc * wc, wc), np.float32) if want_soft else None
    L.check(ctx.lib.pp_trades_cva(ctx.handle, L.ptr(emb_cur), L.ptr(emb_prev), n, hc, wc, dim, L.ptr(off), L.ptr(sh), L.ptr(sw), L.PP_MEM_HOST),
            "pp_trades_cva")
    return off, sh, sw


def trades_cva_dev(ctx: L.Context, cur_dev: int, prev_dev: int, n: int, hc: int, wc: int, off_dev: int, dim: int = 128):
    """pp_trades_cva on device pointers; queued on the context's stream"""
    L.check(ctx.lib.pp_trades_cva(ctx.handle, C.c_void_p(cur_dev), C.c_void_p(prev_dev), n, hc, wc, dim, C.c_void_p(off_dev), None, None,
                                  L.PP_MEM_DEVICE), "pp_trades_cva")


def trades_render_prehm(ctx: L.Context, boxes, hp: int, wp: int, out_dev=None):
    """pp_trades_render_prehm: boxes int [m][3] = (cx, cy, radius) in network-input pixels -> the pooled map [hp / 4][wp / 4] float32 (numpy),
    or written to the device address out_dev (returns None)"""
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 3)
    if out_dev is not None:
        L.check(ctx.lib.pp_trades_render_prehm(ctx.handle, L.ptr(boxes) if len(boxes) else None, len(boxes), hp, wp, C.c_void_p(int(out_dev)),
                                               L.PP_MEM_DEVICE), "pp_trades_render_prehm")
        return None
    out = np.empty((hp // 4, wp // 4), np.float32)
    L.check(ctx.lib.pp_trades_render_prehm(ctx.handle, L.ptr(boxes) if len(boxes) else None, len(boxes), hp, wp, L.ptr(out), L.PP_MEM_HOST),
            "pp_trades_render_prehm")
    return out


def trades_decode(ctx: L.Context, hm_dev: int, reg_dev: int, ltrb_dev: int, trk_dev: int, n: int, h: int, w: int, K: int):
    """pp_trades_decode on device head maps (NHWC) -> (dets [n][K][9] float32 = ct 2, bbox 4, tracking 2, score; inds [n][K] int32)"""
    dets = np.zeros((n, K, 9), np.float32)
    inds = np.zeros((n, K), np.int32)
    L.check(ctx.lib.pp_trades_decode(ctx.handle, C.c_void_p(hm_dev), C.c_void_p(reg_dev), C.c_void_p(ltrb_dev), C.c_void_p(trk_dev), n, h, w, K,
                                     L.ptr(dets), L.ptr(inds), L.PP_MEM_HOST), "pp_trades_decode")
    return dets, inds


# ---- SMPL stage: VIBE (crop_affine.hip, gru.hip, smpl.hip) ---------------------------------------------------------------------------
def warp_affine_normalize_each(ctx: L.Context, frames, frame_idx, matrices, out_wh=(224, 224), lut=None, chan_map=(0, 1, 2),
                               want_crop_u8=False, out_dev=None, frames_dev_shape=None):
    """cv2.warpAffine(frames[frame_idx[i]], matrices[i], out_wh, INTER_LINEAR) + the normalisation table, per sample
    (pp_warp_affine_normalize_each).  frames: numpy [F][H][W][3] u8 -> dict(out [n][oh][ow][4] float32, crop_u8); or a device pointer
    with frames_dev_shape = (F, H, W) and out_dev = the device address of the output (returns None; the call is synchronised)."""
    frame_idx = np.ascontiguousarray(frame_idx, dtype=np.int32)
    n = frame_idx.shape[0]
    matrices = np.ascontiguousarray(matrices, dtype=np.float64).reshape(n, 6)
    lut = normalize_lut() if lut is None else np.ascontiguousarray(lut, np.float32)
    cm = np.asarray(chan_map, dtype=np.int32)
    ow, oh = out_wh
    if isinstance(frames, np.ndarray):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        f, h, w, c = frames.shape
        assert c == 3
        out = np.empty((n, oh, ow, 4), np.float32)
        crop = np.empty((n, oh, ow, 3), np.uint8) if want_crop_u8 else None
        L.check(ctx.lib.pp_warp_affine_normalize_each(ctx.handle, L.ptr(frames), f, h, w, L.ptr(frame_idx), L.ptr(matrices), n, ow, oh,
                                                      L.ptr(lut), L.ptr(cm), L.ptr(out), L.ptr(crop), L.PP_MEM_HOST), "pp_warp_affine_normalize_each")
        return dict(out=out, crop_u8=crop)
    f, h, w = frames_dev_shape
    L.check(ctx.lib.pp_warp_affine_normalize_each(ctx.handle, C.c_void_p(int(frames)), f, h, w, L.ptr(frame_idx), L.ptr(matrices), n, ow, oh,
                                                  L.ptr(lut), L.ptr(cm), C.c_void_p(int(out_dev)), None, L.PP_MEM_DEVICE), "pp_warp_affine_normalize_each")
    return None


def gru_param_blob(layers_params) -> np.ndarray:
    """[(W_ih [3H][in_l], W_hh [3H][H], b_ih [3H], b_hh [3H]), ...] per layer (nn.GRU's weight_ih_l{k} ... in its own order) -> the
    flat float32 blob pp_gru_forward reads"""
    return np.concatenate([np.asarray(a, np.float32).reshape(-1) for layer in layers_params for a in layer])


class Gru:
    """nn.GRU(in, hidden, layers) with its parameters resident on the device (pp_gru_forward)"""

    def __init__(self, ctx: L.Context, layers_params):
        self.ctx = ctx
        self.layers = len(layers_params)
        self.hidden = int(np.shape(layers_params[0][1])[1])
        self.inp = int(np.shape(layers_params[0][0])[1])
        blob = gru_param_blob(layers_params)
        assert blob.size == ctx.lib.pp_gru_param_floats(self.inp, self.hidden, self.layers), blob.size
        self.params = ctx.malloc(blob.nbytes)
        ctx.h2d(self.params, blob)

    def forward(self, x) -> np.ndarray:
        """x [B][T][in] numpy -> y [B][T][hidden]"""
        x = np.ascontiguousarray(x, np.float32)
        b, t, i = x.shape
        assert i == self.inp
        y = np.empty((b, t, self.hidden), np.float32)
        L.check(self.ctx.lib.pp_gru_forward(self.ctx.handle, L.ptr(x), b, t, i, self.hidden, self.layers, C.c_void_p(self.params), L.ptr(y),
                                            L.PP_MEM_HOST), "pp_gru_forward")
        return y

    def forward_dev(self, x_dev: int, b: int, t: int, y_dev: int):
        """device x [b][t][in] -> device y [b][t][hidden]; queued on the context's stream"""
        L.check(self.ctx.lib.pp_gru_forward(self.ctx.handle, C.c_void_p(x_dev), b, t, self.inp, self.hidden, self.layers,
                                            C.c_void_p(self.params), C.c_void_p(y_dev), L.PP_MEM_DEVICE), "pp_gru_forward")

    def close(self):
        if getattr(self, "params", None) and getattr(self.ctx, "handle", None):
            self.ctx.free(self.params)
        self.params = None


class SmplModel:
    """the SMPL body model resident on the device (pp_smpl_model_create / pp_smpl_forward); `body`: the arrays of models/smpl.py"""

    def __init__(self, ctx: L.Context, body: dict, vertex_ids, joint_map):
        self.ctx = ctx
        f32 = lambda k: np.ascontiguousarray(body[k], np.float32)                 # noqa: E731
        self.n_verts = int(body["v_template"].shape[0])
        ids, jm = np.ascontiguousarray(vertex_ids, np.int32), np.ascontiguousarray(joint_map, np.int32)
        assert ids.shape == (21,) and jm.shape == (49,)
        h = C.c_void_p()
        L.check(ctx.lib.pp_smpl_model_create(ctx.handle, L.ptr(f32("v_template")), L.ptr(f32("shapedirs")), L.ptr(f32("posedirs")),
                                             L.ptr(f32("J_regressor")), L.ptr(f32("weights")), L.ptr(f32("J_regressor_extra")), self.n_verts,
                                             L.ptr(ids), L.ptr(jm), C.byref(h)), "pp_smpl_model_create")
        self.handle = h

    def forward(self, betas, rotmat, cam, want_verts=True) -> dict:
        """betas [F][10], rotmat [F][24][3][3], cam [F][3] numpy -> dict(verts [F][V][3] or None, joints3d [F][49][3], kp2d [F][49][2],
        pose_aa [F][72])"""
        betas, rotmat, cam = (np.ascontiguousarray(a, np.float32) for a in (betas, rotmat, cam))
        f = betas.shape[0]
        assert betas.shape == (f, 10) and rotmat.size == f * 216 and cam.shape == (f, 3)
        verts = np.empty((f, self.n_verts, 3), np.float32) if want_verts else None
        j3, k2, aa = np.empty((f, 49, 3), np.float32), np.empty((f, 49, 2), np.float32), np.empty((f, 72), np.float32)
        L.check(self.ctx.lib.pp_smpl_forward(self.ctx.handle, self.handle, L.ptr(betas), L.ptr(rotmat), L.ptr(cam), f, L.ptr(verts), L.ptr(j3),
                                             L.ptr(k2), L.ptr(aa), L.PP_MEM_HOST), "pp_smpl_forward")
        return dict(verts=verts, joints3d=j3, kp2d=k2, pose_aa=aa)

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.pp_smpl_model_destroy(self.handle)
            self.handle = None
