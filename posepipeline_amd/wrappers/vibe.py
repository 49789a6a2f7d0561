"""Drop-in for pose_pipeline/wrappers/vibe.py:11-74 `process_vibe` (SMPLMethodLookup row 0).

Same signature, table reads (`Video * PersonBbox`: video, bbox, present; `VideoInfo.height/width`) and return value: the `key` dict
it was given, with `cams` (n, 4), `verts` (n, 6890, 3), `poses` (n, 72), `betas` (n, 10), `joints3d` (n, 49, 3) and `joints2d`
(n, 49, 2) added, n = the number of PRESENT frames.  Kept reference behaviour:

  * Absent frames are skipped, not zero-filled (utils/bounding_box.py:122-128 `get_person_dataloader`).
  * Crop (`crop_image_bbox`, target_size (224, 224), dilate = scale = 1.0): the square box is fix_bb_aspect_ratio(bbox, ratio=1.0,
    dilate=1.0); its three corners (top-left, bottom-right, bottom-left) go through np.float32 into cv2.getAffineTransform, then
    cv2.warpAffine(INTER_LINEAR, border 0) on the RGB frame, ToTensor and the ImageNet Normalize: channel 0 of the tensor is R.  On the
    device: pp_warp_affine_normalize_each, one forward matrix per frame, solved on the host (`crop_matrices`).
  * The `bbox` the two convert_* helpers get is the stack of the SQUARED boxes.
  * Sequences: the DataLoader (batch 32, no shuffle) yields batches of at most 32 consecutive present frames and each batch is
    `unsqueeze(0)`d: ONE sequence of length <= 32 with a zero initial GRU state.  The last sequence is ragged; frames of different
    sequences never see each other's state.  Here several sequences ride in one pp_gru_forward call (its rows are independent) and
    the ragged one is padded with zero input behind its end, which no real frame reads.
  * cams = convert_crop_cam_to_orig_img(theta[:, :3], boxes, width, height); joints2d = convert_crop_coords_to_orig_img(boxes, kp_2d,
    224); poses = theta[:, 3:75] (axis-angle), betas = theta[:, 75:].

The network is models/vibe.py (backbone program, ops.Gru, head program) and models/smpl.py + csrc/smpl.hip (body model, joints,
projection, axis-angle).

Declared differences:
  * Checkpoints come through weights.get_state_dict and are never fetched: `vibe/spin_model_checkpoint.pth.tar` (dict key `model`;
    the backbone) and `vibe/vibe_model_w_3dpw.pth.tar` (dict key `gen_state_dict`; encoder and regressor -- its `regressor.*` override
    SPIN's, as load_state_dict(strict=False) does in the reference).  Without the files, POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded parameters.
  * The body model is `vibe/SMPL_NEUTRAL.npz` (models/smpl.py) instead of the chumpy pickle; synthetic under the same switch.
  * The video is read with open_video / FrameStreamer and is not deleted.  A read failure inside the present range raises RuntimeError
    (the reference: `assert ret`).
  * Zero present frames: ValueError naming the key (the reference: np.stack of an empty list).
  * UNPINNED (VIBE, SPIN and smplx are not in the reference tree), to check first with the checkpoints at hand: the key names; the 21
    vertex ids; JOINT_MAP; that fc1 and fc2 have no activation between them; the 1e-9 in the camera depth and the 1e-12 of
    F.normalize; the branch order of the quaternion conversion.
"""
from __future__ import annotations

import numpy as np

from .. import _lib, ops, weights
from ..models import smpl as smpl_data
from ..models import vibe as vm
from ..program import Net
from ..utils.bounding_box import convert_crop_cam_to_orig_img, convert_crop_coords_to_orig_img, fix_bb_aspect_ratio
from ..video import open_video

CROP_SIZE = 224
SPIN_CHECKPOINT = "vibe/spin_model_checkpoint.pth.tar"
VIBE_CHECKPOINT = "vibe/vibe_model_w_3dpw.pth.tar"
BACKBONE_BATCH = 32
MAX_SEQ = 2                      # sequences per pp_gru_forward call
CHAN_MAP = (2, 1, 0)             # decoded frames are BGR; tensor channel 0 is R


def get_affine_transform(src, dst) -> np.ndarray:
    """cv2.getAffineTransform on float32 point triples -> 2x3 float64: the 6x6 system in double"""
    a = np.zeros((6, 6), np.float64)
    b = np.zeros(6, np.float64)
    for i in range(3):
        a[2 * i, 0:3] = [src[i, 0], src[i, 1], 1.0]
        a[2 * i + 1, 3:6] = [src[i, 0], src[i, 1], 1.0]
        b[2 * i], b[2 * i + 1] = dst[i, 0], dst[i, 1]
    try:
        m = np.linalg.solve(a, b)
    except np.linalg.LinAlgError:
        m = np.zeros(6)
    return m.reshape(2, 3)


def crop_matrices(bboxes, crop_size=CROP_SIZE):
    """present boxes [n][4] TLWH -> (the squared boxes [n][4] float64, the forward warp matrices [n][2][3] float64)"""
    dst = np.float32([[0, 0], [crop_size, crop_size], [0, crop_size]])
    squared, mats = [], []
    for bbox in np.asarray(bboxes, np.float64).reshape(-1, 4):
        sq = fix_bb_aspect_ratio(bbox, ratio=1.0, dilate=1.0)
        src = np.float32([[sq[0], sq[1]], [sq[0] + sq[2], sq[1] + sq[3]], [sq[0], sq[1] + sq[3]]])
        squared.append(sq)
        mats.append(get_affine_transform(src, dst))
    return np.stack(squared, axis=0), np.stack(mats, axis=0)


def load_state_dicts(seed=7):
    spin = weights.get_state_dict(SPIN_CHECKPOINT, vm.spin_param_shapes(), seed=seed)
    vibe = weights.get_state_dict(VIBE_CHECKPOINT, vm.vibe_param_shapes(), seed=seed + 1, synth=vm.synth_params)
    return spin, vibe


class VibeModel:
    """The resident model on one context: backbone program, GRU, head program, body model, and the device buffers between them."""

    def __init__(self, device=0, numerics=None, ctx=None, spin_sd=None, vibe_sd=None, body=None, backbone=True):
        if vibe_sd is None or (backbone and spin_sd is None):
            loaded = load_state_dicts()
            spin_sd, vibe_sd = (loaded[0] if spin_sd is None else spin_sd), (loaded[1] if vibe_sd is None else vibe_sd)
        body = smpl_data.load_body_model() if body is None else smpl_data.check_body_model(body)
        self._own_ctx = ctx is None
        self.ctx = ctx = _lib.Context(device) if ctx is None else ctx
        self.n_verts = body["v_template"].shape[0]
        self.rows = MAX_SEQ * vm.SEQ
        self.backbone = Net(ctx, vm.build_backbone_program(spin_sd), max_batch=BACKBONE_BATCH, numerics=numerics) if backbone else None
        self.gru = ops.Gru(ctx, vm.gru_layers(vm.checked(vibe_sd, vm.vibe_param_shapes(), "VIBE generator")))
        self.head = Net(ctx, vm.build_head_program(vibe_sd), max_batch=self.rows, numerics=numerics)
        for name, arr in vm.init_inputs(vibe_sd, self.rows).items():
            ctx.h2d(self.head.buffer(name)[0], arr)
        self.smpl = ops.SmplModel(ctx, body, smpl_data.vertex_ids(self.n_verts), smpl_data.JOINT_MAP_54)
        self.lut = ops.normalize_lut(vm.MEAN, vm.STD)
        r = self.rows
        self._sizes = dict(h=r * vm.HIDDEN, rot=r * 216, betas=r * 10, cam=r * 3, verts=r * self.n_verts * 3, j3=r * 147, k2=r * 98, aa=r * 72)
        self._dev = {k: ctx.malloc(n * 4) for k, n in self._sizes.items()}
        self.stage_ms = None

    # ---- features: crop + backbone ---------------------------------------------------------------------------------------------
    def encode_frames(self, frames_dev: int, shape, frame_idx, mats, feat_dev: int):
        """frames_dev [F][H][W][3] u8 BGR on the device; crops frame_idx[i] with mats[i] and writes features [len][2048] at feat_dev"""
        in_ptr = self.backbone.buffer("input")[0]
        out_ptr = self.backbone.buffer("features")[0]
        for i0 in range(0, len(frame_idx), BACKBONE_BATCH):
            k = min(BACKBONE_BATCH, len(frame_idx) - i0)
            ops.warp_affine_normalize_each(self.ctx, frames_dev, frame_idx[i0:i0 + k], mats[i0:i0 + k], (CROP_SIZE, CROP_SIZE), self.lut,
                                           CHAN_MAP, out_dev=in_ptr, frames_dev_shape=shape)
            self.backbone.run(k)
            self.ctx.d2d(feat_dev + i0 * vm.FEAT * 4, out_ptr, k * vm.FEAT * 4)
        self.ctx.synchronize()

    # ---- encoder + regressor + body model on features ------------------------------------------------------------------------------
    def run_head(self, feat_dev: int, n: int, want_verts=True, timed=False) -> dict:
        """feat_dev: device features [ceil(n / 32) * 32][2048], rows >= n zeros.  -> dict(cam [n][3], pose_aa [n][72], betas [n][10],
        verts [n][V][3] or None, joints3d [n][49][3], kp2d [n][49][2]).  timed: device milliseconds (GRU, regressor, SMPL) in stage_ms."""
        ctx, lib, d = self.ctx, self.ctx.lib, self._dev
        P = _lib.ptr
        out = dict(cam=np.empty((n, 3), np.float32), pose_aa=np.empty((n, 72), np.float32), betas=np.empty((n, 10), np.float32),
                   verts=np.empty((n, self.n_verts, 3), np.float32) if want_verts else None,
                   joints3d=np.empty((n, 49, 3), np.float32), kp2d=np.empty((n, 49, 2), np.float32))
        ms = np.zeros(3, np.float64)

        def stage(k, fn):
            if timed:
                ctx.timer_start()
            fn()
            if timed:
                ms[k] += ctx.timer_stop()

        h_in, f_in = self.head.buffer("h")[0], self.head.buffer("features")[0]
        pose6d, (shape_p, _, (_, _, shape_c)), (cam_p, _, (_, _, cam_c)) = self.head.buffer("pose6d")[0], self.head.buffer("shape"), self.head.buffer("cam")
        n_seq = -(-n // vm.SEQ)
        for s0 in range(0, n_seq, MAX_SEQ):
            b = min(MAX_SEQ, n_seq - s0)
            rows, r0 = b * vm.SEQ, s0 * vm.SEQ
            m = min(rows, n - r0)
            x_dev = feat_dev + r0 * vm.FEAT * 4
            stage(0, lambda: self.gru.forward_dev(x_dev, b, vm.SEQ, d["h"]))

            def regress():
                ctx.d2d(h_in, d["h"], rows * vm.HIDDEN * 4)
                ctx.d2d(f_in, x_dev, rows * vm.FEAT * 4)
                self.head.run(rows)
                _lib.check(lib.pp_vibe_head_unpack(ctx.handle, P(pose6d), P(shape_p), shape_c, P(cam_p), cam_c, rows, P(d["rot"]), P(d["betas"]),
                                                   P(d["cam"])), "pp_vibe_head_unpack")
            stage(1, regress)
            stage(2, lambda: _lib.check(lib.pp_smpl_forward(ctx.handle, self.smpl.handle, P(d["betas"]), P(d["rot"]), P(d["cam"]), m, P(d["verts"]),
                                                            P(d["j3"]), P(d["k2"]), P(d["aa"]), _lib.PP_MEM_DEVICE), "pp_smpl_forward"))
            for name, key in (("cam", "cam"), ("pose_aa", "aa"), ("betas", "betas"), ("joints3d", "j3"), ("kp2d", "k2"), ("verts", "verts")):
                if out[name] is not None:
                    ctx.d2h(out[name][r0:r0 + m], d[key])         # synchronous: the device arrays are free for the next chunk
        self.stage_ms = ms if timed else None
        return out

    def close(self):
        for p in getattr(self, "_dev", {}).values():
            self.ctx.free(p)
        self._dev = {}
        for part in ("smpl", "gru", "head", "backbone"):
            obj = getattr(self, part, None)
            if obj is not None:
                obj.close()
                setattr(self, part, None)
        if self._own_ctx and getattr(self, "ctx", None) is not None:
            self.ctx.close()
            self.ctx = None


_cache: dict = {}


def _model(device=0):
    if device not in _cache:
        _cache[device] = VibeModel(device)
    return _cache[device]


def process_vibe(key):
    from ..pipeline import PersonBbox, Video, VideoInfo
    from ..streaming import FrameStreamer

    crop_size = CROP_SIZE
    bboxes_dj, present_dj = (PersonBbox & key).fetch1("bbox", "present")
    video = Video.get_robust_reader(key, return_cap=False)
    present = np.asarray(present_dj).astype(bool)
    frame_ids = np.flatnonzero(present)
    n = len(frame_ids)
    if n == 0:
        raise ValueError(f"process_vibe: the person of {key} is present in no frame")
    bbox, mats = crop_matrices(np.asarray(bboxes_dj, np.float64)[frame_ids], crop_size)

    model = _model()
    ctx = model.ctx
    padded = -(-n // vm.SEQ) * vm.SEQ
    feat_dev = ctx.malloc(padded * vm.FEAT * 4)
    try:
        if padded > n:
            ctx.h2d(feat_dev + n * vm.FEAT * 4, np.zeros((padded - n, vm.FEAT), np.float32))
        last = int(frame_ids[-1]) + 1
        cap = open_video(video)
        streamer = FrameStreamer(ctx, cap, min(BACKBONE_BATCH, last), max_frames=last)
        done = 0
        try:
            for dev_ptr, m, first in streamer:
                lo, hi = np.searchsorted(frame_ids, [first, first + m])
                if hi > lo:
                    model.encode_frames(dev_ptr, (m, streamer.h, streamer.w), frame_ids[lo:hi] - first, mats[lo:hi], feat_dev + int(lo) * vm.FEAT * 4)
                streamer.release()
                done = first + m
        finally:
            streamer.close()
            cap.release()
        if done < last:
            raise RuntimeError(f"process_vibe: the video of {key} ended at frame {done}, the person is present up to frame {last - 1}")
        res = model.run_head(feat_dev, n)
    finally:
        ctx.free(feat_dev)

    key["cams"] = res["cam"]
    key["verts"] = res["verts"]
    key["poses"] = res["pose_aa"]
    key["betas"] = res["betas"]
    key["joints3d"] = res["joints3d"]
    key["joints2d"] = res["kp2d"]

    height, width = (VideoInfo & key).fetch1("height", "width")
    key["cams"] = convert_crop_cam_to_orig_img(key["cams"], bbox, width, height)
    key["joints2d"] = convert_crop_coords_to_orig_img(bbox, key["joints2d"], crop_size)
    return key
