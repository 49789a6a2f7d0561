"""Drop-in for pose_pipeline/wrappers/gastnet_lifting.py:9-78 `process_gastnet` (LiftingMethodLookup row 0, the default of
`lifting_pipeline`).

Same signature, table reads (`TopDownPerson.keypoints`, `VideoInfo.height/width`) and return value: `{"keypoints_3d": (N, 17, 3)
float64, "keypoints_valid": [bool] * N}`, zeros at the invalid frames.  The reference imports GAST-Net's own `tools.preprocess` and
`tools.inference`, which are not in its tree; the host side is restated here from what it computes:

  h36m_coco_format   coordinates: poseformer.coco_h36m (the same landmark rules); scores: copied across the 13 shared joints, then
                     pelvis = mean(hips), thorax = mean(shoulders), spine = mean(new pelvis, new thorax), head = mean(eyes and ears);
                     valid frames: those whose 34 converted coordinates do not sum to 0
  revise_kpts        on the valid frames, the leg joints among [2, 3, 5, 6] with score < 0.3 are replaced by the joint above them
  normalize_screen_coordinates   X / w * 2 - [1, h / w]
  gen_pose           valid frames compacted, `pad` frames replicated on both sides, flip test-time augmentation (second sample: x negated
                     and left / right joints swapped; its output x negated and the swap undone; the two averaged in float32), then
                     camera_to_world with the fixed quaternion, t = 0

The network is models/gastnet.py on a resident Net with max_batch = 2 (the clip and its mirror image), run over chunks of
`spec.chunk` output frames with `pad`-frame halos.  `process_gastnet` and the streamed cascade go through
`GastNetLifter.lift_many` (pp_gastnet_lift_many, csrc/gastnet.hip): the windows, the mirror images, the flip merge and the camera
rotation of every track of a call are device kernels, with one upload and one download per call.  `GastNetLifter.lift` /
`lift_chunks` / `camera_to_world` are the same arithmetic on the host, chunk by chunk: the reference `lift_many` is tested against.

Declared differences:
  * A clip with no valid frame: ValueError (the reference: an AssertionError inside gen_pose).
  * Other than 17 joints: ValueError.
  * The checkpoint is `gastnet/27_frame_model.bin` under MODEL_DATA_DIR (as the reference), `checkpoint["model_pos"]` with the
    `module.` prefix of nn.DataParallel dropped; a missing key is a KeyError, another shape a ValueError.  It is never fetched;
    POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded parameters.  GAST_PATH is not read.
  * The video is not touched.
  * UNPINNED (model/gast_net.py, tools/preprocess.py and tools/inference.py are not in the reference tree), to check first with the
    checkpoint at hand: the presence of init_bn; the width of expand_conv; the adj_con rule (an `e` of another width fails with a
    message that names the mask and both counts); the naming and bias of theta / phi / g; any learned additive term in the joint
    attention; flip augmentation in gen_pose (and whether gen_pose moves z so that its minimum is 0: not done here).
"""
from __future__ import annotations

import os
import time

import numpy as np

from .. import _lib, weights
from ..models import gastnet as gn
from ..program import Net
from .poseformer import _H36M_FROM_COCO, coco_h36m

NUM_JOINTS = 17
CHECKPOINT = "gastnet/27_frame_model.bin"
JOINTS_LEFT, JOINTS_RIGHT = list(gn.H36M_LEFT), list(gn.H36M_RIGHT)
SCORE_THRESHOLD = 0.3
# rotation of the camera the models were trained with (GAST-Net's gen_pose), (w, x, y, z)
CAMERA_QUATERNION = np.array([0.14070565, -0.15007018, -0.7552408, 0.62232804], np.float32)

_MIRROR = np.arange(NUM_JOINTS)
_MIRROR[JOINTS_LEFT + JOINTS_RIGHT] = JOINTS_RIGHT + JOINTS_LEFT


def checkpoint_path() -> str:
    return os.path.join(weights.model_data_dir(), CHECKPOINT)


# ---- host side -------------------------------------------------------------------------------------------------------------------
def h36m_coco_format(keypoints, scores):
    """(N, 17, 2) COCO key points, (N, 17) scores -> ((N, 17, 2) float32 H36M key points, (N, 17) float32 scores, valid frame indices).
    Frames whose COCO coordinates sum to 0 (no detection) stay all-zero, as in GAST-Net's tool."""
    kp = np.asarray(keypoints)
    sc = np.asarray(scores)
    if kp.ndim != 3 or kp.shape[1] != NUM_JOINTS or kp.shape[2] != 2 or sc.shape != kp.shape[:2]:
        raise ValueError(f"h36m_coco_format: key points {kp.shape} / scores {sc.shape}, expected (N, {NUM_JOINTS}, 2) / (N, {NUM_JOINTS})")
    out = np.zeros(kp.shape, np.float32)
    out_s = np.zeros(sc.shape, np.float32)
    if kp.sum() != 0.0:
        out, out_s = h36m_rows(kp, sc)
    valid = np.where(out.reshape(-1, 2 * NUM_JOINTS).sum(axis=1) != 0)[0]
    return out, out_s, valid


def h36m_rows(kp, sc):
    """The conversion of h36m_coco_format without its clip-wide guard: every frame's result depends on that frame alone (what a
    stream, which never sees the whole clip, applies frame by frame).  -> ((N, 17, 2) float32, (N, 17) float32)"""
    out = coco_h36m(kp)
    out_s = np.zeros(sc.shape, np.float32)
    sc = sc.astype(np.float32)
    out_s[:, 9] = sc[:, 0]                                        # nose
    for h, c in _H36M_FROM_COCO.items():
        out_s[:, h] = sc[:, c]
    out_s[:, 0] = (sc[:, 11] + sc[:, 12]) / np.float32(2)
    out_s[:, 8] = (sc[:, 5] + sc[:, 6]) / np.float32(2)
    out_s[:, 7] = (out_s[:, 0] + out_s[:, 8]) / np.float32(2)
    out_s[:, 10] = (((sc[:, 1] + sc[:, 2]) + sc[:, 3]) + sc[:, 4]) / np.float32(4)
    return out, out_s


# the low-score sets among [2, 3, 5, 6] (right knee, right foot, left knee, left foot) that are repaired: set -> (targets, sources)
_REVISE = {(2, 3, 5, 6): ([2, 3, 5, 6], [1, 1, 4, 4]), (2, 3, 6): ([2, 3, 6], [1, 1, 5]), (3, 5, 6): ([3, 5, 6], [2, 4, 4]),
           (3, 6): ([3, 6], [2, 5]), (3,): ([3], [2]), (6,): ([6], [5])}


def revise_kpts(kpts, scores, valid_frames):
    """a copy of kpts (N, 17, 2) in which, on the valid frames, low-score leg joints take the position of the joint above them"""
    out = np.array(kpts, copy=True)
    for f in np.asarray(valid_frames, dtype=np.int64):
        low = tuple(j for j in (2, 3, 5, 6) if scores[f, j] < SCORE_THRESHOLD)
        if low in _REVISE:
            dst, src = _REVISE[low]
            out[f, dst] = out[f, src]
    return out


def normalize_screen_coordinates(x, w, h):
    return x / w * 2 - np.array([1, h / w])


def mirror_input(x):
    """(..., 17, 2): x negated, left and right joints swapped"""
    out = np.array(x, copy=True)
    out[..., 0] *= -1
    return out[..., _MIRROR, :]


def mirror_output(y):
    """(..., 17, 3): x negated, left and right joints swapped (its own inverse)"""
    out = np.array(y, copy=True)
    out[..., 0] *= -1
    return out[..., _MIRROR, :]


def camera_to_world(x, q=CAMERA_QUATERNION):
    """v + 2 (q_w (q x v) + q x (q x v)) in float32, t = 0"""
    v = np.asarray(x, np.float32)
    qv = np.broadcast_to(np.asarray(q, np.float32)[1:], v.shape)
    uv = np.cross(qv, v)
    uuv = np.cross(qv, uv)
    return (v + np.float32(2) * (np.float32(q[0]) * uv + uuv)).astype(np.float32)


def lift_chunks(forward, x_norm, spec, flip_augment=True) -> np.ndarray:
    """The chunk loop of the lifter, apart from the device: x_norm (n, 17, 2) float32 -> (n, 17, 3) float32.
    forward: (b, 17, chunk + 2 pad, 2) float32 (joint-major) -> (b, 17, chunk, 3); b = 2 with flip_augment (the clip, its mirror image).
    `pad` frames are replicated on both sides of the clip; the last chunk is filled up with its last frame (those outputs are dropped)."""
    x = np.asarray(x_norm, np.float32)
    n, pad, chunk = x.shape[0], spec.pad, spec.chunk
    xp = np.pad(x, ((pad, pad), (0, 0), (0, 0)), mode="edge")
    out = np.empty((n, NUM_JOINTS, 3), np.float32)
    for s in range(0, n, chunk):
        m = min(chunk, n - s)
        win = xp[s:s + m + 2 * pad]
        if m < chunk:
            win = np.pad(win, ((0, chunk - m), (0, 0), (0, 0)), mode="edge")
        batch = [win, mirror_input(win)] if flip_augment else [win]
        y = forward(np.ascontiguousarray(np.stack(batch).transpose(0, 2, 1, 3)))
        y = np.asarray(y, np.float32).transpose(0, 2, 1, 3)[:, :m]
        out[s:s + m] = (y[0] + mirror_output(y[1])) / np.float32(2) if flip_augment else y[0]
    return out


def _check_input(x):
    if x.ndim != 3 or x.shape[1] != NUM_JOINTS or x.shape[2] != 2:
        raise ValueError(f"GAST-Net lifts (N, {NUM_JOINTS}, 2) key points; got {x.shape}")
    if x.shape[0] < 1:
        raise ValueError("GAST-Net: the clip has no valid frame")


def load_state_dict(spec=gn.GastNetSpec(), seed=7) -> dict:
    return weights.get_state_dict(CHECKPOINT, gn.gastnet_param_shapes(spec), seed=seed, synth=gn.synth_params, strip_prefix="module.")


class GastNetLifter:
    """The resident model: the layer program with every parameter in its blob, on one context, `max_batch` samples wide (2: one
    chunk and its mirror image; `lift_many` fills a wider batch with the chunks of several tracks).

    numerics: as Net's (None: the process default at this moment).  blob_fn(program) -> Net's blob_dev (a weight blob that is already
    on the device) or None."""

    stream_rule = "GastNet"           # person_stream.PersonStreams(lifter=): the valid frames compacted, windows over those

    def __init__(self, device=0, numerics=None, ctx=None, state_dict=None, spec=gn.GastNetSpec(), flip_augment=True, max_batch=2,
                 blob_fn=None):
        self.spec = spec
        self.flip_augment = bool(flip_augment)
        self.samples_per_chunk = 2 if self.flip_augment else 1      # the window and its mirror image
        if max_batch < (2 if self.flip_augment else 1):
            raise ValueError(f"GastNetLifter: max_batch = {max_batch}; flip augmentation needs two samples per chunk")
        sd = load_state_dict(spec) if state_dict is None else weights.strip_key_prefix(state_dict, "module.")
        self._own_ctx = ctx is None
        self.ctx = _lib.Context(device) if ctx is None else ctx
        prog = gn.build_gastnet_program(spec, sd)
        self.net = Net(self.ctx, prog, max_batch=int(max_batch), numerics=numerics, blob_dev=None if blob_fn is None else blob_fn(prog))
        self.stage_ms = None

    def _forward(self, batch, ms):
        b = batch.shape[0]
        inp = np.zeros(batch.shape[:3] + (4,), np.float32)
        inp[..., :2] = batch
        if ms is not None:
            self.ctx.timer_start()
        self.ctx.h2d(self.net.buffer("input")[0], inp)
        if ms is not None:
            ms["upload"] += self.ctx.timer_stop()
            self.ctx.timer_start()
        self.net.run(b)
        if ms is not None:
            ms["program"] += self.ctx.timer_stop()
        return self.net.read("output", b)

    def lift(self, x_norm, timed=False) -> np.ndarray:
        """x_norm (n, 17, 2) normalised H36M key points of the valid frames, n >= 1 -> (n, 17, 3) float32 camera-space joints.
        timed: also leaves {"upload", "program"} device milliseconds (HIP events around the copies and the program's launches, summed
        over the chunks) and "post" (the host's share: download, flip merge; wall milliseconds) in self.stage_ms."""
        x = np.ascontiguousarray(np.asarray(x_norm), dtype=np.float32)
        _check_input(x)
        ms = {"upload": 0.0, "program": 0.0, "post": 0.0} if timed else None
        t0 = time.perf_counter()
        out = lift_chunks(lambda b: self._forward(b, ms), x, self.spec, self.flip_augment)
        if timed:
            ms["post"] = (time.perf_counter() - t0) * 1e3 - ms["upload"] - ms["program"]
        self.stage_ms = ms
        return out

    def lift_many(self, xs, rotate=True) -> list:
        """xs: list of (n_i, 17, 2) normalised H36M key points (each track's valid frames, n_i >= 1) -> list of (n_i, 17, 3) float32, in
        ONE pp_gastnet_lift_many call: the chunks of every track share the net's batch, windows, mirror images, flip merge and the
        camera rotation are device kernels, one upload and one download.  Element i equals camera_to_world(self.lift(xs[i])) bit for
        bit (self.lift(xs[i]) with rotate=False)."""
        xs = [np.ascontiguousarray(np.asarray(x), dtype=np.float32) for x in xs]
        for x in xs:
            _check_input(x)
        if not xs:
            return []
        seg = np.array([x.shape[0] for x in xs], np.int32)
        packed = np.ascontiguousarray(np.concatenate(xs))
        out = np.empty((int(seg.sum()), NUM_JOINTS, 3), np.float32)
        named = self.net.prog.named
        _lib.check(self.ctx.lib.pp_gastnet_lift_many(self.net.handle, named["input"], named["output"], _lib.ptr(packed), _lib.ptr(seg),
                                                     len(seg), self.spec.pad, int(self.flip_augment),
                                                     _lib.ptr(CAMERA_QUATERNION) if rotate else None, _lib.ptr(out), _lib.PP_MEM_HOST),
                   "pp_gastnet_lift_many")
        ends = np.cumsum(seg)
        return [out[e - n:e] for e, n in zip(ends, seg)]

    def close(self):
        if getattr(self, "net", None) is not None:
            self.net.close()
            self.net = None
        if self._own_ctx and getattr(self, "ctx", None) is not None:
            self.ctx.close()
            self.ctx = None


_cache: dict = {}


def _model(device=0):
    if device not in _cache:
        _cache[device] = GastNetLifter(device)
    return _cache[device]


def process_gastnet(key):
    from ..pipeline import TopDownPerson, VideoInfo

    key = key.copy()
    keypoints = (TopDownPerson & key).fetch1("keypoints")
    height, width = (VideoInfo & key).fetch1("height", "width")
    keypoints = np.asarray(keypoints)
    if keypoints.ndim != 3 or keypoints.shape[1] != NUM_JOINTS or keypoints.shape[2] < 3:
        raise ValueError(f"process_gastnet: TopDownPerson.keypoints of shape {keypoints.shape}, expected (N, {NUM_JOINTS}, 3) COCO key points")

    kpts, scores, valid = h36m_coco_format(keypoints[..., :2], keypoints[..., 2])
    if len(valid) == 0:
        raise ValueError("process_gastnet: the clip has no valid frame (every frame's key points sum to 0)")
    kpts = revise_kpts(kpts, scores, valid)

    x = normalize_screen_coordinates(kpts[valid], w=width, h=height)
    x = x.astype(np.float32)                                   # torch.from_numpy(batch.astype('float32')) rounds to float32
    model = _model()
    if hasattr(model, "lift_many"):                            # the one-call device path: windows, flip merge and rotation on the GPU
        prediction = model.lift_many([x])[0]
    else:                                                      # a model that offers `lift` alone: the same values, rotated on the host
        prediction = camera_to_world(model.lift(x))

    keypoints_3d = np.zeros((keypoints.shape[0], NUM_JOINTS, 3))
    keypoints_3d[valid] = prediction
    is_valid = np.zeros(keypoints.shape[0], bool)
    is_valid[valid] = True
    return {"keypoints_3d": keypoints_3d, "keypoints_valid": [bool(v) for v in is_valid]}
