"""Drop-in for pose_pipeline/wrappers/poseformer.py:9-104 `process_liftformer`.

Same signature, table reads (`TopDownPerson.keypoints`, `VideoInfo.height/width`) and return value: the `key` dict it was given, with
`keypoints_3d` (N, 17, 3) float64 added -- rows 0..39 and N-40..N-1 zeros, row 40 + i the centre frame of the window [i, i + 81).
There is no `keypoints_valid`.  The COCO -> H36M conversion (:19-53) is restated here with the same float32 rounding points, and the
normalisation keeps the reference's quirk: x is divided by the HEIGHT and y by the WIDTH (:57).

The reference runs the whole network once per window in a batch-1 loop.  Here the spatial transformer runs once per frame of the clip
and only the temporal transformer runs per window, batched (pp_poseformer_lift, models/poseformer.py); in float64 the two forms
agree exactly (tests/test_poseformer.py).

Declared differences:
  * Inference mode.  The reference never calls `.eval()`: its DropPath (rates 0 .. 0.1) is live and its output is random from call to
    call.  Here the network is the deterministic inference-mode one.
  * N < 81: ValueError naming the 81-frame receptive field (the reference: a ValueError from np.stack of an empty list).
  * Other than 17 joints: ValueError (the reference: a torch shape error).
  * The checkpoint is `poseformer/detected81f.bin` under MODEL_DATA_DIR (the reference: `../3rdparty/poseformer/` beside its wrapper
    file), `checkpoint["model_pos"]` with the `module.` prefix of nn.DataParallel dropped; a missing key is a KeyError (the reference
    loads with strict=False).  It is never fetched; POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded parameters.
  * The video is not touched.
  * UNPINNED (common/model_poseformer.py is not in the reference tree), to check first with the checkpoint at hand: the key names,
    LayerNorm eps 1e-6 in the blocks against 1e-5 in head.0, the qkv channel order, erf GELU, weighted_mean.weight's shape.
"""
from __future__ import annotations

import numpy as np

from .. import _lib, weights
from ..models import poseformer as pf
from ..program import Net

RECEPTIVE_FIELD = 81
NUM_JOINTS = 17
CHECKPOINT = "poseformer/detected81f.bin"


# COCO joint ids used below
_NOSE, _L_EYE, _R_EYE, _L_EAR, _R_EAR, _L_SHO, _R_SHO, _L_HIP, _R_HIP = 0, 1, 2, 3, 4, 5, 6, 11, 12
# H36M joints that are COCO joints as they stand: H36M index -> COCO index (hips / knees / ankles, shoulders / elbows / wrists)
_H36M_FROM_COCO = {1: 12, 2: 14, 3: 16, 4: 11, 5: 13, 6: 15, 11: 5, 12: 7, 13: 9, 14: 6, 15: 8, 16: 10}


def _mean32(*parts):
    """float32 mean of a few arrays: each rounded to float32, added left to right in float32, divided by the count in float32 (what
    numpy's mean(..., dtype=float32) over a short strided axis evaluates)"""
    acc = parts[0].astype(np.float32)
    for p in parts[1:]:
        acc = acc + p.astype(np.float32)
    return acc / np.float32(len(parts))


def coco_h36m(keypoints) -> np.ndarray:
    """(N, 17, 2) COCO key points -> (N, 17, 2) float32 in H36M order: the conversion of wrappers/poseformer.py:19-53 (the landmark
    rules of GAST-Net's mpii_coco_h36m tool), written from what it computes rather than how.  Twelve joints are COCO joints
    (_H36M_FROM_COCO); the five that COCO lacks are built from landmarks.  With sho / hip / torso the float32 means of the two
    shoulders, the two hips and all four, and `nose` in the input's own dtype (arithmetic that involves it runs in that dtype and is
    rounded to float32 when stored -- the points below are where the reference rounds, pinned by tests/golden/poseformer_pre.npz):
      0  pelvis  = hip
      8  thorax  = f32(sho + (nose - sho) / 3); then y = f32(y - (mean32(eyes.y) - nose.y) * 2 / 3)
      7  spine   = torso, with x = f32(x + 2 * (x - mean32(pelvis.x, thorax.x)))          (all float32)
      9  neck    = f32(nose), then f32(neck - (neck - sho) / 4)                            (all float32)
      10 head    = (mean32 of both eyes' and both ears' x,  f32((f32(l_eye.y) + f32(r_eye.y)) - nose.y))"""
    kp = np.asarray(keypoints)
    if kp.ndim != 3 or kp.shape[1] != NUM_JOINTS or kp.shape[2] != 2:
        raise ValueError(f"coco_h36m: key points of shape {kp.shape}, expected (N, {NUM_JOINTS}, 2)")
    f32 = np.float32
    joint = lambda j: kp[:, j, :]                                      # noqa: E731
    nose = joint(_NOSE)
    sho, hip = _mean32(joint(_L_SHO), joint(_R_SHO)), _mean32(joint(_L_HIP), joint(_R_HIP))
    torso = _mean32(joint(_L_SHO), joint(_R_SHO), joint(_L_HIP), joint(_R_HIP))
    eyes_y = _mean32(joint(_L_EYE)[:, 1], joint(_R_EYE)[:, 1])

    thorax = (sho + (nose - sho) / 3).astype(f32)
    spine = torso.copy()
    spine[:, 0] = torso[:, 0] + 2 * (torso[:, 0] - _mean32(hip[:, 0], thorax[:, 0]))
    thorax[:, 1] = (thorax[:, 1] - (eyes_y - nose[:, 1]) * 2 / 3).astype(f32)
    neck = nose.astype(f32)
    neck = neck - (neck - sho) / 4
    head = np.stack([_mean32(*(joint(j)[:, 0] for j in (_L_EYE, _R_EYE, _L_EAR, _R_EAR))),
                     ((joint(_L_EYE)[:, 1].astype(f32) + joint(_R_EYE)[:, 1].astype(f32)) - nose[:, 1]).astype(f32)], axis=1)

    built = {0: hip, 7: spine, 8: thorax, 9: neck, 10: head}
    out = np.stack([built[j] if j in built else joint(_H36M_FROM_COCO[j]).astype(f32) for j in range(NUM_JOINTS)], axis=1)
    assert out.dtype == f32
    return out


def normalize(keypoints_h36m, height, width) -> np.ndarray:
    """:57 -- x / height, y / width (the reference's order, kept), float64; the network's input is this rounded to float32 (:95)"""
    return keypoints_h36m / np.array([height, width])[None, None, :]


def windows(x, receptive_field=RECEPTIVE_FIELD) -> np.ndarray:
    """:61-64 -- (N, J, 2) -> (N - 80, 81, J, 2), window i = frames [i, i + 81)"""
    x = np.asarray(x)
    if x.shape[0] < receptive_field:
        raise ValueError(f"PoseFormer needs at least {receptive_field} frames (its receptive field); the clip has {x.shape[0]}")
    return np.stack([x[i:i + receptive_field, :, :2] for i in range(x.shape[0] - receptive_field + 1)], axis=0)


def _check_input(x):
    if x.ndim != 3 or x.shape[1] != NUM_JOINTS or x.shape[2] != 2:
        raise ValueError(f"PoseFormer lifts (N, {NUM_JOINTS}, 2) key points; got {x.shape}")
    if x.shape[0] < RECEPTIVE_FIELD:
        raise ValueError(f"PoseFormer needs at least {RECEPTIVE_FIELD} frames (its receptive field); the clip has {x.shape[0]}")


def load_state_dict(seed=5) -> dict:
    shapes = pf.poseformer_param_shapes(pf.PoseFormerSpec())
    return weights.get_state_dict(CHECKPOINT, shapes, seed=seed, synth=pf.synth_params, strip_prefix="module.")


class PoseFormerLifter:
    """The resident model: the temporal program with every parameter in its blob, on one context.

    numerics: as Net's (None: the process default at this moment).  channel_pad: 0 keeps the real 544 / 1632 / 1088 channels, which
    is the form measured no slower in either numerics (DESIGN_LOG.md 5k); 128 builds the padded program (640 / 1920 / 1152), kept for that comparison."""

    def __init__(self, device=0, max_windows=64, numerics=None, ctx=None, state_dict=None, channel_pad=0):
        self.spec = pf.PoseFormerSpec()
        sd = load_state_dict() if state_dict is None else state_dict
        self._own_ctx = ctx is None
        self.ctx = _lib.Context(device) if ctx is None else ctx
        self.max_windows = int(max_windows)
        self.net = Net(self.ctx, pf.build_poseformer_program(self.spec, sd, channel_pad), max_batch=self.max_windows, numerics=numerics)
        self.stage_ms = None

    def lift(self, x_norm, timed=False) -> np.ndarray:
        """x_norm (N, 17, 2) normalised H36M key points, N >= 81 -> (N - 80, 17, 3) float32: row i is frame i + 40.
        timed: also leaves the device milliseconds (spatial, gather, temporal program, mean + head) in self.stage_ms."""
        x = np.ascontiguousarray(np.asarray(x_norm), dtype=np.float32)
        _check_input(x)
        n = x.shape[0]
        out = np.zeros((n - RECEPTIVE_FIELD + 1, NUM_JOINTS * 3), np.float32)
        ms = np.zeros(4, np.float32) if timed else None
        nm, po = self.net.prog.named, self.net.prog.param_offsets
        _lib.check(self.ctx.lib.pp_poseformer_lift(self.net.handle, nm["input"], nm["output"], po["spatial_params"], po["temporal_pos"],
                                                   po["head_params"], _lib.ptr(x), n, _lib.ptr(out), _lib.PP_MEM_HOST, _lib.ptr(ms)),
                   "pp_poseformer_lift")
        self.stage_ms = ms
        return out.reshape(-1, NUM_JOINTS, 3)

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
        _cache[device] = PoseFormerLifter(device)
    return _cache[device]


def process_liftformer(key):
    from ..pipeline import TopDownPerson, VideoInfo

    keypoints = (TopDownPerson & key).fetch1("keypoints")
    height, width = (VideoInfo & key).fetch1("height", "width")
    keypoints = np.asarray(keypoints)
    if keypoints.ndim != 3 or keypoints.shape[1] != NUM_JOINTS:
        raise ValueError(f"process_liftformer: TopDownPerson.keypoints of shape {keypoints.shape}, expected (N, {NUM_JOINTS}, 3) COCO key points")
    if keypoints.shape[0] < RECEPTIVE_FIELD:
        raise ValueError(f"PoseFormer needs at least {RECEPTIVE_FIELD} frames (its receptive field); the clip has {keypoints.shape[0]}")

    keypoints = coco_h36m(keypoints[..., :2])
    keypoints = normalize(keypoints, height, width)

    kp3d = _model().lift(keypoints.astype(np.float32))               # torch.Tensor(...) of :95 rounds to float32
    pad = (RECEPTIVE_FIELD - 1) // 2
    key["keypoints_3d"] = np.concatenate([np.zeros((pad, NUM_JOINTS, 3)), kp3d, np.zeros((pad, NUM_JOINTS, 3))], axis=0)   # :101
    return key
