"""Drop-in for pose_pipeline/wrappers/mmaction.py:9-86 `mmaction_skeleton_action_person` (the SkeletonAction stage).

Same signature, table reads (`TopDownPerson.keypoints`, `VideoInfo.height/width`) and return value: the `key` dict it was given, with
`top5` (per window a list of five (label, score)), `action_scores` (n_windows, num_classes), `label_map`, `action_window_len` = 48 and
`stride` added.  Kept reference behaviour, quirks included:

  * Windows are `range(0, N - clip_len - 1, stride)` (:56): a track of N frames has N - 49 windows at stride 1, none for N <= 49.
  * A window hands the sampler `total_frames = 10` (:61, TOTAL_FRAMES below) although it holds 48 frames.  UniformSampleFrames(clip_len
    48, num_clips 10, test_mode) then takes its "simple strategy" branch (num_frames < clip_len): clip i starts at i * 10 // 10 = i, and
    frame_inds = concat(arange(i, i + 48)) mod 10: only the FIRST 10 frames of a window are ever read, each clip a cyclic repetition of
    them.  The seeded RNG (seed 255) is consulted only on the other two branches, which `uniform_sample_frames` also restates.
  * test_pipeline of slowonly_r50_u48_240e_ntu120_xsub_keypoint.py: PoseDecode (float32), PoseCompact(hw_ratio 1., allow_imgpad True;
    padding 0.25, threshold 10), Resize((-1, 64)), CenterCrop(64), GeneratePoseTarget(sigma 0.6, use_score, with_kp, double, the COCO
    left / right joints), FormatShape('NCTHW'): 20 clips (10 plain, then their 10 mirrored copies) of [17][48][64][64].
  * Zero windows: the reference's code runs through with an empty list: `top5` = [], `action_scores` = np.array([]) (shape (0,),
    float64), the other three keys as usual.  Kept.

The host computes, per window, the key points of the window's distinct sampled frames in crop pixels (`window_keypoints`, float32 /
float64 exactly where the transforms are); pp_pose_target renders them and their mirrored copies on the device, models/posec3d.py is
the network, and the soft-max per clip and the mean over the clips (average_clips = 'prob') are 20 x 81 float32 numbers on the host.

Front-stage de-duplication (`dedup`): conv1, the pool and layer1 are per-frame, and a window has at most 2 * TOTAL_FRAMES distinct
frame maps but 960 clip positions.  With `dedup` the front program runs on the distinct maps and pp_gather_samples expands its OUTPUT
to clip order; without it the gather expands the INPUT maps and the front program runs on every clip position.  Per-sample results do
not depend on the batch they ride in, so the two agree bit for bit (tests/test_gpu_posec3d.py).

Declared differences:
  * The checkpoint `mmaction2/checkpoints/posec3d_ava.pth` and the label map `mmaction2/tools/data/ava/label_map.txt` are looked up
    under $PIPELINE_3RDPARTY and never fetched (the reference names a download URL and two absolute paths of its author's machine);
    a missing file raises FileNotFoundError with the path.  POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded parameters and the labels
    `class_1` ... `class_80`.  num_classes = the largest label id + 1 (:40-43).
  * top5: a class index without an entry in the label map (index 0 of the AVA map) is labelled by its number as a string; the
    reference raises KeyError when such a class reaches the top five.
  * `device` is accepted for the signature's sake: "cuda" / "cuda:k" / k select GPU k; there is no CPU path.
  * UNPINNED (mmaction2 is not in the reference tree), to check first with mmaction2 and the checkpoint at hand: the readings above
    and in models/posec3d.py; how `double=True` makes the mirrored copies -- built here as the 0.x sources are read: Flip(flip_ratio 1,
    left_kp, right_kp) of the key points (x -> 64 - x for non-zero x, left / right joints exchanged) and a second rendering; the other
    reading, heatmap[..., ::-1][:, exchanged channels], mirrors the rendered map instead (pixel x shows pixel 63 - x: one pixel apart,
    and x == 0 differs) and is an OPEN question until the installed mmaction2 is at hand; that PoseDecode casts to float32 and CenterCrop's subtraction of the integer crop origin promotes the key
    points to float64; that PoseCompact's half sizes are float64 (float32 scalar times a Python float under NumPy < 2) while its
    centre stays float32; Resize's `int(x * scale + 0.5)` and its float32 scale factor; that CenterCrop shifts ALL key points (absent
    ones included, whose score is zero) while PoseCompact shifts only non-zero coordinates; eps = 1e-4 and `score < eps` skips;
    average_clips = 'prob'; UniformSampleFrames' default seed 255.
"""
from __future__ import annotations

import os
import time

import numpy as np

from .. import _lib, weights
from ..models import posec3d as pm

TOTAL_FRAMES = 10                 # pose_pipeline/wrappers/mmaction.py:61  `"total_frames": 10,`
START_INDEX = 0                   # :62
CLIP_LEN = 48                     # test_pipeline[0]["clip_len"] (:53)
NUM_CLIPS = 10
SAMPLER_SEED = 255                # UniformSampleFrames(seed=255)
PADDING, THRESHOLD, HW_RATIO = 0.25, 10, (1.0, 1.0)        # PoseCompact
MAP_SIZE = 64                     # Resize((-1, 64)), CenterCrop(64)
SIGMA = 0.6                       # GeneratePoseTarget
LEFT_KP, RIGHT_KP = (1, 3, 5, 7, 9, 11, 13, 15), (2, 4, 6, 8, 10, 12, 14, 16)
CHECKPOINT = "mmaction2/checkpoints/posec3d_ava.pth"
LABEL_MAP = "mmaction2/tools/data/ava/label_map.txt"


# ---- sampling and the key-point transforms (host) ---------------------------------------------------------------------------------
def uniform_sample_frames(total_frames: int, clip_len: int, num_clips: int, seed: int = SAMPLER_SEED, start_index: int = START_INDEX):
    """UniformSampleFrames(test_mode=True)._get_test_clips + the modulo and offset of __call__ -> int64 [num_clips * clip_len]"""
    rng = np.random.RandomState(seed)            # np.random.seed(seed) and the global functions: the same MT19937 stream
    n = int(total_frames)
    if n < clip_len:
        starts = np.arange(num_clips) if n < num_clips else np.arange(num_clips) * n // num_clips
        inds = (starts[:, None] + np.arange(clip_len)[None, :]).reshape(-1)
    elif n < 2 * clip_len:
        parts = []
        for _ in range(num_clips):
            offset = np.zeros(clip_len + 1, np.int64)
            offset[rng.choice(clip_len + 1, n - clip_len, replace=False)] = 1
            parts.append(np.arange(clip_len) + np.cumsum(offset)[:-1])
        inds = np.concatenate(parts)
    else:
        bids = np.arange(clip_len + 1) * n // clip_len
        bsize, bst = np.diff(bids), bids[:clip_len]
        inds = np.concatenate([bst + rng.randint(bsize) for _ in range(num_clips)])
    return np.mod(inds, n).astype(np.int64) + start_index


def window_starts(n_frames: int, clip_len: int = CLIP_LEN, stride: int = 1) -> list:
    return list(range(0, n_frames - clip_len - 1, stride))          # :56


def mirror_perm(n_joints: int = 17) -> np.ndarray:
    perm = np.arange(n_joints, dtype=np.int32)
    perm[list(LEFT_KP)], perm[list(RIGHT_KP)] = RIGHT_KP, LEFT_KP
    return perm


def window_keypoints(keypoints, img_shape, frames, size: int = MAP_SIZE) -> np.ndarray:
    """keypoints [>= max(frames) + 1][K][3] of ONE window (x, y, score), img_shape (h, w) of the video, frames: the distinct sampled
    frame indices -> float64 [len(frames)][K][3]: (x, y) in the size x size crop as GeneratePoseTarget sees them, and the score"""
    kp = np.asarray(keypoints)[np.asarray(frames)]
    xy = kp[..., :2].astype(np.float32)                              # PoseDecode
    score = kp[..., 2].astype(np.float32)
    h, w = int(img_shape[0]), int(img_shape[1])
    # PoseCompact: one box over the non-zero coordinates of every sampled frame
    xy[np.isnan(xy)] = 0.0
    kx, ky = xy[..., 0], xy[..., 1]
    nzx, nzy = kx != 0, ky != 0
    min_x, max_x = np.min(kx[nzx], initial=np.inf), np.max(kx[nzx], initial=-np.inf)
    min_y, max_y = np.min(ky[nzy], initial=np.inf), np.max(ky[nzy], initial=-np.inf)
    if not (max_x - min_x < THRESHOLD or max_y - min_y < THRESHOLD):
        f32 = np.float32
        cx, cy = float((f32(max_x) + f32(min_x)) / f32(2)), float((f32(max_y) + f32(min_y)) / f32(2))
        half_w = float((f32(max_x) - f32(min_x)) / f32(2)) * (1 + PADDING)
        half_h = float((f32(max_y) - f32(min_y)) / f32(2)) * (1 + PADDING)
        half_h = max(HW_RATIO[0] * half_w, half_h)
        half_w = max(1 / HW_RATIO[1] * half_h, half_w)
        x0, x1, y0, y1 = int(cx - half_w), int(cx + half_w), int(cy - half_h), int(cy + half_h)      # allow_imgpad: not clipped
        kx[nzx] -= x0                                               # float32 array minus a Python int stays float32
        ky[nzy] -= y0
        h, w = y1 - y0, x1 - x0
    # Resize((-1, 64), keep_ratio): mmcv.rescale_size with (inf, 64)
    scale = min(np.inf, size / min(h, w))
    new_w, new_h = int(w * float(scale) + 0.5), int(h * float(scale) + 0.5)
    xy = xy * np.array([new_w / w, new_h / h], dtype=np.float32)
    # CenterCrop(64): kps - crop_bbox[:2], an int64 array: the key points become float64
    left, top = (new_w - size) // 2, (new_h - size) // 2
    xy = xy - np.array([left, top], dtype=np.int64)
    return np.concatenate([xy.astype(np.float64), score.astype(np.float64)[..., None]], axis=-1)


def load_label_map(path: str) -> dict:
    """`id: name` lines -> {id: name} (:28-37)"""
    with open(path) as f:
        lines = [x.strip().split(": ") for x in f.readlines()]
    return {int(x[0]): x[1] for x in lines}


def get_label_map() -> dict:
    path = os.path.join(weights.model_data_dir(), LABEL_MAP)
    if os.path.exists(path):
        return load_label_map(path)
    if os.environ.get("POSEPIPE_SYNTHETIC_WEIGHTS") == "1":
        return {i: f"class_{i}" for i in range(1, 81)}
    raise FileNotFoundError(f"{path} (set POSEPIPE_SYNTHETIC_WEIGHTS=1 to run with seeded synthetic weights and labels)")


def load_state_dict(spec: pm.PoseC3DSpec, seed: int = 11) -> dict:
    return weights.get_state_dict(CHECKPOINT, pm.posec3d_param_shapes(spec), seed=seed, synth=pm.synth_params)


def average_clips(logits: np.ndarray) -> np.ndarray:
    """Recognizer3D.average_clip, 'prob': float32 soft-max per clip, then the mean over the clips"""
    x = np.asarray(logits, np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).mean(axis=0, dtype=np.float32)


def top5(x, label_map: dict) -> list:
    ind = np.argpartition(x, -5)[-5:]                                # :75-78
    ind = ind[np.argsort(-x[ind])]
    return [(label_map.get(int(y), str(int(y))), x[y]) for y in ind]


# ---- the resident model ------------------------------------------------------------------------------------------------------------
class SkeletonActionModel:
    """Everything of the stage that lives on one context: the key-point and index buffers, the three programs and their schedule.
    `scores` maps a track to the (n_windows, num_classes) action scores.  total_frames: what the wrapper tells the sampler
    (TOTAL_FRAMES); clips_per_pass: None sizes a pass from the spec (models/posec3d.clips_per_pass).
    timing (also an attribute that may be changed between calls): put device events around the stages, so that `last_timing` holds
    the per-stage milliseconds (targets, front, gather, trunk, head) beside `total_s` and `windows`; the events synchronise the stream
    at every stage, so it is off by default and throughput is measured with it off."""

    def __init__(self, ctx=None, numerics=None, state_dict=None, spec=None, num_clips=NUM_CLIPS, clip_len=CLIP_LEN, dedup=True,
                 total_frames=TOTAL_FRAMES, clips_per_pass=None, device=0, timing=False):
        spec = pm.PoseC3DSpec() if spec is None else spec
        self.spec = spec = pm.replace(spec, clip_len=int(clip_len))
        assert spec.height == spec.width, "Resize((-1, s)) + CenterCrop(s) make a square map"
        sd = load_state_dict(spec) if state_dict is None else state_dict
        self.num_clips, self.clip_len, self.dedup, self.total_frames = int(num_clips), int(clip_len), bool(dedup), int(total_frames)
        self.frame_inds = uniform_sample_frames(self.total_frames, self.clip_len, self.num_clips)
        self.frames = np.unique(self.frame_inds)                     # the distinct frames of a window that are read at all
        n = self.n_frames = len(self.frames)
        slot = np.searchsorted(self.frames, self.frame_inds).reshape(self.num_clips, self.clip_len)
        self.map_index = np.concatenate([slot, slot + n]).astype(np.int32)          # [2 num_clips][clip_len] -> one of the 2 n maps
        self.n_clips = 2 * self.num_clips
        self._own_ctx = ctx is None
        self.ctx = ctx = _lib.Context(device) if ctx is None else ctx
        programs = pm.build_programs(spec, sd)
        self.clips_per_pass = pm.clips_per_pass(spec, self.n_clips, programs[0]) if clips_per_pass is None else int(clips_per_pass)
        pass_frames = self.clips_per_pass * self.clip_len
        self.net = pm.PoseC3DNet(ctx, spec, sd, numerics=numerics, max_clips=self.clips_per_pass,
                                 front_batch=2 * n if self.dedup else pass_frames, programs=programs)
        self.K = spec.in_channels
        self._dev = {"kps": ctx.malloc(n * self.K * 3 * 8), "perm": ctx.malloc(self.K * 4), "idx": ctx.malloc(self.map_index.size * 4)}
        if not self.dedup:
            self._dev["maps"] = ctx.malloc(2 * n * self.net.input_bytes)
        ctx.h2d(self._dev["perm"], mirror_perm(self.K))
        ctx.h2d(self._dev["idx"], self.map_index)
        self.timing = bool(timing)
        self.last_timing = None

    def _gather(self, src, idx_off, n, sample_bytes, dst):
        _lib.check(self.ctx.lib.pp_gather_samples(self.ctx.handle, _lib.ptr(src), 2 * self.n_frames, _lib.ptr(self._dev["idx"] + 4 * idx_off),
                                                  n, sample_bytes // 4, _lib.ptr(dst)), "pp_gather_samples")

    def clip_logits(self, kps: np.ndarray) -> np.ndarray:
        """kps float64 [n_frames][K][3] (window_keypoints) -> logits [2 num_clips][num_classes]"""
        ctx, net, s, n = self.ctx, self.net, self.spec, self.n_frames
        kps = np.ascontiguousarray(kps, np.float64)
        assert kps.shape == (n, self.K, 3), kps.shape
        ms = dict(targets=0.0, front=0.0, gather=0.0, trunk=0.0, head=0.0)

        def stage(name, fn):
            if self.timing:
                ctx.timer_start()
            fn()
            if self.timing:
                ms[name] += ctx.timer_stop()

        maps = net.input_ptr if self.dedup else self._dev["maps"]
        ctx.h2d(self._dev["kps"], kps)                                # synchronous: the host array may go once this returns
        stage("targets", lambda: _lib.check(ctx.lib.pp_pose_target(ctx.handle, _lib.ptr(self._dev["kps"]), n, self.K, s.height, s.width, SIGMA,
                                                                   _lib.ptr(self._dev["perm"]), s.c_pad, _lib.ptr(maps)), "pp_pose_target"))
        if self.dedup:
            stage("front", lambda: net.run_front(2 * n))
        out = np.empty((self.n_clips, s.num_classes), np.float32)
        for c0 in range(0, self.n_clips, self.clips_per_pass):
            nc = min(self.clips_per_pass, self.n_clips - c0)
            m, off = nc * self.clip_len, c0 * self.clip_len
            if self.dedup:
                stage("gather", lambda: self._gather(net.front_out_ptr, off, m, net.front_out_bytes, net.x0_ptr))
            else:
                stage("gather", lambda: self._gather(maps, off, m, net.input_bytes, net.input_ptr))
                stage("front", lambda: (net.run_front(m), net.front_to_trunk(nc)))
            stage("trunk", lambda: net.run_trunk(nc, head=False))

            def head():
                net.run_trunk(nc, body=False)
                out[c0:c0 + nc] = net.read_logits(nc)              # synchronous: the programs' buffers are free for the next pass
            stage("head", head)
        self.last_timing = ms if self.timing else None
        return out

    def scores(self, keypoints, img_shape, stride=1) -> np.ndarray:
        """keypoints [N][K][3] of one person's track, img_shape (h, w) -> float32 (n_windows, num_classes); (0, num_classes) for a track
        without a window.  last_timing: per-stage device milliseconds summed over the windows (when `timing` is set), `total_s` and
        `windows` always."""
        keypoints = np.asarray(keypoints)
        starts = window_starts(keypoints.shape[0], self.clip_len, stride)
        out = np.zeros((len(starts), self.spec.num_classes), np.float32)
        total = dict(targets=0.0, front=0.0, gather=0.0, trunk=0.0, head=0.0)
        t0 = time.perf_counter()
        for i, start in enumerate(starts):
            kps = window_keypoints(keypoints[start:start + self.clip_len], img_shape, self.frames, self.spec.height)
            out[i] = average_clips(self.clip_logits(kps))
            for k, v in (self.last_timing or {}).items():
                total[k] += v
        self.last_timing = dict(total if self.timing else {}, total_s=time.perf_counter() - t0, windows=len(starts))
        return out

    def close(self):
        for p in getattr(self, "_dev", {}).values():
            self.ctx.free(p)
        self._dev = {}
        if getattr(self, "net", None) is not None:
            self.net.close()
            self.net = None
        if self._own_ctx and getattr(self, "ctx", None) is not None:
            self.ctx.close()
            self.ctx = None


_cache: dict = {}


def _device_index(device) -> int:
    if isinstance(device, int):
        return device
    name = str(device)
    if name in ("cuda", "gpu"):
        return 0
    if name.startswith("cuda:"):
        return int(name[5:])
    raise ValueError(f"mmaction_skeleton_action_person: device {device!r}: only GPUs are supported (\"cuda\", \"cuda:k\")")


def _model(device=0):
    if device not in _cache:
        label_map = get_label_map()
        spec = pm.PoseC3DSpec(num_classes=int(np.max([k for k in label_map.keys()])) + 1)       # :40-43
        _cache[device] = (SkeletonActionModel(spec=spec, device=device), label_map)
    return _cache[device]


def mmaction_skeleton_action_person(key, device="cuda", stride=1):
    from ..pipeline import TopDownPerson, VideoInfo

    keypoints = (TopDownPerson & key).fetch1("keypoints")
    img_shape = (VideoInfo & key).fetch1("height", "width")
    model, label_map = _model(_device_index(device))
    scores = model.scores(keypoints, img_shape, stride=stride)
    results = [x for x in scores]

    key["top5"] = [top5(x, label_map) for x in results]
    key["action_scores"] = np.array(results)
    key["label_map"] = label_map
    key["action_window_len"] = model.clip_len
    key["stride"] = stride
    return key
