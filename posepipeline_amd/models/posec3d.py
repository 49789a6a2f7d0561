"""PoseC3D (Duan et al., CVPR 2022): the SlowOnly-R50 3D ResNet over key-point pseudo heat-maps behind
pose_pipeline/wrappers/mmaction.py:9-86 (`Recognizer3D` of slowonly_r50_u48_240e_ntu120_xsub_keypoint.py), inference mode.

mmaction2 is NOT in the reference tree (only the wrapper is): an UNPINNED restatement of its published 0.x sources.

  backbone   ResNet3dSlowOnly(depth 50, in_channels 17, base_channels 32, num_stages 3, stage_blocks (4, 6, 3), inflate (0, 1, 1),
             conv1_stride_s 1, pool1_stride_s 1, spatial_strides (2, 2, 2), temporal_strides (1, 1, 1), lateral False):
             conv1 1x7x7 -> MaxPool3d 1x3x3 stride 1 -> three stages of Bottleneck3d (style 'pytorch': the stride on conv2; inflate_style
             '3x1x1': an inflated block has conv1 3x1x1, conv2 1x3x3, conv3 1x1x1; the projection shortcut is a strided 1x1x1)
  head       I3DHead(512 -> num_classes): AdaptiveAvgPool3d(1), dropout (identity), fc_cls; Recognizer3D.average_clip with
             average_clips = 'prob': soft-max per clip, mean over the clips (the host's 20 x 81 numbers: wrappers/mmaction.py)

Parameter names are the checkpoint's: `backbone.conv1.conv.weight` [32][17][1][7][7], `backbone.conv1.bn.*`,
`backbone.layer2.0.conv1.conv.weight` [64][128][3][1][1], `...downsample.conv.weight`, `...downsample.bn.*`, `cls_head.fc_cls.*`.

Mapping onto 2D layer programs (no new op type: PP_OP_CONV, PP_OP_MAXPOOL, PP_OP_AVGPOOL):
  * a 1xkxk convolution is a 2D convolution with one FRAME per sample: batch = clips * T, sample [H][W][C]  (the frame view);
  * a 3x1x1 convolution is a 2D convolution with kernel (3, 1), padding (1, 0) and one CLIP per sample [T][H * W][C] (the clip view):
    rows are time steps, so the zero rows above t = 0 and below t = T - 1 are Conv3d's temporal padding, and clips never mix;
  * the two views are the SAME memory layout, so a view change is a device-to-device copy between two programs: `front` (frame view:
    conv1, the pool and the leading stages that are not inflated -- per-frame work only), `frame` (the 1x3x3 / 1x1x1 convolutions of
    the later stages, the spatial average) and `clip` (the 3x1x1 convolutions, the temporal average, fc_cls).  Each block of an
    inflated stage is: copy x to the clip program, one op there, copy the result back, one op range of the frame program.
    Buffers filled from outside a range are program inputs: a split net takes their per-sample maxima in the stand-alone pass that
    precedes every range that reads them.  In the clip view a sample (the unit of those maxima) is a clip, in the frame view a frame.
  * AdaptiveAvgPool3d(1) is PP_OP_AVGPOOL over H x W in the frame view, then PP_OP_AVGPOOL over T in the clip view (two float32 means
    instead of one: inside the tolerance of tests/test_gpu_posec3d.py); fc_cls is a 1x1 convolution, its rows padded to a multiple of 4.

UNPINNED, to check first with mmaction2 and the checkpoint at hand: the key names and the 5-D weight shapes; that `posec3d_ava.pth`
is this backbone (base_channels 32, three stages) with an 81-way head; that the projection shortcut has no activation and conv3's ReLU
comes after the addition; BatchNorm eps 1e-5; that the stem pool pads with -inf (MaxPool3d), not zeros; temporal_strides: (1, 1, 1)
by default, as the issue states it, while the published PoseC3D SlowOnly config may carry (1, 1, 2) (the stride on layer3.0's conv2
and projection; weight shapes do not reveal it): `PoseC3DSpec.temporal_strides` builds either, so the check is one line.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np

from .. import _lib as L
from ..program import Net, ProgramBuilder, fold_bn


@dataclass(frozen=True)
class PoseC3DSpec:
    in_channels: int = 17
    base_channels: int = 32
    stage_blocks: tuple = (4, 6, 3)
    inflate: tuple = (0, 1, 1)
    spatial_strides: tuple = (2, 2, 2)
    temporal_strides: tuple = (1, 1, 1)      # per stage, on block 0's conv2 and projection (UNPINNED: see the module docstring)
    conv1_kernel: int = 7
    num_classes: int = 81
    clip_len: int = 48          # T
    height: int = 64
    width: int = 64

    @property
    def c_pad(self) -> int:
        return (self.in_channels + 3) // 4 * 4

    @property
    def feat_channels(self) -> int:
        return self.base_channels * 2 ** (len(self.stage_blocks) - 1) * 4

    @property
    def n_front(self) -> int:
        """the leading stages without a temporal convolution: per-frame work, like conv1 and the pool"""
        n = 0
        while n < len(self.stage_blocks) and not self.inflate[n]:
            n += 1
        return n


def _bn(sh, name, c):
    for s in ("weight", "bias", "running_mean", "running_var"):
        sh[f"{name}.bn.{s}"] = (c,)


def posec3d_param_shapes(spec: PoseC3DSpec = PoseC3DSpec()) -> dict:
    """the checkpoint keys this model reads (BatchNorm's num_batches_tracked is not among them), in module order"""
    sh = {}
    k = spec.conv1_kernel
    sh["backbone.conv1.conv.weight"] = (spec.base_channels, spec.in_channels, 1, k, k)
    _bn(sh, "backbone.conv1", spec.base_channels)
    inpl = spec.base_channels
    for s, blocks in enumerate(spec.stage_blocks):
        planes = spec.base_channels * 2 ** s
        for b in range(blocks):
            q = f"backbone.layer{s + 1}.{b}."
            sh[q + "conv1.conv.weight"] = (planes, inpl, 3 if spec.inflate[s] else 1, 1, 1)
            _bn(sh, q + "conv1", planes)
            sh[q + "conv2.conv.weight"] = (planes, planes, 1, 3, 3)
            _bn(sh, q + "conv2", planes)
            sh[q + "conv3.conv.weight"] = (planes * 4, planes, 1, 1, 1)
            _bn(sh, q + "conv3", planes * 4)
            if b == 0:
                sh[q + "downsample.conv.weight"] = (planes * 4, inpl, 1, 1, 1)
                _bn(sh, q + "downsample", planes * 4)
            inpl = planes * 4
    sh["cls_head.fc_cls.weight"], sh["cls_head.fc_cls.bias"] = (spec.num_classes, inpl), (spec.num_classes,)
    return sh


def synth_params(shapes: dict, seed: int = 0) -> dict:
    """Seeded parameters for POSEPIPE_SYNTHETIC_WEIGHTS=1: He-normal convolutions, BatchNorm as models/synth.py (a small gamma on every
    block's last BatchNorm keeps the residual sum O(1)), and an fc_cls whose logits are O(1) on O(1) features, so that the soft-max
    neither saturates nor flattens."""
    rng = np.random.default_rng(seed)
    p = {}
    for name, shp in shapes.items():
        if name.endswith("running_var"):
            a = rng.uniform(0.5, 1.5, shp)
        elif name.endswith("running_mean"):
            a = rng.normal(0, 0.1, shp)
        elif name.endswith(".bn.weight"):
            a = rng.uniform(0.1, 0.3, shp) if ".conv3." in name else rng.uniform(0.5, 1.0, shp)
        elif name == "cls_head.fc_cls.weight":
            a = rng.normal(0, 4.0 / np.sqrt(shp[1]), shp)
        elif name == "cls_head.fc_cls.bias":
            a = rng.normal(0, 0.5, shp)
        elif len(shp) == 1:
            a = rng.normal(0, 0.1, shp)
        else:
            a = rng.normal(0, np.sqrt(2.0 / int(np.prod(shp[1:]))), shp)
        p[name] = a.astype(np.float32)
    return p


def checked(sd: dict, shapes: dict) -> dict:
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise KeyError(f"PoseC3D: missing parameters {missing[:5]}{'...' if len(missing) > 5 else ''}")
    wrong = [(k, tuple(np.shape(sd[k])), shapes[k]) for k in shapes if tuple(np.shape(sd[k])) != tuple(shapes[k])]
    if wrong:
        raise ValueError(f"PoseC3D: parameter shapes differ (key, found, expected): {wrong[:5]}{'...' if len(wrong) > 5 else ''}")
    return {k: np.asarray(sd[k], np.float32) for k in shapes}


def _conv(pb, sd, x, name, *, temporal=False, **kw):
    """ConvModule `name` (conv + BatchNorm folded) as a 2D convolution of the builder's view"""
    w5 = sd[name + ".conv.weight"]
    w5, b = fold_bn(w5, None, *(sd[f"{name}.bn.{s}"] for s in ("weight", "bias", "running_mean", "running_var")))
    if temporal:
        assert w5.shape[3:] == (1, 1), (name, w5.shape)
        w2 = w5[:, :, :, 0, :]                         # [cout][cin][kt][1]: rows are time steps
        kw.setdefault("pad", (w5.shape[2] // 2, 0))
    else:
        assert w5.shape[2] == 1, (name, w5.shape)
        w2 = w5[:, :, 0]
    return pb.conv(x, w2, b, name=name, **kw)


def build_programs(spec: PoseC3DSpec, sd: dict):
    """-> (programs {"front", "frame", "clip"}, steps).  steps, in order: ("run", program, first op, last op, samples per clip), ("copy",
    (program, buffer name) destination, (program, buffer name) source, floats per clip) and ("subsample", destination, source, T, ts):
    every ts-th of a clip's T frames; the last N_HEAD_STEPS of them are the head.
    front: "input" [H][W][c_pad] -> "front_out"; frame: "x0" (= front_out) -> "pooled" [1][1][C]; clip: "cpool" [T][1][C] -> "logits"."""
    sd = checked(sd, posec3d_param_shapes(spec))
    R = L.PP_RELU_LAST
    T = spec.clip_len
    pa, pf, pc = ProgramBuilder(), ProgramBuilder(), ProgramBuilder()
    assert all(t == 1 for t in spec.temporal_strides[:spec.n_front]) and all(t >= 1 for t in spec.temporal_strides), spec.temporal_strides
    steps = []

    def block(pb, x, y, q, stride, first, out):
        """conv2, the projection shortcut (right in front of conv3, as models/faster_rcnn.resnet50_body) and conv3 of one bottleneck"""
        y = _conv(pb, sd, y, q + "conv2", stride=stride, pad=1, relu=R)
        idn = _conv(pb, sd, x, q + "downsample", stride=stride) if first else x
        return _conv(pb, sd, y, q + "conv3", relu=R, res1=idn, out=out)

    # ---- front: per-frame work only
    x = pa.buf(spec.height, spec.width, spec.c_pad, name="input")
    x = _conv(pa, sd, x, "backbone.conv1", pad=spec.conv1_kernel // 2, relu=R)
    x = pa.maxpool(x, 3, 1, 1, name="backbone.maxpool")
    for s in range(spec.n_front):
        for b in range(spec.stage_blocks[s]):
            q = f"backbone.layer{s + 1}.{b}."
            x = block(pa, x, _conv(pa, sd, x, q + "conv1", relu=R), q, spec.spatial_strides[s] if b == 0 else 1, b == 0, None)
    pa.mark_output(x, "front_out")

    # ---- the later stages: frame program and clip program, block by block.  T: the time steps of a clip at this depth
    h, w, c = pa.dims(x)
    xf, xf_name = pf.buf(h, w, c, name="x0"), "x0"
    for s in range(spec.n_front, len(spec.stage_blocks)):
        planes = spec.base_channels * 2 ** s
        stride, ts = spec.spatial_strides[s], spec.temporal_strides[s]
        h, w, _ = pf.dims(xf)
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        pong = [pf.buf(ho, wo, planes * 4, name=f"x{s}_{k}") for k in range(2)]      # block outputs, alternating
        for b in range(spec.stage_blocks[s]):
            q = f"backbone.layer{s + 1}.{b}."
            hi, wi, ci = pf.dims(xf)
            strided = b == 0 and ts > 1
            f0 = len(pf.vops)
            if spec.inflate[s]:
                tag = f"{s}{'a' if b == 0 else 'b'}"          # block 0 sees the previous stage's map size, the others this stage's
                if "cx" + tag not in pc.named:
                    pc.buf(T, hi * wi, ci, name="cx" + tag)
                    pc.buf(T, hi * wi, planes, name="ct" + tag)
                    pf.buf(hi, wi, planes, name="t" + tag)
                i0 = len(pc.vops)
                _conv(pc, sd, pc.named["cx" + tag], q + "conv1", temporal=True, relu=R, out=pc.named["ct" + tag])
                steps += [("copy", ("clip", "cx" + tag), ("frame", xf_name), T * hi * wi * ci), ("run", "clip", i0, i0 + 1, 1),
                          ("copy", ("frame", "t" + tag), ("clip", "ct" + tag), T * hi * wi * planes)]
                y, y_name = pf.named["t" + tag], "t" + tag
            elif strided:                                     # conv1 on every frame, in a range of its own, into a buffer with a name
                y, y_name = _conv(pf, sd, xf, q + "conv1", relu=R, out=pf.buf(hi, wi, planes, name=f"t{s}a")), f"t{s}a"
                steps.append(("run", "frame", f0, len(pf.vops), T))
                f0 = len(pf.vops)
            else:
                y = _conv(pf, sd, xf, q + "conv1", relu=R)
            if strided:
                # Conv3d's temporal stride sits on conv2 and on the projection, both 1 wide in time: they see every ts-th frame.  In the
                # frame view that is a choice of samples: pp_gather_samples of conv1's result and of the block's input
                ys, xs = pf.buf(hi, wi, planes, name=f"ys{s}"), pf.buf(hi, wi, ci, name=f"xs{s}")
                steps += [("subsample", ("frame", f"ys{s}"), ("frame", y_name), T, ts), ("subsample", ("frame", f"xs{s}"), ("frame", xf_name), T, ts)]
                y, xf, T = ys, xs, (T - 1) // ts + 1
            xf = block(pf, xf, y, q, stride if b == 0 else 1, b == 0, pong[b % 2])
            xf_name = f"x{s}_{b % 2}"
            steps.append(("run", "frame", f0, len(pf.vops), T))

    # ---- head
    h, w, c = pf.dims(xf)
    f0 = len(pf.vops)
    pf.mark_output(pf.avgpool(xf, h, w, 1, name="cls_head.pool_hw"), "pooled")
    i0 = len(pc.vops)
    g = pc.avgpool(pc.buf(T, 1, c, name="cpool"), T, 1, 1, name="cls_head.pool_t")
    n_pad = (spec.num_classes + 3) // 4 * 4
    fw, fb = np.zeros((n_pad, c, 1, 1), np.float32), np.zeros(n_pad, np.float32)
    fw[:spec.num_classes, :, 0, 0], fb[:spec.num_classes] = sd["cls_head.fc_cls.weight"], sd["cls_head.fc_cls.bias"]
    pc.conv(g, fw, fb, out=pc.buf(1, 1, n_pad, name="logits"), name="cls_head.fc_cls")
    steps += [("run", "frame", f0, len(pf.vops), T), ("copy", ("clip", "cpool"), ("frame", "pooled"), T * c), ("run", "clip", i0, len(pc.vops), 1)]
    return {"front": pa.build(), "frame": pf.build(), "clip": pc.build()}, steps


N_HEAD_STEPS = 3
# activation budget of a pass: the sweep of tools/posec3d_timing.py (DESIGN_LOG.md 5x) rises steeply up to 4 clips per pass (727 MiB
# at the default spec) and slowly beyond (20 clips: 3.6 GB for 16 - 34 % more windows/s); 768 MiB keeps the buffers in the hundreds of MB
PASS_BUDGET_BYTES = 768 << 20


def front_bytes_per_frame(progs) -> int:
    """device bytes of the front program's activation buffers per sample of its batch (2 n distinct maps with de-duplication, the
    frames of a pass without): outside activation_bytes_per_clip and PASS_BUDGET_BYTES"""
    return sum(h * w * c for h, w, c in progs["front"].bufs) * 4


def activation_bytes_per_clip(spec: PoseC3DSpec, progs=None) -> int:
    """device bytes the frame and clip programs' activation buffers take per clip of a pass (the front program excluded)"""
    if progs is None:
        progs = build_programs(spec, synth_params(posec3d_param_shapes(spec)))[0]
    per = lambda p: sum(h * w * c for h, w, c in p.bufs) * 4                       # noqa: E731
    return per(progs["frame"]) * spec.clip_len + per(progs["clip"])


def clips_per_pass(spec: PoseC3DSpec, n_clips: int, progs=None, budget_bytes: int = PASS_BUDGET_BYTES) -> int:
    """how many clips one pass takes so that the two programs' activation buffers stay within `budget_bytes`"""
    return int(max(1, min(n_clips, budget_bytes // activation_bytes_per_clip(spec, progs))))


class PoseC3DNet:
    """The three resident programs on one context and the schedule between them.  A pass is `n` clips (<= max_clips) whose frames, in
    clip order, are the samples of the frame program."""

    def __init__(self, ctx, spec: PoseC3DSpec, sd: dict, numerics=None, max_clips: int = 1, front_batch: int | None = None, programs=None):
        """programs: what build_programs(spec, sd) returned, where the caller has built it already"""
        self.ctx, self.spec = ctx, spec
        self.progs, self.steps = build_programs(spec, sd) if programs is None else programs
        self.max_clips = int(max_clips)
        T = spec.clip_len
        self.front_batch = int(front_batch or self.max_clips * T)
        self.nets = {"front": Net(ctx, self.progs["front"], max_batch=self.front_batch, numerics=numerics),
                     "frame": Net(ctx, self.progs["frame"], max_batch=self.max_clips * T, numerics=numerics),
                     "clip": Net(ctx, self.progs["clip"], max_batch=self.max_clips, numerics=numerics)}
        self.numerics = self.nets["frame"].numerics
        self._plan, self._idx = [], []
        for st in self.steps:
            if st[0] == "run":
                self._plan.append(st)
                continue
            (dn, db), (sn, sb) = st[1], st[2]
            dptr, dbytes, _ = self.nets[dn].buffer(db)
            sptr, sbytes, _ = self.nets[sn].buffer(sb)
            if st[0] == "copy":
                assert st[3] * 4 % dbytes == 0 and st[3] * 4 % sbytes == 0, st       # whole samples on both sides
                self._plan.append(("copy", dptr, sptr, st[3] * 4))
            else:                                                                    # every ts-th frame of each clip
                t_in, ts = st[3], st[4]
                t_out = (t_in - 1) // ts + 1
                idx = (np.arange(self.max_clips)[:, None] * t_in + np.arange(t_out)[None, :] * ts).astype(np.int32).reshape(-1)
                assert dbytes == sbytes and idx.max() < self.max_clips * t_in
                self._idx.append(ctx.malloc(idx.nbytes))
                ctx.h2d(self._idx[-1], idx)
                self._plan.append(("subsample", dptr, sptr, self._idx[-1], t_in, t_out, sbytes // 4))
        self.input_ptr, self.input_bytes, _ = self.nets["front"].buffer("input")
        self.front_out_ptr, self.front_out_bytes, _ = self.nets["front"].buffer("front_out")
        self.x0_ptr = self.nets["frame"].buffer("x0")[0]

    @property
    def flops_per_clip(self) -> float:
        runs = sum(sum(self.progs[st[1]].op_flops[st[2]:st[3]]) * st[4] for st in self.steps if st[0] == "run")
        return self.progs["front"].flops * self.spec.clip_len + runs

    def run_front(self, n_frames: int):
        self.nets["front"].run(n_frames)

    def front_to_trunk(self, n_clips: int):
        """front_out of the pass's frames (already in clip order) -> the frame program's input"""
        self.ctx.d2d(self.x0_ptr, self.front_out_ptr, n_clips * self.spec.clip_len * self.front_out_bytes)

    def run_trunk(self, n_clips: int, head: bool = True, body: bool = True):
        """"x0" holds the front stage's output for n_clips clips; queues everything up to "logits" on the context's stream"""
        assert 0 < n_clips <= self.max_clips
        n_body = len(self._plan) - N_HEAD_STEPS
        for st in self._plan[0 if body else n_body: len(self._plan) if head else n_body]:
            if st[0] == "run":
                self.nets[st[1]].run(n_clips * st[4], st[2], st[3])
            elif st[0] == "copy":
                self.ctx.d2d(st[1], st[2], n_clips * st[3])
            else:
                L.check(self.ctx.lib.pp_gather_samples(self.ctx.handle, L.ptr(st[2]), n_clips * st[4], L.ptr(st[3]), n_clips * st[5], st[6],
                                                       L.ptr(st[1])), "pp_gather_samples")

    def read_logits(self, n_clips: int) -> np.ndarray:
        return self.nets["clip"].read("logits", n_clips).reshape(n_clips, -1)[:, :self.spec.num_classes].copy()

    def forward(self, maps: np.ndarray) -> np.ndarray:
        """Host convenience: maps [n_clips][T][H][W][c_pad] float32 -> logits [n_clips][num_classes], the plain form (the front stage
        runs on every frame)"""
        s = self.spec
        maps = np.ascontiguousarray(maps, np.float32)
        assert maps.shape[1:] == (s.clip_len, s.height, s.width, s.c_pad), maps.shape
        out = np.empty((maps.shape[0], s.num_classes), np.float32)
        for c0 in range(0, maps.shape[0], self.max_clips):
            n = min(self.max_clips, maps.shape[0] - c0)
            frames = maps[c0:c0 + n].reshape(n * s.clip_len, s.height, s.width, s.c_pad)
            for f0 in range(0, len(frames), self.front_batch):
                m = min(self.front_batch, len(frames) - f0)
                self.ctx.h2d(self.input_ptr, frames[f0:f0 + m])
                self.run_front(m)
                self.ctx.d2d(self.x0_ptr + f0 * self.front_out_bytes, self.front_out_ptr, m * self.front_out_bytes)
            self.run_trunk(n)
            out[c0:c0 + n] = self.read_logits(n)
        return out

    def close(self):
        for p in getattr(self, "_idx", []):
            self.ctx.free(p)
        self._idx = []
        for net in getattr(self, "nets", {}).values():
            net.close()
        self.nets = {}


def replace(spec: PoseC3DSpec, **kw) -> PoseC3DSpec:
    return dataclasses.replace(spec, **kw)
