"""HRFormer-B top-down pose network (384x288 input, 17 joints) as a pp_net layer program.

The model behind `method="HRFormer_COCO"` of the reference's top-down wrapper (pose_pipeline/wrappers/mmpose.py:37-40,
`TopDownMethodLookup` row 3 "MMPoseHrformerCoco").  Its hyper-parameters are those of the config the reference vendors
(3rdparty/mmpose/config/top_down/hrformer_base_coco_384x288.py; tests/golden/arch_config_hrformer.json holds the values and
tests/test_hrformer.py compares the spec with them).  The module INTERNALS are not in the reference tree: what follows is an
UNPINNED RESTATEMENT of mmpose 0.x `backbones/hrformer.py`, as models/hrnetv2.py and models/vitpose.py restate theirs, and the
checkpoint key names are assumed (mmpose 0.x, the era of `hrformer_base_coco_384x288-ecf0758d_20220316.pth`).

Architecture
  * stem, layer1 (2 Bottlenecks 64 -> 256) and the transitions (3x3 conv + BN + ReLU, stride 2 for a new branch): mmpose HRNet,
    built by the code of models/hrnet.py;
  * stages 2 / 3 / 4: 1 / 4 / 2 modules of 2 / 3 / 4 branches, channels (78, 156, 312, 624), heads (2, 4, 8, 16) -- head dim 39
    everywhere --, 2 HRFormerBlocks per branch and module; the last module fuses to branch 0 only;
  * HRFormerBlock on an NHWC map: x = x + Attn(LN1(x)); x = x + FFN(LN2(x)); LayerNorm over the channels, eps 1e-6;
      Attn  7x7 windows on the map zero-padded (AFTER LN1, BEFORE the qkv Linear) to multiples of 7, pad // 2 in front; qkv Linear with
            bias, q * hd^-0.5, + relative-position bias table[(yi - yj + 6) * 13 + (xi - xj + 6)][head], softmax, @ v, proj Linear,
            crop.  Padded tokens take part as keys with k = b_k, v = b_v;
      FFN   1x1 conv C -> 4C (bias) + BN + GELU, depthwise 3x3 (bias) + BN + GELU, 1x1 conv 4C -> C (bias) + BN + GELU (erf form);
  * fuse layers: j > i  1x1 conv + BN, bilinear x 2^(j-i) (align_corners=False);  j < i  i - j steps of depthwise 3x3 s2 + BN,
    1x1 conv + BN, a ReLU after every step but the last, channels change in the last step; summed in mmpose's j order, then ReLU;
  * head: one 1x1 conv 78 -> 17.

Program form (one HRFormerBlock = 9 ops):
    LN1 (PP_OP_LAYERNORM) -> qkv 1x1 conv on the UN-padded map (PP_OP_CONV, C -> 3 C_buf) -> PP_OP_WINDOW_ATTN (window padding, the
    bias substitution for padded tokens, softmax, @ v) -> proj 1x1 conv with the residual in its epilogue -> LN2 -> fc1 (BN folded,
    NO activation) -> PP_OP_DWCONV3X3 with GELU on its input (fc1's) and on its output -> fc2 (BN folded, no activation) ->
    PP_OP_GELU_ADD (x + gelu(.)).  GELU therefore lives in the new kernels only; the convolution kernels are untouched.

Activation buffers need channel counts that are multiples of 4: the 78-wide branch is stored with 80 channels (q, k and v each
as 78 + 2 in the 240-wide qkv map) by zero weights and biases, the idiom of models/hrnetv2.py.  A padded channel holds exact
zeros everywhere: LayerNorm and the attention op write zeros there, gelu(0) = 0, and zero weights leave the others' sums alone.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import _lib as L
from ..program import Program, fold_bn
from .hrnet import _HR, _conv_bn


@dataclass(frozen=True)
class HRFormerSpec:
    channels: tuple = (78, 156, 312, 624)
    heads: tuple = (2, 4, 8, 16)
    mlp_ratios: tuple = (4, 4, 4, 4)
    windows: tuple = (7, 7, 7, 7)
    num_joints: int = 17
    in_h: int = 384
    in_w: int = 288
    stages: tuple = ((1, 2), (4, 3), (2, 4))     # (modules, branches) of stages 2 .. 4
    blocks_per_branch: int = 2
    layer1_blocks: int = 2

    @property
    def heatmap_hw(self):
        return self.in_h // 4, self.in_w // 4


def hrformer_base_384x288(num_joints=17):
    return HRFormerSpec(num_joints=num_joints)


def _pad4(c):
    return (c + 3) // 4 * 4


# ---- parameter inventory ---------------------------------------------------------------------------------------------------------
def _bn(sh, name, c):
    for s in ("weight", "bias", "running_mean", "running_var"):
        sh[f"{name}.{s}"] = (c,)


def hrformer_param_shapes(spec: HRFormerSpec) -> dict:
    """name -> shape of every parameter the program reads (mmpose 0.x key names, ASSUMED: no checkpoint is at hand).  A checkpoint's
    other keys -- `relative_position_index` buffers, `num_batches_tracked`, `ffn.layers.N.*` aliases -- are ignored."""
    sh: dict = {}
    B = "backbone."
    _conv_bn(sh, B + "conv1", B + "bn1", 64, 3, 3)
    _conv_bn(sh, B + "conv2", B + "bn2", 64, 64, 3)
    for i in range(spec.layer1_blocks):
        p = f"{B}layer1.{i}."
        cin = 64 if i == 0 else 256
        _conv_bn(sh, p + "conv1", p + "bn1", 64, cin, 1)
        _conv_bn(sh, p + "conv2", p + "bn2", 64, 64, 3)
        _conv_bn(sh, p + "conv3", p + "bn3", 256, 64, 1)
        if i == 0:
            _conv_bn(sh, p + "downsample.0", p + "downsample.1", 256, 64, 1)
    ch = spec.channels
    pre = [256]
    for si, (n_mod, n_br) in enumerate(spec.stages):
        cur = list(ch[:n_br])
        t = f"{B}transition{si + 1}."
        for i in range(n_br):
            if i < len(pre):
                if pre[i] != cur[i]:
                    _conv_bn(sh, f"{t}{i}.0", f"{t}{i}.1", cur[i], pre[i], 3)
            else:
                for j in range(i + 1 - len(pre)):
                    cin = pre[-1]
                    cout = cur[i] if j == i - len(pre) else cin
                    _conv_bn(sh, f"{t}{i}.{j}.0", f"{t}{i}.{j}.1", cout, cin, 3)
        for m in range(n_mod):
            mp = f"{B}stage{si + 2}.{m}."
            for b in range(n_br):
                c, hid = cur[b], cur[b] * spec.mlp_ratios[b]
                for k in range(spec.blocks_per_branch):
                    p = f"{mp}branches.{b}.{k}."
                    for ln in ("norm1", "norm2"):
                        sh[p + ln + ".weight"] = (c,)
                        sh[p + ln + ".bias"] = (c,)
                    a = p + "attn.attn."
                    sh[a + "qkv.weight"] = (3 * c, c)
                    sh[a + "qkv.bias"] = (3 * c,)
                    sh[a + "proj.weight"] = (c, c)
                    sh[a + "proj.bias"] = (c,)
                    sh[a + "relative_position_bias_table"] = ((2 * spec.windows[b] - 1) ** 2, spec.heads[b])
                    f = p + "ffn."
                    sh[f + "fc1.weight"] = (hid, c, 1, 1)
                    sh[f + "fc1.bias"] = (hid,)
                    _bn(sh, f + "norm1", hid)
                    sh[f + "dw3x3.weight"] = (hid, 1, 3, 3)
                    sh[f + "dw3x3.bias"] = (hid,)
                    _bn(sh, f + "norm2", hid)
                    sh[f + "fc2.weight"] = (c, hid, 1, 1)
                    sh[f + "fc2.bias"] = (c,)
                    _bn(sh, f + "norm3", c)
            last = (si == len(spec.stages) - 1) and (m == n_mod - 1)
            for i in range(1 if last else n_br):
                for j in range(n_br):
                    f = f"{mp}fuse_layers.{i}.{j}."
                    if j > i:
                        _conv_bn(sh, f + "0", f + "1", cur[i], cur[j], 1)
                    elif j < i:
                        for k in range(i - j):
                            cout = cur[i] if k == i - j - 1 else cur[j]
                            sh[f"{f}{k}.0.weight"] = (cur[j], 1, 3, 3)
                            _bn(sh, f"{f}{k}.1", cur[j])
                            _conv_bn(sh, f"{f}{k}.2", f"{f}{k}.3", cout, cur[j], 1)
        pre = cur
    sh["keypoint_head.final_layer.weight"] = (spec.num_joints, ch[0], 1, 1)
    sh["keypoint_head.final_layer.bias"] = (spec.num_joints,)
    return sh


def param_count(shapes: dict) -> int:
    """learnable parameters: everything but the BatchNorm running statistics"""
    return int(sum(int(np.prod(s)) for k, s in shapes.items() if not k.endswith(("running_mean", "running_var"))))


def synth_params(spec: HRFormerSpec, seed: int = 0, smooth: bool = False) -> dict:
    """Seeded synthetic parameters (models/synth.py) with what the generic initialisers do not know about a transformer block:
    LayerNorm gains around one (not all ones), small NON-zero asymmetric relative-position tables, attention and FFN weights of
    the scale of a trained block; the BN in front of the last GELU of every FFN is damped so that ~40 residual blocks keep an O(1)
    stream.  smooth: `smooth_state_dict` for the convolutions (positive averaging kernels: single-peaked heat-maps)."""
    from . import synth
    shapes = hrformer_param_shapes(spec)
    sd = (synth.smooth_state_dict if smooth else synth.synth_state_dict)(shapes, seed)
    rng = np.random.default_rng(seed + 7919)
    for k, shp in shapes.items():
        if ".branches." not in k:
            continue
        if k.endswith(("norm1.weight", "norm2.weight")) and ".ffn." not in k:            # LayerNorm gain
            sd[k] = rng.uniform(0.7, 1.3, shp).astype(np.float32)
        elif k.endswith(("norm1.bias", "norm2.bias")) and ".ffn." not in k:
            sd[k] = rng.normal(0, 0.1, shp).astype(np.float32)
        elif k.endswith("relative_position_bias_table"):
            sd[k] = rng.normal(0, 0.5, shp).astype(np.float32)
        elif k.endswith(("qkv.weight", "proj.weight")):
            sd[k] = rng.normal(0, (0.5 if k.endswith("proj.weight") else 1.0) / np.sqrt(shp[1]), shp).astype(np.float32)
        elif k.endswith(("qkv.bias", "proj.bias", "fc1.bias", "dw3x3.bias", "fc2.bias")):
            sd[k] = rng.normal(0, 0.1, shp).astype(np.float32)
        elif smooth and ".ffn." in k and len(shp) > 1:                                   # signed FFN weights: the branch is not a pure smoother
            sd[k] = rng.normal(0, np.sqrt(1.0 / int(np.prod(shp[1:]))), shp).astype(np.float32)
        elif k.endswith("ffn.norm3.weight"):
            sd[k] = rng.uniform(0.1, 0.3, shp).astype(np.float32)
    if smooth:
        for k in sd:
            if k.endswith(("proj.weight", "ffn.norm3.weight")):
                sd[k] = (sd[k] * 0.2).astype(np.float32)       # damp both residual branches: the convolutional path keeps the blob
    return sd


# ---- program builder ---------------------------------------------------------------------------------------------------------------
def _pad_out(w, b, c_pad):
    """zero output channels up to c_pad (the readers' weights for them are zero as well)"""
    cout = w.shape[0]
    if cout == c_pad:
        return w, b
    w = np.concatenate([w, np.zeros((c_pad - cout,) + w.shape[1:], np.float32)])
    b = np.concatenate([np.zeros(cout, np.float32) if b is None else b, np.zeros(c_pad - cout, np.float32)])
    return w, b


class _HRFormer(_HR):
    bilinear_fuse = True

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.layer1_blocks = spec.layer1_blocks

    def _folded(self, conv, bn):
        sd = self.sd
        return fold_bn(sd[conv + ".weight"], sd.get(conv + ".bias"), sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"],
                       sd[bn + ".running_var"])

    def cb(self, x, conv, bn, *, stride=1, pad=1, relu=L.PP_RELU_NONE, **kw):
        w, b = self._folded(conv, bn)
        w, b = _pad_out(w, b, _pad4(w.shape[0]))
        return self.pb.conv(x, w, b, stride=stride, pad=pad, relu=relu, name=conv, **kw)

    def branch_block(self, x, p, branch):
        spec, pb, sd = self.spec, self.pb, self.sd
        c, heads = spec.channels[branch], spec.heads[branch]
        cb = _pad4(c)
        a = p + "attn.attn."
        # x = x + Attn(LN1(x))
        t = pb.layernorm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps=1e-6, name=p + "norm1")
        wq = np.zeros((3, cb, c), np.float32)
        wq[:, :c] = sd[a + "qkv.weight"].reshape(3, c, c)
        bq = np.zeros((3, cb), np.float32)
        bq[:, :c] = sd[a + "qkv.bias"].reshape(3, c)
        qkv = pb.conv(t, wq.reshape(3 * cb, c, 1, 1), bq.reshape(-1), pad=0, name=a + "qkv")
        att = pb.window_attention(qkv, sd[a + "relative_position_bias_table"], sd[a + "qkv.bias"], c_real=c, heads=heads,
                                  window=spec.windows[branch], name=a + "window")
        wp, bp = _pad_out(sd[a + "proj.weight"].reshape(c, c, 1, 1), sd[a + "proj.bias"], cb)
        x = pb.conv(att, wp, bp, pad=0, res1=x, name=a + "proj")
        # x = x + FFN(LN2(x))
        f = p + "ffn."
        t = pb.layernorm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps=1e-6, name=p + "norm2")
        w1, b1 = self._folded(f + "fc1", f + "norm1")
        assert w1.shape[0] % 4 == 0
        y = pb.conv(t, w1, b1, pad=0, name=f + "fc1")                    # its GELU is the depthwise op's input activation
        wd, bd = self._folded(f + "dw3x3", f + "norm2")
        y = pb.dwconv3x3(y, wd, bd, act=L.PP_ACT_GELU, gelu_in=True, name=f + "dw3x3")
        w2, b2 = self._folded(f + "fc2", f + "norm3")
        w2, b2 = _pad_out(w2, b2, cb)
        y = pb.conv(y, w2, b2, pad=0, name=f + "fc2")                    # its GELU and the residual add: PP_OP_GELU_ADD
        return pb.gelu_add(y, res1=x, name=f + "gelu_add")

    def fuse_down(self, y, f, steps, relu, acc, res2):
        pb = self.pb
        for k in range(steps):
            last = k == steps - 1
            wd, bd = self._folded(f"{f}{k}.0", f"{f}{k}.1")
            y = pb.dwconv3x3(y, wd, bd, stride=2, name=f"{f}{k}.0")
            y = self.cb(y, f"{f}{k}.2", f"{f}{k}.3", pad=0, relu=relu if last else L.PP_RELU_LAST, res1=acc if last else -1,
                        res2=res2 if last else -1)
        return y

    def fuse_up(self, ups, acc, name):
        return self.pb.bilinear_add(ups[0][0], up_log2=ups[0][1], res1=acc, relu=L.PP_RELU_LAST, more=ups[1:], name=name)


def build_hrformer_program(spec: HRFormerSpec, state_dict: dict) -> Program:
    """state_dict: name -> numpy array in torch layouts (see hrformer_param_shapes); keys it does not name are ignored."""
    shapes = hrformer_param_shapes(spec)
    for k, shp in shapes.items():
        if k not in state_dict:
            raise KeyError(f"missing parameter {k}")
        if tuple(state_dict[k].shape) != tuple(shp):
            raise ValueError(f"{k}: shape {state_dict[k].shape} != {shp}")
    return _HRFormer(spec, {k: np.asarray(state_dict[k]) for k in shapes}).build()
