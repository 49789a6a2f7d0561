"""HRNetv2-W18 top-down hand network (256x256 input, 21 joints) as a pp_net layer program.

The model behind the `HRNet_dark` / `HRNet_udp` methods of the reference's hand stage (pose_pipeline/wrappers/
hand_estimation.py:31-42: mmpose's rhd2d `hrnetv2_w18 ... dark` and onehand10k `hrnetv2_w18 ... udp` configs).  Those
configs are NOT in the reference tree: this module is an UNPINNED RESTATEMENT of the published mmpose architecture, like
ViTPose (models/vitpose.py) and YOLOX here.  Parameter names follow mmpose 0.x (`backbone.*`,
`keypoint_head.final_layer.{0,1,3}.*`), the era of the checkpoints whose URLs the reference names.

What separates it from the pose HRNet of models/hrnet.py:
  * widths (18, 36, 72, 144); the last module has multiscale_output=True, so all four fuse outputs exist;
  * every coarse-to-fine fuse branch is conv1x1 + BN + Upsample(2^(j-i), mode='bilinear', align_corners=False).  The terms
    are summed in mmpose's j order, then ReLU: one PP_OP_BILINEAR_ADD pass per fuse output;
  * head (TopdownHeatmapSimpleHead with input_transform='resize_concat', num_conv_layers=2): the four outputs are bilinearly
    resized (align_corners=False) to 64x64 and concatenated in branch order (18 + 36 + 72 + 144 = 270 channels), then
    final_layer.0 conv1x1 270 -> 270 WITH bias, final_layer.1 BN, ReLU, final_layer.3 conv1x1 270 -> 21 with bias.
    Here the last module's first fuse pass writes its result straight into channels [0, 20) of the concatenation buffer (a
    resize to the same size is the identity) and three more PP_OP_BILINEAR_ADD passes fill the other slices.

Activation buffers need channel counts that are multiples of 4: the 18-wide branch is stored with 20 channels, the
concatenation with 272 (18 + 2 zeros, 36, 72, 144) and the head's hidden layer with 272, by zero weights and biases, as the
VideoPose3D input is.  A padded channel holds exact zeros everywhere, and a zero weight times a zero activation leaves every
float32 accumulation chain unchanged, so the results are those of the unpadded network bit for bit (tests/hand_ref.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import _lib as L
from ..program import Program, fold_bn
from .hrnet import _HR, _conv_bn, hrnet_backbone_shapes


@dataclass(frozen=True)
class HRNetV2Spec:
    width: int = 18
    num_joints: int = 21
    in_h: int = 256
    in_w: int = 256
    stages: tuple = ((1, 2), (4, 3), (3, 4))
    blocks_per_branch: int = 4

    @property
    def channels(self):
        return tuple(self.width * (2 ** i) for i in range(4))

    @property
    def heatmap_hw(self):
        return self.in_h // 4, self.in_w // 4

    @property
    def concat_channels(self):
        return sum(self.channels)


def hrnetv2_w18_256x256(num_joints=21):
    return HRNetV2Spec(18, num_joints, 256, 256)


def _pad4(c):
    return (c + 3) // 4 * 4


def concat_layout(spec):
    """(offset of each branch's slice in the concatenation buffer, buffer channels): slices start at multiples of 4"""
    offs, o = [], 0
    for c in spec.channels:
        offs.append(o)
        o += _pad4(c)
    return offs, o


def bilinear_op_count(spec):
    """PP_OP_BILINEAR_ADD ops of the program, from the stage table: one per fuse output that has a coarser branch (all but the
    last of every module; every module has all its outputs), plus one resize per coarser branch in front of the head"""
    return sum(n_mod * (n_br - 1) for n_mod, n_br in spec.stages) + (spec.stages[-1][1] - 1)


def hrnetv2_param_shapes(spec: HRNetV2Spec) -> dict:
    assert len(spec.stages) == 3 and spec.stages[-1][1] == 4, "the resize_concat head takes the four branches of stage 4"
    sh = hrnet_backbone_shapes(spec, multiscale_output=True)
    cc = spec.concat_channels
    H = "keypoint_head.final_layer."
    _conv_bn(sh, H + "0", H + "1", cc, cc, 1)
    sh[H + "0.bias"] = (cc,)
    sh[H + "3.weight"] = (spec.num_joints, cc, 1, 1)
    sh[H + "3.bias"] = (spec.num_joints,)
    return sh


class _HRv2(_HR):
    multiscale_output = True
    bilinear_fuse = True

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.head_in = None       # the concatenation buffer, once the head is being assembled

    def cb(self, x, conv, bn, *, stride=1, pad=1, relu=L.PP_RELU_NONE, **kw):
        sd = self.sd
        w, b = fold_bn(sd[conv + ".weight"], None, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"],
                       sd[bn + ".running_var"])
        cout = w.shape[0]
        if cout % 4:        # zero output channels up to a multiple of 4 (the readers' weights for them are zero as well)
            w = np.concatenate([w, np.zeros((_pad4(cout) - cout,) + w.shape[1:], np.float32)])
            b = np.concatenate([b, np.zeros(_pad4(cout) - cout, np.float32)])
        return self.pb.conv(x, w, b, stride=stride, pad=pad, relu=relu, name=conv, **kw)

    def fuse_up(self, ups, acc, name):
        last0 = name == self._last_fuse0
        return self.pb.bilinear_add(ups[0][0], up_log2=ups[0][1], res1=acc, relu=L.PP_RELU_LAST, more=ups[1:], name=name,
                                    out=self.head_in if last0 else None)

    def build(self) -> Program:
        spec, pb, sd = self.spec, self.pb, self.sd
        hh, hw = spec.heatmap_hw
        offs, cbuf = concat_layout(spec)
        # branch 0 of the last module is already at heat-map resolution: its fuse pass writes channels [0, 20) of the
        # concatenation directly (bilinear resizing to the same size is the identity)
        self.head_in = pb.buf(hh, hw, cbuf)
        self._last_fuse0 = f"backbone.stage{len(spec.stages) + 1}.{spec.stages[-1][0] - 1}.fuse_layers.0.up"
        ys = self.backbone()
        assert ys[0] == self.head_in and len(ys) == 4
        for i in range(1, 4):
            pb.bilinear_add(ys[i], up_log2=i, out=self.head_in, out_c_off=offs[i], name=f"keypoint_head.resize.{i}")
        # final_layer.0 (+ bias) / .1 BN / ReLU on the padded channel layout: input channel k of the checkpoint is buffer
        # channel k + (the padding in front of its branch)
        H = "keypoint_head.final_layer."
        cc = spec.concat_channels
        w0, b0 = fold_bn(sd[H + "0.weight"], sd[H + "0.bias"], sd[H + "1.weight"], sd[H + "1.bias"], sd[H + "1.running_mean"],
                         sd[H + "1.running_var"])
        src = np.concatenate([offs[i] + np.arange(c) for i, c in enumerate(spec.channels)])
        hid = _pad4(cc)
        wp = np.zeros((hid, cbuf, 1, 1), np.float32)
        wp[:cc, src] = w0
        bp = np.zeros(hid, np.float32)
        bp[:cc] = b0
        y = pb.conv(self.head_in, wp, bp, pad=0, relu=L.PP_RELU_LAST, name=H + "0")
        out = pb.buf(hh, hw, spec.num_joints, name="output")
        pb.conv(y, sd[H + "3.weight"], sd[H + "3.bias"], pad=0, out=out, out_nchw=True, name=H + "3")
        return pb.build()


def build_hrnetv2_program(spec: HRNetV2Spec, state_dict: dict) -> Program:
    """state_dict: name -> numpy array in torch layouts (see hrnetv2_param_shapes)."""
    shapes = hrnetv2_param_shapes(spec)
    for k, shp in shapes.items():
        if k not in state_dict:
            raise KeyError(f"missing parameter {k}")
        if tuple(state_dict[k].shape) != tuple(shp):
            raise ValueError(f"{k}: shape {state_dict[k].shape} != {shp}")
    return _HRv2(spec, state_dict).build()
