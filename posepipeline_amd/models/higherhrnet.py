"""HigherHRNet-W48 bottom-up pose network (associative embedding) as a pp_net layer program.

The model behind `mmpose_bottom_up` (pose_pipeline/wrappers/mmpose.py:84-121, the VENDORED config it first assigns:
3rdparty/mmpose/config/bottom_up/higherhrnet/coco/higher_hrnet48_coco_512x512.py).  The hyper-parameters are pinned by that
config (`vendored_config`, tests/golden/arch_config_higherhrnet.json); the head's module structure and key names
(`BottomUpHigherResolutionHead`) are an UNPINNED RESTATEMENT of mmpose 0.x, which is not in the reference tree.

  * backbone: the HRNet of models/hrnet.py with multiscale_output=False (keys `backbone.*`): branch 0, `width` channels at 1/4;
  * y0 = final_layers.0(x): conv1x1 width -> 2 * num_joints with bias (channels 0 .. K-1 heat-maps, K .. 2K-1 tags);
  * x = cat(x, y0); deconv_layers.0.0 = ConvTranspose2d(width + 2K, width, 4, 2, 1, bias=False) + BN + ReLU;
    deconv_layers.0.1.{0..3} = BasicBlock(width); y1 = final_layers.1(x): conv1x1 width -> K at 1/2.

How it is expressed with the existing ops (no new pp_op field):
  * the concatenation is one [h][w][width + pad4(2K)] buffer: a 1x1 / stride-1 PP_OP_MAXPOOL copies x into channels [0, width)
    (a max over one value: an exact slice copy), final_layers.0 writes [width, ...) by output channel offset, with zero weights
    and biases for the padding channels so that every channel of the buffer is written;
  * final_layers.0 runs a second time into the NCHW output "output0" (the post-processing reads planes);
  * the transposed convolution is four 2x2 convolutions + PP_OP_DEPTH_TO_SPACE (ProgramBuilder.deconv4x4s2), float32 at the
    net's numerics; the padding channels of its input meet zero weights.
The program is built for one padded input size [hp][wp][4] (bottomup.input_size): "output0" [2K][hp/4][wp/4], "output1" [K][hp/2][wp/2].
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import _lib as L
from ..program import Program, fold_bn
from .hrnet import _HR, _conv_bn, hrnet_backbone_shapes


@dataclass(frozen=True)
class HigherHRNetSpec:
    image_size: int = 512
    width: int = 48
    num_joints: int = 17
    stages: tuple = ((1, 2), (4, 3), (3, 4))
    blocks_per_branch: int = 4
    num_basic_blocks: int = 4          # of the head, behind the transposed convolution

    @property
    def channels(self):
        return tuple(self.width * (2 ** i) for i in range(4))


def higher_hrnet48_coco_512x512():
    return HigherHRNetSpec()


def vendored_config(spec: HigherHRNetSpec) -> dict:
    """The settings of higher_hrnet48_coco_512x512.py this package reads or implies, in the config's own layout (data_cfg,
    backbone.extra, keypoint_head without the loss, test_cfg, the normalisation): what tests/golden/arch_config_higherhrnet.json
    pins.  The fields that are not in the spec are the constants the code is written for (bottomup.TEST_CFG, ops.normalize_lut)."""
    from .. import bottomup
    k, ch = spec.num_joints, spec.channels
    joints = list(range(k))
    extra = {"stage1": dict(num_modules=1, num_branches=1, block="BOTTLENECK", num_blocks=[4], num_channels=[64])}
    for i, (n_mod, n_br) in enumerate(spec.stages):
        extra[f"stage{i + 2}"] = dict(num_modules=n_mod, num_branches=n_br, block="BASIC", num_blocks=[spec.blocks_per_branch] * n_br,
                                      num_channels=list(ch[:n_br]))
    return {
        "data_cfg": dict(image_size=spec.image_size, base_size=256, base_sigma=2, heatmap_size=[128, 256], num_joints=k,
                         dataset_channel=[joints], inference_channel=joints, num_scales=2, scale_aware_sigma=False),
        "backbone": dict(type="HRNet", in_channels=3, extra=extra),
        "keypoint_head": dict(type="BottomUpHigherResolutionHead", in_channels=spec.width, num_joints=k, tag_per_joint=True,
                              extra=dict(final_conv_kernel=1), num_deconv_layers=1, num_deconv_filters=[spec.width],
                              num_deconv_kernels=[4], num_basic_blocks=spec.num_basic_blocks, cat_output=[True],
                              with_ae_loss=[True, False]),
        "test_cfg": dict(num_joints=k, **bottomup.TEST_CFG),
        "normalize": dict(mean=list(bottomup.MEAN), std=list(bottomup.STD)),
    }


def higherhrnet_param_shapes(spec: HigherHRNetSpec) -> dict:
    """every key the program reads"""
    sh = hrnet_backbone_shapes(spec, multiscale_output=False)
    w, k = spec.width, spec.num_joints
    H = "keypoint_head."
    sh[H + "final_layers.0.weight"] = (2 * k, w, 1, 1)
    sh[H + "final_layers.0.bias"] = (2 * k,)
    sh[H + "deconv_layers.0.0.0.weight"] = (w + 2 * k, w, 4, 4)           # ConvTranspose2d layout [cin][cout][4][4]
    for s in ("weight", "bias", "running_mean", "running_var"):
        sh[H + "deconv_layers.0.0.1." + s] = (w,)
    for i in range(spec.num_basic_blocks):
        p = f"{H}deconv_layers.0.1.{i}."
        _conv_bn(sh, p + "conv1", p + "bn1", w, w, 3)
        _conv_bn(sh, p + "conv2", p + "bn2", w, w, 3)
    sh[H + "final_layers.1.weight"] = (k, w, 1, 1)
    sh[H + "final_layers.1.bias"] = (k,)
    return sh


def _pad4(c):
    return (c + 3) // 4 * 4


@dataclass(frozen=True)
class _Sized:
    """what the HRNet builder reads of a spec, for one input size"""
    width: int
    num_joints: int
    in_h: int
    in_w: int
    stages: tuple
    blocks_per_branch: int

    @property
    def channels(self):
        return tuple(self.width * (2 ** i) for i in range(4))


class _HigherHR(_HR):
    num_basic_blocks = 4

    def build(self) -> Program:
        spec, pb, sd = self.spec, self.pb, self.sd
        w, k = spec.width, spec.num_joints
        assert w % 4 == 0
        H = "keypoint_head."
        x = self.backbone()[0]
        h, wd, _ = pb.dims(x)
        w0, b0 = sd[H + "final_layers.0.weight"], sd[H + "final_layers.0.bias"]
        out0 = pb.buf(h, wd, 2 * k, name="output0")
        pb.conv(x, w0, b0, pad=0, out=out0, out_nchw=True, name=H + "final_layers.0")
        # cat(x, y0) in one buffer: the slice copy, then final_layers.0 again by channel offset (padding channels: zeros)
        ypad = _pad4(2 * k)
        cat = pb.buf(h, wd, w + ypad)
        pb.maxpool(x, 1, 1, 0, out=cat, out_c_off=0, name=H + "cat.x")
        wp = np.zeros((ypad, w, 1, 1), np.float32)
        wp[:2 * k] = w0
        bp = np.zeros(ypad, np.float32)
        bp[:2 * k] = b0
        pb.conv(x, wp, bp, pad=0, out=cat, out_c_off=w, name=H + "cat.y0")
        # ConvTranspose2d + BN (folded over the OUTPUT channels, axis 1 of the transposed layout) + ReLU
        D = H + "deconv_layers.0.0."
        wt = np.transpose(sd[D + "0.weight"], (1, 0, 2, 3))                 # [cout][cin][4][4]
        wf, bf = fold_bn(wt, None, sd[D + "1.weight"], sd[D + "1.bias"], sd[D + "1.running_mean"], sd[D + "1.running_var"])
        y = pb.deconv4x4s2(cat, np.transpose(wf, (1, 0, 2, 3)), bf, relu=L.PP_RELU_LAST, name=D + "0")
        for i in range(self.num_basic_blocks):
            y = self.basic(y, f"{H}deconv_layers.0.1.{i}.")
        out1 = pb.buf(2 * h, 2 * wd, k, name="output1")
        pb.conv(y, sd[H + "final_layers.1.weight"], sd[H + "final_layers.1.bias"], pad=0, out=out1, out_nchw=True,
                name=H + "final_layers.1")
        return pb.build()


def build_higherhrnet_program(spec: HigherHRNetSpec, state_dict: dict, in_h: int, in_w: int) -> Program:
    """state_dict: name -> numpy array in torch layouts (see higherhrnet_param_shapes); (in_h, in_w): the padded input size, multiples
    of 64 (BottomUpGetImgSize aligns to 64; the four branches need 32)."""
    assert in_h % 32 == 0 and in_w % 32 == 0, (in_h, in_w)
    shapes = higherhrnet_param_shapes(spec)
    for key, shp in shapes.items():
        if key not in state_dict:
            raise KeyError(f"missing parameter {key}")
        if tuple(state_dict[key].shape) != tuple(shp):
            raise ValueError(f"{key}: shape {state_dict[key].shape} != {shp}")
    b = _HigherHR(_Sized(spec.width, spec.num_joints, int(in_h), int(in_w), spec.stages, spec.blocks_per_branch), state_dict)
    b.num_basic_blocks = spec.num_basic_blocks
    return b.build()
