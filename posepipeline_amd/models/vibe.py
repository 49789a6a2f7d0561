"""VIBE (Kocabas et al., CVPR 2020), the `VIBE_Demo` model behind pose_pipeline/wrappers/vibe.py:25-32
(seqlen 16, n_layers 2, hidden_size 1024, add_linear, use_residual), inference mode.

VIBE, SPIN and smplx are NOT in the reference tree: an UNPINNED restatement of their published sources.  Per frame:

  backbone   SPIN's `hmr.feature_extractor`: torchvision-style ResNet-50 (stride on conv2) -> AvgPool2d(7, 1) -> f [2048].  A layer
             program (resnet50_body + PP_OP_AVGPOOL, as models/reid_r50.py); checkpoint keys `conv1.*`, `bn1.*`, `layer{1..4}.*`
  encoder    nn.GRU(2048, 1024, num_layers 2) over one sequence (ops.Gru, csrc/gru.hip), then y = Linear(1024 -> 2048)(relu(h)) + f;
             keys `encoder.gru.{weight,bias}_{ih,hh}_l{0,1}`, `encoder.linear.*`
  regressor  SPIN's, three iterations from init_pose [144] / init_shape [10] / init_cam [3]: xc = cat(y, pose, shape, cam) [2205] ->
             fc1 -> fc2 (NO activation between them; dropout is the identity) -> pose += decpose(xc), shape += decshape(xc), cam +=
             deccam(xc); keys `regressor.{fc1,fc2,decpose,decshape,deccam}.*`, `regressor.init_{pose,shape,cam}`

The encoder's Linear and the regressor are ONE layer program of 1x1 PP_OP_CONVs on [1][1][C] buffers, one sample per frame:
`+=` is `res1` with PP_RELU_NONE (acc + bias + res), relu(h) a PP_OP_UPSAMPLE_ADD with PP_RELU_LAST, and the concatenation a wider
buffer written in channel slices (1x1 PP_OP_MAXPOOL with in_c_off / out_c_off is a slice copy).  Slices must start at multiples of 4,
so xc is laid out as y [0, 2048) | pose [2048, 2192) | shape [2192, 2202) | 2 zeros | cam [2204, 2207) | 1 zero, and fc1's columns
are permuted to match (zeros under the padding).  The initial estimates are program INPUTS ("init_pose", "init_shape", "init_cam"),
filled once for every sample slot when the model is made resident.  No dedicated kernel was needed.
"""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ..program import Program, ProgramBuilder
from .faster_rcnn import resnet50_body, resnet50_param_shapes

CROP = 224
FEAT, HIDDEN, GRU_LAYERS = 2048, 1024, 2
NPOSE, NSHAPE, NCAM = 144, 10, 3
XC = FEAT + NPOSE + 12 + 4                       # 2208: the padded concatenation
OFF_POSE, OFF_SHAPE, OFF_CAM = FEAT, FEAT + NPOSE, FEAT + NPOSE + 12
SEQ = 32                                         # the reference's DataLoader batch = one GRU sequence
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def spin_param_shapes() -> dict:
    """the backbone keys of SPIN's checkpoint (`model`): torchvision names, no prefix"""
    sh = {}
    resnet50_param_shapes(sh, "")
    return {k[len("backbone."):]: v for k, v in sh.items()}


def vibe_param_shapes() -> dict:
    """the generator keys read from VIBE's checkpoint (`gen_state_dict`)"""
    sh = {}
    for l in range(GRU_LAYERS):
        inp = FEAT if l == 0 else HIDDEN
        sh[f"encoder.gru.weight_ih_l{l}"], sh[f"encoder.gru.weight_hh_l{l}"] = (3 * HIDDEN, inp), (3 * HIDDEN, HIDDEN)
        sh[f"encoder.gru.bias_ih_l{l}"], sh[f"encoder.gru.bias_hh_l{l}"] = (3 * HIDDEN,), (3 * HIDDEN,)
    sh["encoder.linear.weight"], sh["encoder.linear.bias"] = (FEAT, HIDDEN), (FEAT,)
    sh["regressor.fc1.weight"], sh["regressor.fc1.bias"] = (1024, FEAT + NPOSE + NSHAPE + NCAM), (1024,)
    sh["regressor.fc2.weight"], sh["regressor.fc2.bias"] = (1024, 1024), (1024,)
    for name, n in (("decpose", NPOSE), ("decshape", NSHAPE), ("deccam", NCAM)):
        sh[f"regressor.{name}.weight"], sh[f"regressor.{name}.bias"] = (n, 1024), (n,)
    sh["regressor.init_pose"], sh["regressor.init_shape"], sh["regressor.init_cam"] = (1, NPOSE), (1, NSHAPE), (1, NCAM)
    return sh


def synth_params(shapes: dict, seed: int = 0) -> dict:
    """Seeded parameters for POSEPIPE_SYNTHETIC_WEIGHTS=1: PyTorch's own initial scales (GRU and Linear uniform +-1 / sqrt(fan), the
    decoders with SPIN's xavier gain 0.01 scale), init_pose the identity in the 6-D form, init_cam (0.9, 0, 0)"""
    rng = np.random.default_rng(seed)
    p = {}
    for name, shp in shapes.items():
        if name == "regressor.init_pose":
            a = np.tile(np.array([1, 0, 0, 1, 0, 0], np.float64), 24).reshape(shp) + rng.normal(0, 0.05, shp)
        elif name == "regressor.init_shape":
            a = rng.normal(0, 0.2, shp)
        elif name == "regressor.init_cam":
            a = np.array([[0.9, 0.0, 0.0]])
        elif ".gru." in name:
            a = rng.uniform(-1, 1, shp) / np.sqrt(HIDDEN)
        elif name.startswith("regressor.dec"):
            a = rng.uniform(-1, 1, shp) * (0.1 / np.sqrt(1024))
        else:
            fan = shp[1] if len(shp) == 2 else shapes[name[:-len("bias")] + "weight"][1]
            a = rng.uniform(-1, 1, shp) / np.sqrt(fan)
        p[name] = a.astype(np.float32)
    return p


def checked(sd: dict, shapes: dict, what: str) -> dict:
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise KeyError(f"{what}: missing parameters {missing[:5]}{'...' if len(missing) > 5 else ''}")
    wrong = [(k, tuple(np.shape(sd[k])), shapes[k]) for k in shapes if tuple(np.shape(sd[k])) != tuple(shapes[k])]
    if wrong:
        raise ValueError(f"{what}: parameter shapes differ (key, found, expected): {wrong[:5]}{'...' if len(wrong) > 5 else ''}")
    return {k: np.asarray(sd[k], np.float32) for k in shapes}


def gru_layers(sd: dict) -> list:
    """[(W_ih, W_hh, b_ih, b_hh)] per layer, for ops.Gru"""
    return [tuple(sd[f"encoder.gru.{n}_l{l}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(GRU_LAYERS)]


def build_backbone_program(spin_sd: dict) -> Program:
    """"input" [224][224][4] (R, G, B, 0 normalised) -> "features" [1][1][2048]"""
    sd = {"backbone." + k: v for k, v in checked(spin_sd, spin_param_shapes(), "SPIN backbone").items()}
    pb = ProgramBuilder()
    x = pb.buf(CROP, CROP, 4, name="input")
    c5 = resnet50_body(pb, sd, x, "")[3]                      # [7][7][2048]
    pb.mark_output(pb.avgpool(c5, 7, 7, 1, name="avgpool"), "features")
    return pb.build()


def _rows(w, n):
    out = np.zeros((n,) + w.shape[1:], np.float32)
    out[:w.shape[0]] = w
    return out


def fc1_permuted(w) -> np.ndarray:
    """fc1.weight [1024][2205] (columns y | pose | shape | cam) -> [1024][2208] in the padded xc layout"""
    out = np.zeros((w.shape[0], XC), np.float32)
    out[:, :OFF_SHAPE + NSHAPE] = w[:, :FEAT + NPOSE + NSHAPE]
    out[:, OFF_CAM:OFF_CAM + NCAM] = w[:, FEAT + NPOSE + NSHAPE:]
    return out


def build_head_program(vibe_sd: dict, n_iter: int = 3) -> Program:
    """inputs "h" [1][1][1024] (the GRU's output), "features" [1][1][2048], "init_pose" [144], "init_shape" [12], "init_cam" [4] ->
    outputs "pose6d" [144], "shape" [12] (10 real), "cam" [4] (3 real)"""
    sd = checked(vibe_sd, vibe_param_shapes(), "VIBE generator")
    as_conv = lambda w: np.asarray(w, np.float32)[:, :, None, None]                   # noqa: E731
    pb = ProgramBuilder()
    h = pb.buf(1, 1, HIDDEN, name="h")
    f = pb.buf(1, 1, FEAT, name="features")
    pose, shape, cam = pb.buf(1, 1, NPOSE, name="init_pose"), pb.buf(1, 1, 12, name="init_shape"), pb.buf(1, 1, 4, name="init_cam")
    rh = pb.upsample_add(h, up_log2=0, relu=L.PP_RELU_LAST, name="encoder.relu")
    y = pb.conv(rh, as_conv(sd["encoder.linear.weight"]), sd["encoder.linear.bias"], res1=f, name="encoder.linear")
    fc1_w, fc2_w = as_conv(fc1_permuted(sd["regressor.fc1.weight"])), as_conv(sd["regressor.fc2.weight"])
    for it in range(n_iter):
        xc = pb.buf(1, 1, XC)
        pb.maxpool(y, 1, 1, 0, name=f"cat{it}.y", out=xc, out_c_off=0)
        pb.maxpool(pose, 1, 1, 0, name=f"cat{it}.pose", out=xc, out_c_off=OFF_POSE)
        pb.maxpool(shape, 1, 1, 0, name=f"cat{it}.shape", out=xc, out_c_off=OFF_SHAPE)
        pb.maxpool(cam, 1, 1, 0, name=f"cat{it}.cam", out=xc, out_c_off=OFF_CAM)
        a = pb.conv(xc, fc1_w, sd["regressor.fc1.bias"], name=f"fc1.{it}")
        b = pb.conv(a, fc2_w, sd["regressor.fc2.bias"], name=f"fc2.{it}")
        pose = pb.conv(b, as_conv(sd["regressor.decpose.weight"]), sd["regressor.decpose.bias"], res1=pose, name=f"decpose.{it}")
        shape = pb.conv(b, as_conv(_rows(sd["regressor.decshape.weight"], 12)), _rows(sd["regressor.decshape.bias"], 12), res1=shape,
                        name=f"decshape.{it}")
        cam = pb.conv(b, as_conv(_rows(sd["regressor.deccam.weight"], 4)), _rows(sd["regressor.deccam.bias"], 4), res1=cam, name=f"deccam.{it}")
    pb.mark_output(pose, "pose6d")
    pb.mark_output(shape, "shape")
    pb.mark_output(cam, "cam")
    return pb.build()


def init_inputs(vibe_sd: dict, n: int) -> dict:
    """what the head program's three init_* inputs hold, for n sample slots"""
    pad = lambda a, c: np.tile(_rows(np.asarray(a, np.float32).reshape(-1, 1), c).reshape(1, c), (n, 1))      # noqa: E731
    return {"init_pose": pad(vibe_sd["regressor.init_pose"], NPOSE), "init_shape": pad(vibe_sd["regressor.init_shape"], 12),
            "init_cam": pad(vibe_sd["regressor.init_cam"], 4)}
