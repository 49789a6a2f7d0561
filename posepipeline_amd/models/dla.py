"""DLA-34 with the DCN up-sampling head (`pose_dla_dcn` of CenterNet / FairMOT) as a layer program.

The network behind pose_pipeline/wrappers/fairmot.py (`create_model('dla_34', heads, head_conv=256)`): restated from the published
model (lib/models/networks/pose_dla_dcn.py), UNPINNED -- FairMOT and DCNv2 are not vendored.  State-dict keys are upstream's.

  base     DLA(levels [1, 1, 1, 2, 2, 1], channels [16, 32, 64, 128, 256, 512], BasicBlock):
           base_layer 7x7 3 -> 16 + BN + ReLU; level0 3x3 16 -> 16; level1 3x3 stride 2 16 -> 32; level2 .. level5 Trees of BasicBlocks
           (MaxPool2d(2) downsample, 1x1 + BN projection of the residual where channels change, Root = 1x1 over the concatenated
           children + BN + ReLU, level_root on levels 3 - 5).  A Root's concatenation is ONE buffer whose channel slices the
           producers write (the last block's conv2 directly, the others by a 1x1 "max-pool" slice copy, as models/yolox.py).
           Levels 3 and 4 also own a `project` whose result upstream computes and never uses (their tree1 is a Tree, which takes
           no residual): it is neither in the inventory nor in the program.  `base.fc` of the ImageNet classifier is not used either.
  dla_up   DLAUp(2, [64, 128, 256, 512], [1, 2, 4, 8]): ida_0 (256; 2 DCNs), ida_1 (128; 4), ida_2 (64; 6)
  ida_up   IDAUp(64, [64, 128, 256], [1, 2, 4]): 4 DCNs
  IDAUp step: layers[i] = up(proj(layers[i])); layers[i] = node(layers[i] + layers[i - 1]).  proj / node = DCN(3x3) + BN + ReLU
           (PP_OP_CONV conv_offset_mask 3x3 -> 27, then PP_OP_DCN3X3 with the BN folded into its weight and bias); up = depthwise
           ConvTranspose2d(2f, f, f // 2) with the checkpoint's weights (PP_OP_DWDECONV), which also carries the `+ layers[i - 1]`.
  heads    hm 1, wh 4, id 128, reg 2 on the 64-channel stride-4 map: 3x3 64 -> 256 + ReLU, 1x1 -> c, both with bias.

16 DCN layers in all; shapes (cin -> cout at h x w, 608 x 1088 input): 512 -> 256 at 19 x 34; 256 -> 256, 256 -> 128 (x2), 256 -> 64 at
38 x 68; 128 -> 128 (x2), 128 -> 64 (x4) at 76 x 136; 64 -> 64 (x5) at 152 x 272.

The program input is [hp][wp][4] float32 RGB / 255 (pp_fairmot_preprocess); the outputs are the buffers "hm", "wh", "id", "reg",
NHWC with exactly their own channels.
"""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ..program import Program, ProgramBuilder, fold_bn

LEVELS = (1, 1, 1, 2, 2, 1)
CHANNELS = (16, 32, 64, 128, 256, 512)
HEADS = (("hm", 1), ("wh", 4), ("id", 128), ("reg", 2))
HEAD_CONV = 256
DOWN_RATIO = 4
BN_EPS = 1e-5
CHECKPOINT = "fairmot/fairmot_dla34.pth"


def _bn(shapes, name, c):
    for s in ("weight", "bias", "running_mean", "running_var"):
        shapes[f"{name}.{s}"] = (c,)


def _block(shapes, name, cin, cout):
    shapes[name + ".conv1.weight"] = (cout, cin, 3, 3)
    _bn(shapes, name + ".bn1", cout)
    shapes[name + ".conv2.weight"] = (cout, cout, 3, 3)
    _bn(shapes, name + ".bn2", cout)


def _tree(shapes, name, levels, cin, cout, level_root, extra):
    """extra: channels of the children handed down to this tree's root"""
    if level_root:
        extra = extra + cin
    if levels == 1:
        if cin != cout:
            shapes[name + ".project.0.weight"] = (cout, cin, 1, 1)
            _bn(shapes, name + ".project.1", cout)
        _block(shapes, name + ".tree1", cin, cout)
        _block(shapes, name + ".tree2", cout, cout)
        shapes[name + ".root.conv.weight"] = (cout, 2 * cout + extra, 1, 1)
        _bn(shapes, name + ".root.bn", cout)
    else:
        _tree(shapes, name + ".tree1", levels - 1, cin, cout, False, 0)
        _tree(shapes, name + ".tree2", levels - 1, cout, cout, False, extra + cout)


def _deform(shapes, name, cin, cout):
    shapes[name + ".actf.0.weight"] = (cout,)
    shapes[name + ".actf.0.bias"] = (cout,)
    shapes[name + ".actf.0.running_mean"] = (cout,)
    shapes[name + ".actf.0.running_var"] = (cout,)
    shapes[name + ".conv.weight"] = (cout, cin, 3, 3)
    shapes[name + ".conv.bias"] = (cout,)
    shapes[name + ".conv.conv_offset_mask.weight"] = (27, cin, 3, 3)
    shapes[name + ".conv.conv_offset_mask.bias"] = (27,)


def _ida(shapes, name, o, channels, up_f):
    for i in range(1, len(channels)):
        f = int(up_f[i])
        _deform(shapes, f"{name}.proj_{i}", channels[i], o)
        _deform(shapes, f"{name}.node_{i}", o, o)
        shapes[f"{name}.up_{i}.weight"] = (o, 1, 2 * f, 2 * f)


def _dla_up_plan():
    """DLAUp.__init__ of DLAUp(2, [64, 128, 256, 512], [1, 2, 4, 8]): per ida_i (o, input channels, up factors)"""
    channels = list(CHANNELS[2:])
    in_channels = list(channels)
    scales = [1, 2, 4, 8]
    plan = []
    for i in range(len(channels) - 1):
        j = -i - 2
        plan.append((channels[j], list(in_channels[j:]), [s // scales[j] for s in scales[j:]]))
        scales[j + 1:] = [scales[j]] * len(scales[j + 1:])
        in_channels[j + 1:] = [channels[j]] * len(in_channels[j + 1:])
    return plan


def dla34_trunk_param_shapes() -> dict:
    """{upstream state-dict key: shape} of base, dla_up and ida_up: everything in front of the heads (shared with models/trades.py)"""
    s: dict = {}
    s["base.base_layer.0.weight"] = (16, 3, 7, 7)
    _bn(s, "base.base_layer.1", 16)
    s["base.level0.0.weight"] = (16, 16, 3, 3)
    _bn(s, "base.level0.1", 16)
    s["base.level1.0.weight"] = (32, 16, 3, 3)
    _bn(s, "base.level1.1", 32)
    for lv in range(2, 6):
        _tree(s, f"base.level{lv}", LEVELS[lv], CHANNELS[lv - 1], CHANNELS[lv], lv >= 3, 0)
    for i, (o, chans, up_f) in enumerate(_dla_up_plan()):
        _ida(s, f"dla_up.ida_{i}", o, chans, up_f)
    _ida(s, "ida_up", 64, [64, 128, 256], [1, 2, 4])
    return s


def dla34_param_shapes() -> dict:
    """{upstream state-dict key: shape} of every parameter the inference pass reads"""
    s = dla34_trunk_param_shapes()
    for head, c in HEADS:
        s[f"{head}.0.weight"] = (HEAD_CONV, 64, 3, 3)
        s[f"{head}.0.bias"] = (HEAD_CONV,)
        s[f"{head}.2.weight"] = (c, HEAD_CONV, 1, 1)
        s[f"{head}.2.bias"] = (c,)
    return s


def dla34_param_count() -> int:
    return int(sum(int(np.prod(v)) for v in dla34_param_shapes().values()))


def check_state_dict(sd: dict) -> dict:
    """keys and shapes of a checkpoint dict against the inventory (a `module.` prefix is dropped first); returns the float32 dict of
    the inventory's keys.  KeyError names missing parameters, ValueError a wrong shape.  Keys outside the inventory (base.fc,
    the unused projections, num_batches_tracked) are ignored."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    shapes = dla34_param_shapes()
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise KeyError(f"FairMOT DLA-34 checkpoint: missing parameters {missing[:5]}{'...' if len(missing) > 5 else ''}")
    for k, shp in shapes.items():
        if tuple(np.shape(sd[k])) != tuple(shp):
            raise ValueError(f"FairMOT DLA-34 checkpoint: {k} has shape {tuple(np.shape(sd[k]))}, expected {tuple(shp)}")
    return {k: np.asarray(sd[k], np.float32) for k in shapes}


def synth_dla34_state_dict(shapes: dict, seed: int) -> dict:
    """Seeded parameters: synth.synth_state_dict, then offsets of a fraction of a pixel (a He-normal conv_offset_mask moves every
    tap by several pixels), the transposed convolutions as upstream's `fill_up_weights` (bilinear) with a seeded 10 % perturbation
    (so that a kernel that assumed bilinear weights fails), and the `hm` head biased by seed_synthetic_head"""
    from .synth import synth_state_dict
    sd = synth_state_dict(shapes, seed)
    rng = np.random.default_rng(seed + 1000)
    for k in shapes:
        if k.endswith("conv_offset_mask.weight"):
            sd[k] = (sd[k] * np.float32(0.25)).astype(np.float32)
        elif ".up_" in k and k.endswith(".weight"):
            kk = shapes[k][2]
            f = int(np.ceil(kk / 2))
            c = (2 * f - 1 - f % 2) / (2.0 * f)
            i = np.arange(kk)
            w1 = 1 - np.abs(i / f - c)
            w = np.outer(w1, w1)[None, None] * rng.uniform(0.9, 1.1, shapes[k])
            sd[k] = w.astype(np.float32)
    return seed_synthetic_head(sd)


def seed_synthetic_head(sd: dict, hm_bias: float = -2.2, hm_gain: float = 100.0) -> dict:
    """Make seeded weights behave like a detector with few candidates.  The seeded network's raw heat-map logits are almost flat
    (measured at 608 x 1088 on clips and on noise: mean -0.04, standard deviation 0.009, about 4 500 local maxima, of which 40 - 70
    -- at the zero-padded lower border -- exceed 0.01 and none lies between 0.0 and 0.015), so the last layer of the `hm` head is
    amplified by 100 and biased by -2.2: logit > -1.386 (sigmoid > 0.2) then means raw > 0.008, which tens of cells pass and whose
    nearest other peak scores 0.07.  Box sizes get a positive bias so that candidates are boxes of a few cells.  In place."""
    sd["hm.2.weight"] = (sd["hm.2.weight"] * np.float32(hm_gain)).astype(np.float32)
    sd["hm.2.bias"] = np.full_like(sd["hm.2.bias"], hm_bias)
    sd["wh.2.bias"] = np.full_like(sd["wh.2.bias"], 6.0)
    return sd


def get_state_dict(seed: int = 11) -> dict:
    """fairmot/fairmot_dla34.pth under MODEL_DATA_DIR, keys and shapes checked; POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded
    parameters when the file is absent"""
    import os
    from .. import weights
    path = os.path.join(weights.model_data_dir(), CHECKPOINT)
    if os.path.exists(path):
        return check_state_dict(weights.load_state_dict(path))
    return weights.get_state_dict(CHECKPOINT, dla34_param_shapes(), seed=seed, synth=synth_dla34_state_dict)


def dla34_trunk(pb: ProgramBuilder, sd: dict, hp: int, wp: int) -> int:
    """base, dla_up and ida_up on the builder's new "input" buffer [hp][wp][4] -> the 64-channel stride-4 feature map (virtual
    buffer).  hp, wp: multiples of 32."""
    assert hp % 32 == 0 and wp % 32 == 0, (hp, wp)
    RELU = L.PP_RELU_LAST

    def convbn(x, conv, bn, *, stride=1, relu=RELU, **kw):
        wt = sd[conv + ".weight"]
        w, b = fold_bn(wt, None, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"], BN_EPS)
        return pb.conv(x, w, b, stride=stride, pad=wt.shape[2] // 2, relu=relu, name=conv, **kw)

    def slice_copy(src, dst, off):
        pb.maxpool(src, 1, 1, 0, name="route", out=dst, out_c_off=off)

    def block(x, name, stride, residual, **kw):
        y = convbn(x, name + ".conv1", name + ".bn1", stride=stride)
        return convbn(y, name + ".conv2", name + ".bn2", res1=residual, **kw)

    def tree(x, name, levels, cin, cout, stride, level_root, children):
        children = list(children)
        bottom = pb.maxpool(x, stride, stride, 0, name=name + ".downsample") if stride > 1 else x
        if level_root:
            children.append(bottom)
        if levels > 1:
            x1 = tree(x, name + ".tree1", levels - 1, cin, cout, stride, False, [])
            return tree(x1, name + ".tree2", levels - 1, cout, cout, 1, False, children + [x1])
        residual = convbn(bottom, name + ".project.0", name + ".project.1", relu=L.PP_RELU_NONE) if cin != cout else bottom
        x1 = block(x, name + ".tree1", stride, residual)
        h, w, _ = pb.dims(x1)
        cat = pb.buf(h, w, 2 * cout + sum(pb.dims(c)[2] for c in children))      # torch.cat([x2, x1, *children], 1)
        block(x1, name + ".tree2", 1, x1, out=cat, out_c_off=0)
        slice_copy(x1, cat, cout)
        off = 2 * cout
        for c in children:
            slice_copy(c, cat, off)
            off += pb.dims(c)[2]
        return convbn(cat, name + ".root.conv", name + ".root.bn")

    def deform(x, name):
        om = pb.conv(x, sd[name + ".conv.conv_offset_mask.weight"], sd[name + ".conv.conv_offset_mask.bias"], pad=1,
                     name=name + ".conv.conv_offset_mask")
        w, b = fold_bn(sd[name + ".conv.weight"], sd[name + ".conv.bias"], sd[name + ".actf.0.weight"], sd[name + ".actf.0.bias"],
                       sd[name + ".actf.0.running_mean"], sd[name + ".actf.0.running_var"], BN_EPS)
        return pb.dcn3x3(x, om, w, b, relu=RELU, name=name + ".conv")

    def ida(layers, name, startp, endp):
        for i in range(startp + 1, endp):
            k = i - startp
            up_w = sd[f"{name}.up_{k}.weight"]
            y = deform(layers[i], f"{name}.proj_{k}")
            y = pb.dwdeconv(y, up_w, up_w.shape[2] // 2, res1=layers[i - 1], name=f"{name}.up_{k}")
            layers[i] = deform(y, f"{name}.node_{k}")

    x = pb.buf(hp, wp, 4, name="input")
    x = convbn(x, "base.base_layer.0", "base.base_layer.1")
    y = [convbn(x, "base.level0.0", "base.level0.1")]
    y.append(convbn(y[0], "base.level1.0", "base.level1.1", stride=2))
    for lv in range(2, 6):
        y.append(tree(y[-1], f"base.level{lv}", LEVELS[lv], CHANNELS[lv - 1], CHANNELS[lv], 2, lv >= 3, []))
    layers = list(y)
    out = [layers[-1]]
    for i in range(3):                                   # DLAUp.forward, startp = 2
        ida(layers, f"dla_up.ida_{i}", len(layers) - i - 2, len(layers))
        out.insert(0, layers[-1])
    z = out[:3]
    ida(z, "ida_up", 0, 3)
    feat = z[-1]
    h, w, _ = pb.dims(feat)
    assert (h, w) == (hp // DOWN_RATIO, wp // DOWN_RATIO)
    return feat


def build_dla34_program(sd: dict, hp: int, wp: int, keep=()) -> Program:
    """hp, wp: network input size, multiples of 32.  keep: op names whose outputs keep a buffer of their own, found under that
    name in Program.named (tests and profiles that read an intermediate map)"""
    pb = ProgramBuilder()
    feat = dla34_trunk(pb, sd, hp, wp)
    h, w, _ = pb.dims(feat)
    for head, c in HEADS:
        t = pb.conv(feat, sd[f"{head}.0.weight"], sd[f"{head}.0.bias"], pad=1, relu=L.PP_RELU_LAST, name=f"{head}.0")
        o = pb.buf(h, w, c, name=head)
        pb.conv(t, sd[f"{head}.2.weight"], sd[f"{head}.2.bias"], out=o, name=f"{head}.2")
    for name in keep:
        pb.mark_output(next(op["out"] for op in pb.vops if op["name"] == name), name)
    return pb.build()


def activation_bytes_per_frame(prog: Program) -> int:
    """bytes of the program's activation arena per sample (halo included)"""
    pads = prog.buf_pad or [0] * len(prog.bufs)
    return int(sum((h + p) * (w + p) * c * 4 for (h, w, c), p in zip(prog.bufs, pads)))
