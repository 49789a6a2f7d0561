"""GAST-Net (Liu et al., "A Graph Attention Spatio-temporal Convolutional Network for 3D Human Pose Estimation in Video") as a pp_net
layer program: the lifter behind pose_pipeline/wrappers/gastnet_lifting.py:27-57, `SpatioTemporalModel(adj, 17, 2, 17, filter_widths,
channels)` in eval mode, whole-clip dilated form (as models/videopose3d.py).

`model/gast_net.py` is NOT in the reference tree: what follows is an UNPINNED restatement of the published model (the
list of what to check first is in wrappers/gastnet.py).  gastnet_param_shapes() is what a real checkpoint meets first; where it
disagrees, the checkpoint wins and the change belongs in this file only.

Activations are NHWC with H = the 17 joints, W = time, C = channels (the model's own tensors are (B, C, T, J): its (k, 1) temporal
kernels are (1, k) kernels here, `dil=(1, d)`).  Every BatchNorm is folded on the host (fold_bn, float64).  With fw = filter_widths,
C = channels:

  init_bn       BatchNorm2d over the 2 input features = an affine on the input, folded into expand_conv: weights scaled per input
                channel + a bias term (exact: the convolution has no padding)
  x = relu(expand_bn(expand_conv(x)))          2 -> C, temporal fw[0], no bias
  x = GAB_0(x)                                 C -> 2 C
  for i = 1 .. len(fw) - 1, Ci = 2^i C, dilation d = prod(fw[:i]):
      res = centre crop of x (res1_off_w)
      x = relu(bn(layers_conv.{2i-2}(x)))      Ci -> Ci, temporal fw[i], dilation d
      x = res + relu(bn(layers_conv.{2i-1}(x)))  1x1 (PP_RELU_FIRST)
      x = GAB_i(x)                             Ci -> 2 Ci
  shrink        1x1, 2^len(fw) C -> 3, no bias: "output" (17, chunk, 3)

GAB(x), the GraphAttentionBlock `layers_graph_conv.{i}` of input width D:  relu(cat_bn(cat_conv(cat(x, L(x), G(x))))), cat_conv 1x1
3 D -> 2 D without bias.  The three parts are written into one 3 D-wide buffer with out_c_off.  PP_OP_CONV reads whole buffers only, so
the convolution that produces x is launched twice, once into a buffer of its own (what L and G read) and once into the first third of
the wide one: 1 / 16 of a block's multiply-adds, and no copy pass.

L = local_graph_layer: gcn_sym and gcn_con, two SemCHGraphConv(D, D) over the symmetry and the connection graph (W (2, D, D), e (D,
nnz(mask)), bias (D,)), each followed by bn_1 / bn_2 + ReLU; concatenated; cat_conv 1x1 2 D -> D without bias, cat_bn, ReLU.  A
SemCHGraphConv is, per output channel c,  out[j, c] = sum_i A_c[j, i] * h_[i != j][i, c] + bias[c],  h0 = x W[0], h1 = x W[1],
A_c = softmax_i(e_c scattered on the mask in row-major order of its non-zeros, -9e15 elsewhere).  A_c is constant at inference:
graph_matrices() evaluates it in float64 and folds the BatchNorm behind it in (rows of A_c scaled, scale and shift on the bias).
Both graph convolutions read the same x: ONE 1x1 convolution D -> 4 D, [sym h0 | sym h1 | con h0 | con h1], then ONE PP_OP_GRAPH_MIX
writing 2 D channels.

G = global_graph_layer: MultiGlobalGraph with `heads` heads of D / heads channels: per head 1x1 projections theta.{h}, phi.{h}, g.{h}
with bias; softmax_j(theta_i . phi_j) g_j over the 17 joints of one frame, no 1 / sqrt(d) scale; heads concatenated; cat_conv 1x1 D -> D
without bias, cat_bn, ReLU.  ONE 1x1 convolution D -> 3 D in PP_OP_ATTENTION's [q | k | v] head-major order, then PP_OP_JOINT_ATTN.

The rf = 81 model (`81_frame_model.bin`) is GastNetSpec(filter_widths=(3, 3, 3, 3), channels=64): the same code.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import _lib as L
from ..program import Program, ProgramBuilder, fold_bn

H36M_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
H36M_LEFT = (4, 5, 6, 11, 12, 13)
H36M_RIGHT = (1, 2, 3, 14, 15, 16)
H36M_DISTAL = (3, 6, 10, 13, 16)
_BN = ("weight", "bias", "running_mean", "running_var")


@dataclass(frozen=True)
class GastNetSpec:               # wrappers/gastnet_lifting.py:27-48, rf = 27
    num_joints: int = 17
    in_features: int = 2
    filter_widths: tuple = (3, 3, 3)
    channels: int = 128
    heads: int = 4
    chunk: int = 256             # output frames per program invocation

    @property
    def receptive_field(self):
        rf = 1
        for f in self.filter_widths:
            rf *= f
        return rf

    @property
    def pad(self):
        return (self.receptive_field - 1) // 2


# ---- the graphs ------------------------------------------------------------------------------------------------------------------
def skeleton_adjacency() -> np.ndarray:
    """adj_mx_from_skeleton: A + A^T + I over the parent links, every row divided by its sum (float64)"""
    a = np.zeros((17, 17))
    for j, p in enumerate(H36M_PARENTS):
        if p >= 0:
            a[j, p] = a[p, j] = 1.0
    a += np.eye(17)
    return a / a.sum(axis=1, keepdims=True)


def graph_masks() -> dict:
    """{"sym", "con"}: boolean [17][17] masks of the two SemCHGraphConv.  sym: the identity plus the left <-> right pairs (29
    non-zeros).  con: adj + adj^2 with the 2nd-order rows of the non-distal joints and the 1st-order rows of the distal joints zeroed,
    > 0 (UNPINNED: the rule of the published local_graph_layer as restated in the issue)."""
    sym = np.eye(17, dtype=bool)
    for l, r in zip(H36M_LEFT, H36M_RIGHT):
        sym[l, r] = sym[r, l] = True
    adj = skeleton_adjacency()
    first, second = adj.copy(), adj @ adj
    distal = np.zeros(17, bool)
    distal[list(H36M_DISTAL)] = True
    first[distal] = 0.0
    second[~distal] = 0.0
    con = (first + second) > 0
    assert sym.any(axis=1).all() and con.any(axis=1).all()          # no empty row: every softmax has a term on the mask
    return {"sym": sym, "con": con}


def gastnet_param_shapes(spec: GastNetSpec = GastNetSpec()) -> dict:
    """every key read, with its torch shape"""
    masks = graph_masks()
    fw, c = spec.filter_widths, spec.channels
    sh = {}

    def bn(prefix, n):
        for s in _BN:
            sh[f"{prefix}.{s}"] = (n,)

    def gab(prefix, d):
        hd = d // spec.heads
        for name, bn_name in (("gcn_sym", "bn_1"), ("gcn_con", "bn_2")):
            sh[f"{prefix}.local_graph_layer.{name}.W"] = (2, d, d)
            sh[f"{prefix}.local_graph_layer.{name}.e"] = (d, int(masks[name[4:]].sum()))
            sh[f"{prefix}.local_graph_layer.{name}.bias"] = (d,)
            bn(f"{prefix}.local_graph_layer.{bn_name}", d)
        sh[f"{prefix}.local_graph_layer.cat_conv.weight"] = (d, 2 * d, 1, 1)
        bn(f"{prefix}.local_graph_layer.cat_bn", d)
        for h in range(spec.heads):
            for p in ("theta", "phi", "g"):
                sh[f"{prefix}.global_graph_layer.{p}.{h}.weight"] = (hd, d, 1, 1)
                sh[f"{prefix}.global_graph_layer.{p}.{h}.bias"] = (hd,)
        sh[f"{prefix}.global_graph_layer.cat_conv.weight"] = (d, d, 1, 1)
        bn(f"{prefix}.global_graph_layer.cat_bn", d)
        sh[f"{prefix}.cat_conv.weight"] = (2 * d, 3 * d, 1, 1)
        bn(f"{prefix}.cat_bn", 2 * d)

    bn("init_bn", spec.in_features)
    sh["expand_conv.weight"] = (c, spec.in_features, fw[0], 1)
    bn("expand_bn", c)
    gab("layers_graph_conv.0", c)
    for i in range(1, len(fw)):
        ci = c << i
        sh[f"layers_conv.{2 * i - 2}.weight"] = (ci, ci, fw[i], 1)
        sh[f"layers_conv.{2 * i - 1}.weight"] = (ci, ci, 1, 1)
        bn(f"layers_bn.{2 * i - 2}", ci)
        bn(f"layers_bn.{2 * i - 1}", ci)
        gab(f"layers_graph_conv.{i}", ci)
    sh["shrink.weight"] = (3, c << len(fw), 1, 1)
    return sh


def synth_params(shapes: dict, seed: int = 0) -> dict:
    """Seeded synthetic parameters for POSEPIPE_SYNTHETIC_WEIGHTS=1 (the `synth=` hook of weights.get_state_dict): convolution and
    graph weights N(0, 1 / fan_in), BatchNorm gamma and variance near 1, beta and mean small, the graph logits e N(0, 1): activations
    of order one at every depth for normalised key points."""
    rng = np.random.default_rng(seed)
    p = {}
    for name, shp in shapes.items():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "running_var":
            a = rng.uniform(0.6, 1.4, shp)
        elif leaf == "running_mean":
            a = rng.normal(0, 0.1, shp)
        elif leaf == "e":
            a = rng.standard_normal(shp)
        elif leaf == "W":
            a = rng.standard_normal(shp) * np.sqrt(1.0 / shp[1])
        elif len(shp) == 1 and leaf == "weight":                      # BatchNorm gamma
            a = rng.uniform(0.8, 1.2, shp)
        elif len(shp) == 1:                                           # BatchNorm beta, biases
            a = rng.normal(0, 0.1, shp)
        else:
            a = rng.standard_normal(shp) * np.sqrt(1.0 / int(np.prod(shp[1:])))
        p[name] = a.astype(np.float32)
    return p


def checked_state_dict(spec: GastNetSpec, sd: dict) -> dict:
    """the keys read as float32 arrays.  A missing key is a KeyError, another shape a ValueError; an `e` of another width names the
    mask and both counts (the masks are unpinned: that is the first thing a real checkpoint can disagree with)."""
    shapes = gastnet_param_shapes(spec)
    masks = graph_masks()
    for k, shp in shapes.items():
        if k not in sd:
            raise KeyError(f"missing parameter {k}")
        got = tuple(np.shape(sd[k]))
        if got != tuple(shp):
            if k.endswith(".e") and len(got) == 2 and got[0] == shp[0]:
                which = "sym" if ".gcn_sym." in k else "con"
                raise ValueError(f"{k}: the checkpoint's graph has {got[1]} edges, the {which} mask built here (models/gastnet.graph_masks) "
                                 f"has {int(masks[which].sum())}")
            raise ValueError(f"{k}: shape {got} != {shp}")
    return {k: np.asarray(sd[k], np.float32) for k in shapes}


def graph_matrices(e, mask, gcn_bias, bn) -> tuple:
    """A SemCHGraphConv's constant part with the BatchNorm behind it folded in, float64 -> float32 once.
    e (D, nnz), mask bool [17][17], gcn_bias (D,), bn = (gamma, beta, mean, var) -> (A [17][17][D] with zeros off the mask, bias [D])"""
    e = np.asarray(e, np.float64)
    d = e.shape[0]
    logits = np.full((d, 17, 17), -9e15)
    logits[:, mask] = e                                               # row-major order of the mask's non-zeros
    logits -= logits.max(axis=2, keepdims=True)
    a = np.exp(logits)
    a /= a.sum(axis=2, keepdims=True)
    a[:, ~mask] = 0.0                                                 # (exp(-9e15 - max) is 0 already)
    gamma, beta, mean, var = (np.asarray(v, np.float64) for v in bn)
    scale = gamma / np.sqrt(var + 1e-5)
    a *= scale[:, None, None]
    bias = beta + (np.asarray(gcn_bias, np.float64) - mean) * scale
    return np.ascontiguousarray(np.transpose(a, (1, 2, 0))).astype(np.float32), bias.astype(np.float32)


def _time_kernel(w):
    """torch (cout, cin, k, 1) over (time, joints) -> (cout, cin, 1, k) over (joints, time)"""
    return np.transpose(np.asarray(w), (0, 1, 3, 2))


def build_gastnet_program(spec: GastNetSpec, sd: dict) -> Program:
    """"input" [17][chunk + 2 pad][4] (x, y, 0, 0 per joint and frame) -> "output" [17][chunk][3]"""
    if spec.num_joints != 17 or spec.in_features != 2:
        raise ValueError(f"GAST-Net lifts 17 H36M joints of 2 features; got {spec}")
    if spec.channels % 16 or spec.channels <= 0 or spec.channels % (4 * spec.heads):
        raise ValueError(f"channels = {spec.channels}: a multiple of 16 (and of 4 * heads) is needed, the head widths are multiples of 4")
    if (spec.channels << (len(spec.filter_widths) - 1)) // spec.heads > 128:
        raise ValueError(f"{spec}: the widest block has heads of more than 128 channels (PP_OP_JOINT_ATTN)")
    if any(f % 2 == 0 or f < 1 for f in spec.filter_widths):
        raise ValueError(f"filter_widths {spec.filter_widths}: odd widths only")
    sd = checked_state_dict(spec, sd)
    masks = graph_masks()
    fw, heads = spec.filter_widths, spec.heads
    pb = ProgramBuilder()

    def bn_of(prefix):
        return tuple(sd[f"{prefix}.{s}"] for s in _BN)

    def cbr(x, weight, bn, *, conv_bias=None, dil=1, name, **kw):
        gamma, beta, mean, var = bn_of(bn)
        w, b = fold_bn(weight, conv_bias, gamma, beta, mean, var)
        return pb.conv(x, w, b, dil=(1, dil), name=name, **kw)

    def twice(x, weight, bn, d, *, name, **kw):
        """the convolution that produces a block's input: (its own buffer, the 3 d-wide buffer whose first third holds it too)"""
        dense = cbr(x, weight, bn, name=name, **kw)
        h, w, _ = pb.dims(dense)
        wide = pb.buf(h, w, 3 * d)
        cbr(x, weight, bn, name=name + ".cat", out=wide, out_c_off=0, **kw)
        return dense, wide

    def gab(x, wide, d, prefix):
        lg, gg = prefix + ".local_graph_layer", prefix + ".global_graph_layer"
        # L: one projection for both graphs, one mix
        proj = np.concatenate([sd[f"{lg}.{g}.W"][k].T for g in ("gcn_sym", "gcn_con") for k in (0, 1)], axis=0)      # [4 d][d]
        hh = pb.conv(x, proj.reshape(4 * d, d, 1, 1), None, name=lg + ".W")
        mats, biases = zip(*(graph_matrices(sd[f"{lg}.gcn_{g}.e"], masks[g], sd[f"{lg}.gcn_{g}.bias"], bn_of(f"{lg}.{b}"))
                             for g, b in (("sym", "bn_1"), ("con", "bn_2"))))
        mixed = pb.graph_mix(hh, mats, biases, [masks["sym"], masks["con"]], relu=L.PP_RELU_LAST, name=lg + ".mix")
        cbr(mixed, sd[f"{lg}.cat_conv.weight"], f"{lg}.cat_bn", relu=L.PP_RELU_LAST, out=wide, out_c_off=d, name=lg + ".cat_conv")
        # G: q | k | v head-major, joint attention
        wq = np.concatenate([sd[f"{gg}.{p}.{h}.weight"] for p in ("theta", "phi", "g") for h in range(heads)], axis=0)   # [3 d][d][1][1]
        bq = np.concatenate([sd[f"{gg}.{p}.{h}.bias"] for p in ("theta", "phi", "g") for h in range(heads)])
        qkv = pb.conv(x, wq, bq, name=gg + ".qkv")
        att = pb.joint_attention(qkv, c_real=d, heads=heads, name=gg + ".attn")
        cbr(att, sd[f"{gg}.cat_conv.weight"], f"{gg}.cat_bn", relu=L.PP_RELU_LAST, out=wide, out_c_off=2 * d, name=gg + ".cat_conv")
        return cbr(wide, sd[f"{prefix}.cat_conv.weight"], f"{prefix}.cat_bn", relu=L.PP_RELU_LAST, name=prefix + ".cat_conv")

    # init_bn folded into expand_conv (float64): w' = w * a[cin], bias = sum over (cin, k) of w * b[cin]
    g0, b0, m0, v0 = (np.asarray(v, np.float64) for v in bn_of("init_bn"))
    a_in = g0 / np.sqrt(v0 + 1e-5)
    b_in = b0 - m0 * a_in
    w_exp = _time_kernel(sd["expand_conv.weight"]).astype(np.float64)
    bias_exp = (w_exp * b_in[None, :, None, None]).sum(axis=(1, 2, 3))
    w_exp = w_exp * a_in[None, :, None, None]

    t_in = spec.chunk + 2 * spec.pad
    c = spec.channels
    x = pb.buf(17, t_in, 4, name="input")
    x, wide = twice(x, w_exp, "expand_bn", c, conv_bias=bias_exp, relu=L.PP_RELU_LAST, name="expand_conv")
    x = gab(x, wide, c, "layers_graph_conv.0")
    dil = fw[0]
    for i in range(1, len(fw)):
        ci = c << i
        y = cbr(x, _time_kernel(sd[f"layers_conv.{2 * i - 2}.weight"]), f"layers_bn.{2 * i - 2}", dil=dil, relu=L.PP_RELU_LAST,
                name=f"layers_conv.{2 * i - 2}")
        x, wide = twice(y, sd[f"layers_conv.{2 * i - 1}.weight"], f"layers_bn.{2 * i - 1}", ci, relu=L.PP_RELU_FIRST, res1=x,
                        res1_off_w=dil * (fw[i] // 2), name=f"layers_conv.{2 * i - 1}")
        x = gab(x, wide, ci, f"layers_graph_conv.{i}")
        dil *= fw[i]
    out = pb.buf(17, spec.chunk, 3, name="output")
    pb.conv(x, sd["shrink.weight"], None, out=out, name="shrink")
    return pb.build()
