"""PoseFormer (Zheng et al., ICCV 2021), the 81-frame `detected81f.bin` model, as the lifter behind
pose_pipeline/wrappers/poseformer.py:72-83.

`common/model_poseformer.py` is NOT in the reference tree: what follows is an UNPINNED restatement of the published model
(INTEGRATION.md), evaluated in inference mode (dropout and stochastic depth are identities).  With r = 32 channels per joint,
J = 17 joints, D = r * J = 544, F = 81 frames:

  block     timm's: x += proj(attn(LN1(x))); x += fc2(gelu(fc1(LN2(x)))); LayerNorm eps 1e-6; qkv Linear dim -> 3 dim with bias, output
            channel s * dim + head * hd + d = (q, k, v)[s]; softmax((q k^T) hd^-0.5) v; erf GELU; hidden int(dim * 2.0)
  spatial   per frame, 17 tokens of dim 32, 8 heads: x[j] = Spatial_patch_to_embedding(in[j]) + Spatial_pos_embed[0][j]; 4 blocks
            Spatial_blocks.{0..3}; Spatial_norm; the frame's 544 features at index j * 32 + c
  temporal  per window, 81 tokens of dim 544, 8 heads (hd 68): x[f] = feature[i + f] + Temporal_pos_embed[0][f]; 4 blocks blocks.{0..3};
            Temporal_norm; weighted_mean = Conv1d(81 -> 1, kernel 1) over the frame axis; head.0 LayerNorm (eps 1e-5); head.1 Linear 544 -> 51

On the device (csrc/poseformer.hip): the spatial stage is one fused kernel, run ONCE per frame of the clip -- the reference runs it
inside every 81-frame window, 81 times per frame.  The temporal stage is the layer program built here: LayerNorm, the Linear layers as
1x1 PP_OP_CONV on the matrix-core kernels (activations [B][1][81][C]), PP_OP_ATTENTION, PP_OP_GELU_ADD; it ends with Temporal_norm.
The weighted mean and the head are one more kernel.  The spatial parameters, Temporal_pos_embed and the head parameters ride in the
program's weight blob (Program.param_offsets holds their offsets), so the net's one resident blob is everything pp_poseformer_lift reads.

Channel padding: with `channel_pad` = 128 the temporal buffers are 640 / 3 * 640 / 1152 channels wide instead of 544 / 3 * 544 / 1088, so
that every Linear layer has a multiple of 128 output channels and is eligible for the split product kernel.  The padding rows and
columns of every weight and bias are exact zeros, LayerNorm and attention write exact zeros there, and gelu(0) = 0: the padding
channels are zeros end to end.  Measured, the padded form is 13 % slower in exact numerics and no faster in split numerics
(DESIGN_LOG.md 5k): the lifter builds the unpadded one, and the padded form is kept as a builder argument so that the comparison can be repeated.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ..program import Program, ProgramBuilder
from ..weights import strip_key_prefix


@dataclass(frozen=True)
class PoseFormerSpec:            # wrappers/poseformer.py:72-83
    num_frame: int = 81
    num_joints: int = 17
    in_chans: int = 2
    embed_dim_ratio: int = 32
    depth: int = 4
    num_heads: int = 8
    mlp_ratio: float = 2.0
    out_dim: int = 3

    @property
    def dim(self):
        return self.embed_dim_ratio * self.num_joints

    @property
    def pad(self):               # frames on each side of an output frame
        return (self.num_frame - 1) // 2


_BLOCK_KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
               "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _block_shapes(prefix, dim, hid):
    return {prefix + "norm1.weight": (dim,), prefix + "norm1.bias": (dim,), prefix + "attn.qkv.weight": (3 * dim, dim),
            prefix + "attn.qkv.bias": (3 * dim,), prefix + "attn.proj.weight": (dim, dim), prefix + "attn.proj.bias": (dim,),
            prefix + "norm2.weight": (dim,), prefix + "norm2.bias": (dim,), prefix + "mlp.fc1.weight": (hid, dim),
            prefix + "mlp.fc1.bias": (hid,), prefix + "mlp.fc2.weight": (dim, hid), prefix + "mlp.fc2.bias": (dim,)}


def poseformer_param_shapes(spec: PoseFormerSpec = PoseFormerSpec()) -> dict:
    """every key read, with its torch shape (110 tensors, 9 602 885 elements for the default spec)"""
    r, j, d, f = spec.embed_dim_ratio, spec.num_joints, spec.dim, spec.num_frame
    s = {"Spatial_patch_to_embedding.weight": (r, spec.in_chans), "Spatial_patch_to_embedding.bias": (r,),
         "Spatial_pos_embed": (1, j, r), "Temporal_pos_embed": (1, f, d)}
    for i in range(spec.depth):
        s.update(_block_shapes(f"Spatial_blocks.{i}.", r, int(r * spec.mlp_ratio)))
    for i in range(spec.depth):
        s.update(_block_shapes(f"blocks.{i}.", d, int(d * spec.mlp_ratio)))
    s.update({"Spatial_norm.weight": (r,), "Spatial_norm.bias": (r,), "Temporal_norm.weight": (d,), "Temporal_norm.bias": (d,),
              "weighted_mean.weight": (1, f, 1), "weighted_mean.bias": (1,), "head.0.weight": (d,), "head.0.bias": (d,),
              "head.1.weight": (j * spec.out_dim, d), "head.1.bias": (j * spec.out_dim,)})
    return s


def checked_state_dict(spec: PoseFormerSpec, sd: dict) -> dict:
    """{key: float32 array} of exactly the keys read, from a state dict whose keys may carry nn.DataParallel's `module.` prefix.  A
    missing key is a KeyError and a tensor of another shape a ValueError: the key names and weighted_mean.weight's shape are unpinned
    (INTEGRATION.md), so a checkpoint that differs must fail here, not be zero-padded into a parameter block."""
    sd = strip_key_prefix(sd, "module.")
    shapes = poseformer_param_shapes(spec)
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise KeyError(f"PoseFormer: missing parameters {missing[:5]}{'...' if len(missing) > 5 else ''}")
    wrong = [(k, tuple(np.shape(sd[k])), shapes[k]) for k in shapes if tuple(np.shape(sd[k])) != tuple(shapes[k])]
    if wrong:
        raise ValueError(f"PoseFormer: parameter shapes differ (key, found, expected): {wrong[:5]}{'...' if len(wrong) > 5 else ''}")
    return {k: np.asarray(sd[k], np.float32) for k in shapes}


def synth_params(shapes: dict, seed: int = 0) -> dict:
    """Seeded synthetic parameters for POSEPIPE_SYNTHETIC_WEIGHTS=1 (the `synth=` hook of weights.get_state_dict): Linear weights
    N(0, 1 / fan_in), LayerNorm gamma near 1 and beta small, position embeddings N(0, 0.02), weighted_mean.weight near 1 / 81 -- outputs
    of order one for inputs in [0, 1]."""
    rng = np.random.default_rng(seed)
    p = {}
    for name, shp in shapes.items():
        if name.endswith("pos_embed"):
            a = rng.normal(0, 0.02, shp)
        elif name == "weighted_mean.weight":
            a = rng.uniform(0.8, 1.2, shp) / shp[1]
        elif len(shp) == 1 and name.endswith(".weight"):          # LayerNorm gamma
            a = rng.uniform(0.8, 1.2, shp)
        elif len(shp) == 1:
            a = rng.normal(0, 0.05, shp)
        else:
            a = rng.standard_normal(shp) * np.sqrt(1.0 / int(np.prod(shp[1:])))
        p[name] = a.astype(np.float32)
    return p


def spatial_param_block(spec: PoseFormerSpec, sd: dict) -> np.ndarray:
    """flat fp32 block in the layout pp_poseformer_spatial documents (include/posepipe_hip.h)"""
    parts = [sd["Spatial_patch_to_embedding.weight"], sd["Spatial_patch_to_embedding.bias"], sd["Spatial_pos_embed"]]
    for i in range(spec.depth):
        parts += [sd[f"Spatial_blocks.{i}.{n}"] for n in _BLOCK_KEYS]
    parts += [sd["Spatial_norm.weight"], sd["Spatial_norm.bias"]]
    return np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in parts])


def head_param_block(spec: PoseFormerSpec, sd: dict) -> np.ndarray:
    """weighted_mean.weight [81] padded to 84, its bias padded to 4, head.0 gamma / beta [544], head.1.weight [51][544], head.1.bias padded to 52"""
    def padded(a, n):
        out = np.zeros(n, np.float32)
        a = np.asarray(a, np.float32).reshape(-1)
        out[:a.size] = a
        return out
    return np.concatenate([padded(sd["weighted_mean.weight"], 84), padded(sd["weighted_mean.bias"], 4),
                           padded(sd["head.0.weight"], spec.dim), padded(sd["head.0.bias"], spec.dim),
                           padded(sd["head.1.weight"], spec.num_joints * spec.out_dim * spec.dim), padded(sd["head.1.bias"], 52)])


def _check_spec(spec):
    want = PoseFormerSpec()
    if spec != want:
        raise ValueError(f"the device code is the 81-frame model {want}; got {spec}")


def _pad_up(n, m):
    return n if not m else -(-n // m) * m


def _pad2(w, rows, cols):
    out = np.zeros((rows, cols), np.float32)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _pad1(b, n):
    out = np.zeros(n, np.float32)
    out[:b.shape[0]] = b
    return out


def build_poseformer_program(spec: PoseFormerSpec, sd: dict, channel_pad: int = 0) -> Program:
    """The temporal stage as a layer program: "input" [1][81][C] (what the window gather writes) -> 4 blocks -> Temporal_norm ->
    "output" [1][81][C], C = 544 rounded up to `channel_pad` (0: no padding).  Program.param_offsets holds the blob offsets of the
    blocks pp_poseformer_lift reads: "spatial_params", "temporal_pos", "head_params"."""
    _check_spec(spec)
    sd = checked_state_dict(spec, sd)
    d, f, heads = spec.dim, spec.num_frame, spec.num_heads
    hid = int(d * spec.mlp_ratio)
    c, hp = _pad_up(d, channel_pad), _pad_up(hid, channel_pad)
    b = ProgramBuilder()
    x = b.buf(1, f, c, name="input")
    for i in range(spec.depth):
        p = {n: np.asarray(sd[f"blocks.{i}.{n}"], np.float32) for n in _BLOCK_KEYS}
        ln = b.layernorm(x, p["norm1.weight"], p["norm1.bias"], eps=1e-6, name=f"blocks.{i}.norm1")
        # q | k | v each in its own third of 3 * C channels: the layout PP_OP_ATTENTION reads
        wq = np.zeros((3, c, c), np.float32)
        wq[:, :d, :d] = p["attn.qkv.weight"].reshape(3, d, d)
        bq = np.zeros((3, c), np.float32)
        bq[:, :d] = p["attn.qkv.bias"].reshape(3, d)
        qkv = b.conv(ln, wq.reshape(3 * c, c, 1, 1), bq.reshape(-1), name=f"blocks.{i}.attn.qkv")
        att = b.attention(qkv, c_real=d, heads=heads, name=f"blocks.{i}.attn")
        x = b.conv(att, _pad2(p["attn.proj.weight"], c, c).reshape(c, c, 1, 1), _pad1(p["attn.proj.bias"], c), res1=x,
                   name=f"blocks.{i}.attn.proj")
        ln = b.layernorm(x, p["norm2.weight"], p["norm2.bias"], eps=1e-6, name=f"blocks.{i}.norm2")
        h = b.conv(ln, _pad2(p["mlp.fc1.weight"], hp, c).reshape(hp, c, 1, 1), _pad1(p["mlp.fc1.bias"], hp), name=f"blocks.{i}.mlp.fc1")
        h = b.gelu_add(h, name=f"blocks.{i}.mlp.act")
        x = b.conv(h, _pad2(p["mlp.fc2.weight"], c, hp).reshape(c, hp, 1, 1), _pad1(p["mlp.fc2.bias"], c), res1=x,
                   name=f"blocks.{i}.mlp.fc2")
    b.mark_output(b.layernorm(x, sd["Temporal_norm.weight"], sd["Temporal_norm.bias"], eps=1e-6, name="Temporal_norm"), "output")
    b.add_params("spatial_params", spatial_param_block(spec, sd))
    b.add_params("temporal_pos", np.asarray(sd["Temporal_pos_embed"], np.float32).reshape(f, d))
    b.add_params("head_params", head_param_block(spec, sd))
    return b.build()
