"""References for PoseFormer (posepipeline_amd/models/poseformer.py), written apart from the library code:

  * a numpy forward in the dtype of its arguments (float64 in the tests), in two forms -- `forward_windows` evaluates the whole
    network per 81-frame window, as the reference wrapper does; `forward_clip` evaluates the spatial stage once per frame of the
    clip and only the temporal stage per window, as the device code does;
  * `PoseTransformerT`, an independently written torch module (nn.Linear, nn.LayerNorm, F.gelu, softmax, nn.Conv1d) with the
    state-dict keys of the published model, in inference mode.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

F_WIN, J, R, D, HEADS, DEPTH = 81, 17, 32, 544, 8, 4


def _erf(x):
    """erf in x's dtype (numpy has none; torch's is correctly rounded to well under the tolerances used with it)"""
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


# ---- numpy --------------------------------------------------------------------------------------------------------------------
def layernorm_np(x, g, b, eps):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def gelu_np(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def attention_np(qkv, heads):
    """qkv [..., T, 3 * dim] with channel s * dim + head * hd + d -> [..., T, dim]"""
    t, dim = qkv.shape[-2], qkv.shape[-1] // 3
    hd = dim // heads
    q, k, v = np.moveaxis(qkv.reshape(qkv.shape[:-1] + (3, heads, hd)), -3, 0)       # each [..., T, heads, hd]
    q, k, v = (np.swapaxes(a, -3, -2) for a in (q, k, v))                             # [..., heads, T, hd]
    s = (q @ np.swapaxes(k, -1, -2)) * hd ** -0.5
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    return np.swapaxes(p @ v, -3, -2).reshape(qkv.shape[:-2] + (t, dim))


def block_np(x, sd, prefix, heads):
    g = lambda n: sd[prefix + n]
    h = layernorm_np(x, g("norm1.weight"), g("norm1.bias"), 1e-6)
    a = attention_np(h @ g("attn.qkv.weight").T + g("attn.qkv.bias"), heads)
    x = x + (a @ g("attn.proj.weight").T + g("attn.proj.bias"))
    h = layernorm_np(x, g("norm2.weight"), g("norm2.bias"), 1e-6)
    h = gelu_np(h @ g("mlp.fc1.weight").T + g("mlp.fc1.bias"))
    return x + (h @ g("mlp.fc2.weight").T + g("mlp.fc2.bias"))


def spatial_np(x, sd):
    """x [n][17][2] -> features [n][544]"""
    h = x @ sd["Spatial_patch_to_embedding.weight"].T + sd["Spatial_patch_to_embedding.bias"] + sd["Spatial_pos_embed"][0]
    for i in range(DEPTH):
        h = block_np(h, sd, f"Spatial_blocks.{i}.", HEADS)
    h = layernorm_np(h, sd["Spatial_norm.weight"], sd["Spatial_norm.bias"], 1e-6)
    return h.reshape(x.shape[0], J * R)


def temporal_np(feat, sd):
    """feat [b][81][544] (windows of features) -> [b][17][3]"""
    h = feat + sd["Temporal_pos_embed"][0]
    for i in range(DEPTH):
        h = block_np(h, sd, f"blocks.{i}.", HEADS)
    h = layernorm_np(h, sd["Temporal_norm.weight"], sd["Temporal_norm.bias"], 1e-6)
    # every product below is a stack of per-sample matrices: a sample's result does not depend on the batch it shares
    y = (sd["weighted_mean.weight"].reshape(1, -1, 1) * h).sum(axis=1, keepdims=True) + sd["weighted_mean.bias"][0]     # [b][1][544]
    y = layernorm_np(y, sd["head.0.weight"], sd["head.0.bias"], 1e-5)
    return (y @ sd["head.1.weight"].T + sd["head.1.bias"]).reshape(-1, J, 3)


def forward_windows(x, sd):
    """the reference's form: the whole network per window.  x [n][17][2], n >= 81 -> [n - 80][17][3]"""
    out = []
    for i in range(x.shape[0] - F_WIN + 1):
        out.append(temporal_np(spatial_np(x[i:i + F_WIN], sd)[None], sd)[0])
    return np.stack(out)


def forward_clip(x, sd, batch=16):
    """the device's form: the spatial stage once per frame of the clip, the temporal stage per window"""
    feat = spatial_np(x, sd)
    n_win = x.shape[0] - F_WIN + 1
    out = []
    for i0 in range(0, n_win, batch):
        wins = np.stack([feat[i:i + F_WIN] for i in range(i0, min(i0 + batch, n_win))])
        out.append(temporal_np(wins, sd))
    return np.concatenate(out)


def as_dtype(sd, dt):
    return {k: np.asarray(v).astype(dt) for k, v in sd.items()}


# ---- torch --------------------------------------------------------------------------------------------------------------------
class _Attn(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        b, t, c = x.shape
        qkv = self.qkv(x).reshape(b, t, 3, self.heads, c // self.heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        a = ((q @ k.transpose(-2, -1)) * (c // self.heads) ** -0.5).softmax(dim=-1)
        return self.proj((a @ v).transpose(1, 2).reshape(b, t, c))


class _Mlp(nn.Module):
    def __init__(self, dim, hid):
        super().__init__()
        self.fc1 = nn.Linear(dim, hid)
        self.fc2 = nn.Linear(hid, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, dim, heads, ratio=2.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attn(dim, heads)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, int(dim * ratio))

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class PoseTransformerT(nn.Module):
    """inference-mode PoseFormer: (b, 81, 17, 2) -> (b, 1, 17, 3)"""

    def __init__(self):
        super().__init__()
        self.Spatial_patch_to_embedding = nn.Linear(2, R)
        self.Spatial_pos_embed = nn.Parameter(torch.zeros(1, J, R))
        self.Temporal_pos_embed = nn.Parameter(torch.zeros(1, F_WIN, D))
        self.Spatial_blocks = nn.ModuleList([_Block(R, HEADS) for _ in range(DEPTH)])
        self.blocks = nn.ModuleList([_Block(D, HEADS) for _ in range(DEPTH)])
        self.Spatial_norm = nn.LayerNorm(R, eps=1e-6)
        self.Temporal_norm = nn.LayerNorm(D, eps=1e-6)
        self.weighted_mean = nn.Conv1d(F_WIN, 1, kernel_size=1)
        self.head = nn.Sequential(nn.LayerNorm(D), nn.Linear(D, J * 3))

    def spatial(self, x):
        b, f = x.shape[:2]
        h = self.Spatial_patch_to_embedding(x.reshape(b * f, J, 2)) + self.Spatial_pos_embed
        for blk in self.Spatial_blocks:
            h = blk(h)
        return self.Spatial_norm(h).reshape(b, f, D)

    def temporal(self, h):
        h = h + self.Temporal_pos_embed
        for blk in self.blocks:
            h = blk(h)
        return self.weighted_mean(self.Temporal_norm(h))          # (b, 1, D)

    def forward(self, x):
        b = x.shape[0]
        return self.head(self.temporal(self.spatial(x))).reshape(b, 1, J, 3)


def torch_model(sd, dtype):
    m = PoseTransformerT()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dtype).eval()


@torch.no_grad()
def torch_forward_windows(x, sd, dtype):
    """x [n][17][2] -> [n - 80][17][3] with the torch module, one window per sample"""
    m = torch_model(sd, dtype)
    xt = torch.from_numpy(np.asarray(x)).to(dtype)
    wins = torch.stack([xt[i:i + F_WIN] for i in range(xt.shape[0] - F_WIN + 1)])
    return torch.cat([m(wins[i:i + 8]) for i in range(0, wins.shape[0], 8)])[:, 0].numpy()


@torch.no_grad()
def torch_spatial(x, sd, dtype):
    m = torch_model(sd, dtype)
    return m.spatial(torch.from_numpy(np.asarray(x)).to(dtype)[None])[0].numpy()


def torch_attention(qkv, heads, dtype):
    """qkv [b][t][3 * dim] -> [b][t][dim] by torch ops"""
    q = torch.from_numpy(np.asarray(qkv)).to(dtype)
    b, t, c3 = q.shape
    c = c3 // 3
    q = q.reshape(b, t, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
    a = ((q[0] @ q[1].transpose(-2, -1)) * (c // heads) ** -0.5).softmax(dim=-1)
    return (a @ q[2]).transpose(1, 2).reshape(b, t, c).numpy()
