"""References for the GAST-Net lifter, written apart from posepipeline_amd/models/gastnet.py: a numpy forward in the dtype of its
arguments (float64 in the tests) that evaluates SemCHGraphConv literally (the softmax per call, adj * E and adj * (1 - E)), and a torch
module with the same state-dict keys, in eval mode.  Tensors are (B, T, 17, C) in numpy and (B, C, T, 17) in torch, as in the
published model.  Both run the dilated whole-clip form: T_in frames give T_in - (rf - 1) output frames."""
import numpy as np
import torch
from torch import nn

J = 17
EDGES = [(1, 0), (2, 1), (3, 2), (4, 0), (5, 4), (6, 5), (7, 0), (8, 7), (9, 8), (10, 9), (11, 8), (12, 11), (13, 12), (14, 8), (15, 14),
         (16, 15)]
PAIRS = [(4, 1), (5, 2), (6, 3), (11, 14), (12, 15), (13, 16)]
END_JOINTS = [3, 6, 10, 13, 16]


def masks():
    a = np.eye(J)
    for c, p in EDGES:
        a[c, p] = a[p, c] = 1
    a = a / a.sum(1, keepdims=True)
    sym = np.eye(J)
    for l, r in PAIRS:
        sym[l, r] = sym[r, l] = 1
    a2 = a @ a
    con = np.zeros((J, J))
    for j in range(J):
        con[j] = a2[j] if j in END_JOINTS else a[j]
    return {"sym": sym > 0, "con": con > 0}


def as_dtype(sd, dtype):
    return {k: np.asarray(v, dtype) for k, v in sd.items()}


# ---- numpy ---------------------------------------------------------------------------------------------------------------------------
def _bn(x, sd, p, eps=1e-5):
    return (x - sd[p + ".running_mean"]) / np.sqrt(sd[p + ".running_var"] + x.dtype.type(eps)) * sd[p + ".weight"] + sd[p + ".bias"]


def _relu(x):
    return np.maximum(x, 0)


def _conv_t(x, w, dil=1):
    """x (B, T, J, Cin), w (Cout, Cin, k, 1) -> (B, T - dil (k - 1), J, Cout)"""
    k = w.shape[2]
    t_out = x.shape[1] - dil * (k - 1)
    return sum(x[:, i * dil:i * dil + t_out] @ w[:, :, i, 0].T for i in range(k))


def _softmax(a, axis):
    e = np.exp(a - a.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def sem_ch_graph_conv(x, w, e, bias, mask):
    """x (B, T, J, D) -> (B, T, J, D), literally"""
    h0, h1 = x @ w[0], x @ w[1]
    d = e.shape[0]
    adj = np.full((d, J, J), -9e15, x.dtype)
    adj[:, mask] = e
    adj = _softmax(adj, 2)
    eye = np.eye(J, dtype=x.dtype)
    return np.einsum("cji,btic->btjc", adj * eye, h0) + np.einsum("cji,btic->btjc", adj * (1 - eye), h1) + bias


def joint_attention(q, k, v):
    """(B, T, J, d) each -> softmax_j(q_i . k_j) v_j"""
    return _softmax(np.einsum("btid,btjd->btij", q, k), 3) @ v


def _gab(x, sd, p, heads, m):
    lg, gg = p + ".local_graph_layer", p + ".global_graph_layer"
    a = _relu(_bn(sem_ch_graph_conv(x, sd[lg + ".gcn_sym.W"], sd[lg + ".gcn_sym.e"], sd[lg + ".gcn_sym.bias"], m["sym"]), sd, lg + ".bn_1"))
    b = _relu(_bn(sem_ch_graph_conv(x, sd[lg + ".gcn_con.W"], sd[lg + ".gcn_con.e"], sd[lg + ".gcn_con.bias"], m["con"]), sd, lg + ".bn_2"))
    loc = _relu(_bn(_conv_t(np.concatenate([a, b], -1), sd[lg + ".cat_conv.weight"]), sd, lg + ".cat_bn"))
    outs = []
    for h in range(heads):
        q, k, v = (_conv_t(x, sd[f"{gg}.{n}.{h}.weight"]) + sd[f"{gg}.{n}.{h}.bias"] for n in ("theta", "phi", "g"))
        outs.append(joint_attention(q, k, v))
    glob = _relu(_bn(_conv_t(np.concatenate(outs, -1), sd[gg + ".cat_conv.weight"]), sd, gg + ".cat_bn"))
    return _relu(_bn(_conv_t(np.concatenate([x, loc, glob], -1), sd[p + ".cat_conv.weight"]), sd, p + ".cat_bn"))


def forward_np(x, sd, filter_widths, heads=4):
    """x (B, T_in, 17, 2) -> (B, T_in - (rf - 1), 17, 3), in x's dtype (sd in the same dtype)"""
    m = masks()
    x = _bn(x, sd, "init_bn")
    x = _relu(_bn(_conv_t(x, sd["expand_conv.weight"]), sd, "expand_bn"))
    x = _gab(x, sd, "layers_graph_conv.0", heads, m)
    dil = filter_widths[0]
    for i in range(1, len(filter_widths)):
        crop = dil * (filter_widths[i] // 2)
        res = x[:, crop:x.shape[1] - crop]
        x = _relu(_bn(_conv_t(x, sd[f"layers_conv.{2 * i - 2}.weight"], dil), sd, f"layers_bn.{2 * i - 2}"))
        x = res + _relu(_bn(_conv_t(x, sd[f"layers_conv.{2 * i - 1}.weight"]), sd, f"layers_bn.{2 * i - 1}"))
        x = _gab(x, sd, f"layers_graph_conv.{i}", heads, m)
        dil *= filter_widths[i]
    return _conv_t(x, sd["shrink.weight"])


def forward_windows_np(x, sd, filter_widths, heads=4):
    """the reference's form: one receptive field per output frame.  x (N + rf - 1, 17, 2) -> (N, 17, 3)"""
    rf = int(np.prod(filter_widths))
    return np.concatenate([forward_np(x[None, i:i + rf], sd, filter_widths, heads)[0] for i in range(x.shape[0] - rf + 1)])


# ---- torch ---------------------------------------------------------------------------------------------------------------------------
class SemCHGraphConv(nn.Module):
    def __init__(self, d, mask):
        super().__init__()
        self.register_buffer("mask", torch.from_numpy(mask), persistent=False)
        self.W = nn.Parameter(torch.zeros(2, d, d))
        self.e = nn.Parameter(torch.zeros(d, int(mask.sum())))
        self.bias = nn.Parameter(torch.zeros(d))

    def forward(self, x):                       # (B, T, J, D)
        h0, h1 = torch.matmul(x, self.W[0]), torch.matmul(x, self.W[1])
        adj = -9e15 * torch.ones(self.e.shape[0], J, J, dtype=x.dtype)
        adj[:, self.mask] = self.e
        adj = torch.softmax(adj, dim=2)
        eye = torch.eye(J, dtype=x.dtype)
        mix = lambda a, h: torch.einsum("cji,btic->btjc", a, h)      # noqa: E731
        return mix(adj * eye, h0) + mix(adj * (1 - eye), h1) + self.bias


class LocalGraph(nn.Module):
    def __init__(self, d, m):
        super().__init__()
        self.gcn_sym, self.gcn_con = SemCHGraphConv(d, m["sym"]), SemCHGraphConv(d, m["con"])
        self.bn_1, self.bn_2 = nn.BatchNorm2d(d), nn.BatchNorm2d(d)
        self.cat_conv, self.cat_bn = nn.Conv2d(2 * d, d, 1, bias=False), nn.BatchNorm2d(d)

    def forward(self, x):                       # (B, C, T, J)
        xl = x.permute(0, 2, 3, 1)
        a = torch.relu(self.bn_1(self.gcn_sym(xl).permute(0, 3, 1, 2)))
        b = torch.relu(self.bn_2(self.gcn_con(xl).permute(0, 3, 1, 2)))
        return torch.relu(self.cat_bn(self.cat_conv(torch.cat([a, b], 1))))


class GlobalGraph(nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        mk = lambda: nn.ModuleList([nn.Conv2d(d, d // heads, 1) for _ in range(heads)])      # noqa: E731
        self.theta, self.phi, self.g = mk(), mk(), mk()
        self.cat_conv, self.cat_bn = nn.Conv2d(d, d, 1, bias=False), nn.BatchNorm2d(d)

    def forward(self, x):
        outs = []
        for t, p, g in zip(self.theta, self.phi, self.g):
            q, k, v = (f(x).permute(0, 2, 3, 1) for f in (t, p, g))           # (B, T, J, d)
            outs.append(torch.matmul(torch.softmax(torch.matmul(q, k.transpose(2, 3)), dim=3), v).permute(0, 3, 1, 2))
        return torch.relu(self.cat_bn(self.cat_conv(torch.cat(outs, 1))))


class GraphAttentionBlock(nn.Module):
    def __init__(self, d, heads, m):
        super().__init__()
        self.local_graph_layer, self.global_graph_layer = LocalGraph(d, m), GlobalGraph(d, heads)
        self.cat_conv, self.cat_bn = nn.Conv2d(3 * d, 2 * d, 1, bias=False), nn.BatchNorm2d(2 * d)

    def forward(self, x):
        return torch.relu(self.cat_bn(self.cat_conv(torch.cat([x, self.local_graph_layer(x), self.global_graph_layer(x)], 1))))


class SpatioTemporalModel(nn.Module):
    def __init__(self, filter_widths, channels, heads=4):
        super().__init__()
        m = masks()
        fw, c = filter_widths, channels
        self.fw = tuple(fw)
        self.init_bn = nn.BatchNorm2d(2)
        self.expand_conv, self.expand_bn = nn.Conv2d(2, c, (fw[0], 1), bias=False), nn.BatchNorm2d(c)
        convs, bns, gabs = [], [], [GraphAttentionBlock(c, heads, m)]
        dil = fw[0]
        for i in range(1, len(fw)):
            ci = c * 2 ** i
            convs += [nn.Conv2d(ci, ci, (fw[i], 1), dilation=(dil, 1), bias=False), nn.Conv2d(ci, ci, 1, bias=False)]
            bns += [nn.BatchNorm2d(ci), nn.BatchNorm2d(ci)]
            gabs.append(GraphAttentionBlock(ci, heads, m))
            dil *= fw[i]
        self.layers_conv, self.layers_bn, self.layers_graph_conv = nn.ModuleList(convs), nn.ModuleList(bns), nn.ModuleList(gabs)
        self.shrink = nn.Conv2d(c * 2 ** len(fw), 3, 1, bias=False)

    def forward(self, x):                       # (B, T, J, 2) -> (B, T_out, J, 3)
        x = x.permute(0, 3, 1, 2)
        x = torch.relu(self.expand_bn(self.expand_conv(self.init_bn(x))))
        x = self.layers_graph_conv[0](x)
        dil = self.fw[0]
        for i in range(1, len(self.fw)):
            crop = dil * (self.fw[i] // 2)
            res = x[:, :, crop:x.shape[2] - crop]
            x = torch.relu(self.layers_bn[2 * i - 2](self.layers_conv[2 * i - 2](x)))
            x = res + torch.relu(self.layers_bn[2 * i - 1](self.layers_conv[2 * i - 1](x)))
            x = self.layers_graph_conv[i](x)
            dil *= self.fw[i]
        return self.shrink(x).permute(0, 2, 3, 1)


def torch_model(sd, filter_widths, channels, dtype, heads=4):
    model = SpatioTemporalModel(filter_widths, channels, heads).to(dtype)
    res = model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys), res
    return model.eval()


def torch_forward(x, sd, filter_widths, channels, dtype, heads=4):
    """x (B, T_in, 17, 2) numpy -> numpy (B, T_out, 17, 3) evaluated by torch on the CPU in `dtype`"""
    with torch.no_grad():
        return torch_model(sd, filter_widths, channels, dtype, heads)(torch.from_numpy(np.ascontiguousarray(x)).to(dtype)).numpy()
