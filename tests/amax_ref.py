"""float64 restatement of the tiny programs of tests/test_gpu_amax.py.  TEST INFRASTRUCTURE ONLY.

`RefBuilder` has the methods of posepipeline_amd.program.ProgramBuilder that those programs use, with the same signatures, so that
ONE function states a program and is run twice: on a ProgramBuilder (what the GPU executes) and on a RefBuilder (numpy float64,
`run`).  The ops themselves are not restated here where a reference module already has them: the convolution is `conv64` of
tests/test_gpu_split.py, DCNv2 / the depthwise transposed convolution are tests/fairmot_ref.py's, LayerNorm / GELU / the depthwise
3x3 are tests/hrformer_ref.py's (torch, float64), the bilinear resize is tests/bottomup_ref.py's, attention is
tests/poseformer_ref.py's.

`run` also returns max |.| per sample of every buffer an op has just written: the covariance property of the GPU tests is only
claimed while those stay inside [2^-100, 2^100] (float32 normals, far from pp_amax_exp's clamp).

`peak_offset` says where a test puts a sample's largest element: the first float, the last float, or the float on a boundary of the
2048-float4 blocks of upsample_add_kernel / bilinear_add_kernel.
"""
from __future__ import annotations

import numpy as np
import torch

from posepipeline_amd import _lib as L
from tests import bottomup_ref, fairmot_ref, hrformer_ref, poseformer_ref
from tests.test_gpu_split import conv64

F64 = np.float64
BLOCK_FLOATS = 2048 * 4           # one block of the element-wise kernels: 256 threads x UA_R = 8 float4


def peak_offset(where, per, i, channels=None, c_min=0, coarse=None):
    """offset (in floats, inside the sample) of sample i's largest element; per: floats per sample of the dense [n][h][w][c] tensor
    that the producer kernel writes.
    'block': a float next to the first block boundary strictly inside the sample -- the block's first float for even i, the
    previous block's last float for odd i; the middle of the sample where no boundary falls inside it.
    channels / c_min: only channels >= c_min of the `channels` per pixel may hold the peak (the others are overwritten by an op):
    an offset on a lower channel moves to the pixel's channel c_min for 'first' and to the last channel of the pixel before it
    otherwise (for 'block': the previous block's last float).
    coarse = (H, W, C, u): the peak goes into a coarse input [H >> u][W >> u][C] of an up-sampling op whose output is [H][W][C]
    (per = H W C): the offset returned is that of the coarse pixel under the output pixel, same channel."""
    if where == "first":
        off = 0
    elif where == "last":
        off = per - 1
    else:
        assert where == "block", where
        b = (i * per // BLOCK_FLOATS + 1) * BLOCK_FLOATS          # first boundary > the sample's first float
        off = per // 2 if b >= (i + 1) * per else b - i * per - (i & 1)
    if channels is not None and off % channels < c_min:
        off = off + c_min if off < channels else off - off % channels - 1
    if coarse is not None:
        H, W, C, u = coarse
        assert per == H * W * C
        y, x, c = off // (W * C), off // C % W, off % C
        off = ((y >> u) * (W >> u) + (x >> u)) * C + c
    return off


class RefBuilder:
    def __init__(self):
        self.shapes = []
        self.named = {}
        self.fns = []          # (out buffer, fn(B) -> None)

    # ---- buffers ---------------------------------------------------------------------------------------------------------------
    def buf(self, h, w, c, name=None, pinned=False):
        self.shapes.append((int(h), int(w), int(c)))
        if name is not None:
            self.named[name] = len(self.shapes) - 1
        return len(self.shapes) - 1

    def dims(self, v):
        return self.shapes[v]

    def _out(self, out, h, w, c, off=0):
        if out is None:
            assert off == 0
            return self.buf(h, w, c)
        oh, ow, oc = self.shapes[out]
        assert (oh, ow) == (h, w) and off + c <= oc, (self.shapes[out], h, w, c, off)
        return out

    def _op(self, out, fn):
        self.fns.append((out, fn))
        return out

    # ---- ops -------------------------------------------------------------------------------------------------------------------
    def conv(self, x, weight, bias, *, stride=1, pad=0, relu=L.PP_RELU_NONE, res1=-1, out=None, out_c_off=0, name="conv"):
        w = np.asarray(weight, F64)
        cout, cin, kh, kw = w.shape
        assert isinstance(pad, int) and cin == self.shapes[x][2]
        b = np.zeros(cout, F64) if bias is None else np.asarray(bias, F64)
        h, wd, _ = self.shapes[x]
        out = self._out(out, (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1, cout, out_c_off)

        def fn(B):
            B[out][..., out_c_off:out_c_off + cout] = conv64(B[x], w, b, pad, stride, B[res1] if res1 >= 0 else None, relu)
        return self._op(out, fn)

    def maxpool(self, x, k, stride, pad, name="maxpool", out=None, out_c_off=0, in_c_off=0, c=None):
        h, w, cx = self.shapes[x]
        c = cx if c is None else c
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        out = self._out(out, ho, wo, c, out_c_off)

        def fn(B):
            xs = B[x][..., in_c_off:in_c_off + c]
            xp = np.full((xs.shape[0], h + 2 * pad, w + 2 * pad, c), -np.inf)
            xp[:, pad:pad + h, pad:pad + w] = xs
            y = np.full((xs.shape[0], ho, wo, c), -np.inf)
            for dy in range(k):
                for dx in range(k):
                    y = np.maximum(y, xp[:, dy:dy + (ho - 1) * stride + 1:stride, dx:dx + (wo - 1) * stride + 1:stride])
            B[out][..., out_c_off:out_c_off + c] = y
        return self._op(out, fn)

    def avgpool(self, x, kh, kw, stride=1, name="avgpool"):
        h, w, c = self.shapes[x]
        ho, wo = (h - kh) // stride + 1, (w - kw) // stride + 1
        out = self.buf(ho, wo, c)

        def fn(B):
            y = np.zeros((B[x].shape[0], ho, wo, c))
            for dy in range(kh):
                for dx in range(kw):
                    y += B[x][:, dy:dy + (ho - 1) * stride + 1:stride, dx:dx + (wo - 1) * stride + 1:stride]
            B[out][...] = y / (kh * kw)
        return self._op(out, fn)

    def upsample_add(self, t, *, up_log2, res1=-1, res2=-1, relu=L.PP_RELU_NONE, name="upsample_add", more=()):
        h, w, c = self.shapes[t]
        out = self.buf(h << up_log2, w << up_log2, c)
        terms = [(t, up_log2)] + list(more)

        def fn(B):
            y = B[res1].copy() if res1 >= 0 else 0.0
            for tb, u in terms:
                y = y + np.repeat(np.repeat(B[tb], 1 << u, axis=1), 1 << u, axis=2)
            if res2 >= 0:
                y = y + B[res2]
            B[out][...] = np.maximum(y, 0) if relu == L.PP_RELU_LAST else y
        return self._op(out, fn)

    def bilinear_add(self, t, *, up_log2, res1=-1, relu=L.PP_RELU_NONE, more=(), out=None, out_c_off=0, name="bilinear_add"):
        h, w, c = self.shapes[t]
        ho, wo = h << up_log2, w << up_log2
        out = self._out(out, ho, wo, c, out_c_off)
        terms = [(t, up_log2)] + list(more)

        def fn(B):
            y = B[res1].copy() if res1 >= 0 else 0.0
            for tb, _ in terms:      # F.interpolate(mode='bilinear', align_corners=False) on [n][c][h][w]
                y = y + np.transpose(bottomup_ref.resize(np.transpose(B[tb], (0, 3, 1, 2)), ho, wo, False, F64), (0, 2, 3, 1))
            B[out][..., out_c_off:out_c_off + c] = np.maximum(y, 0) if relu == L.PP_RELU_LAST else y
        return self._op(out, fn)

    def depth_to_space(self, x, name="depth_to_space"):
        h, w, c4 = self.shapes[x]
        c = c4 // 4
        out = self.buf(2 * h, 2 * w, c)

        def fn(B):
            for g in range(4):
                B[out][:, g // 2::2, g % 2::2] = B[x][..., g * c:(g + 1) * c]
        return self._op(out, fn)

    def dwconv3x3(self, x, weight, bias, *, stride=1, act=L.PP_RELU_NONE, gelu_in=False, name="dwconv3x3"):
        h, w, c = self.shapes[x]
        assert act == L.PP_RELU_NONE and not gelu_in and np.asarray(weight).shape[0] == c
        out = self.buf((h - 1) // stride + 1, (w - 1) // stride + 1, c)
        wt = torch.from_numpy(np.asarray(weight, F64))
        bt = torch.zeros(c, dtype=torch.float64) if bias is None else torch.from_numpy(np.asarray(bias, F64))

        def fn(B):
            B[out][...] = hrformer_ref.dwconv3x3_t(torch.from_numpy(B[x]), wt, bt, stride=stride).numpy()
        return self._op(out, fn)

    def layernorm(self, x, gamma, beta, *, eps=1e-6, name="layernorm"):
        h, w, c = self.shapes[x]
        assert np.asarray(gamma).size == c
        out = self.buf(h, w, c)
        g, b = torch.from_numpy(np.asarray(gamma, F64)), torch.from_numpy(np.asarray(beta, F64))

        def fn(B):
            B[out][...] = hrformer_ref.layernorm(torch.from_numpy(B[x]), g, b, eps).numpy()
        return self._op(out, fn)

    def gelu_add(self, x, *, res1=-1, name="gelu_add"):
        out = self.buf(*self.shapes[x])

        def fn(B):
            y = hrformer_ref.gelu(torch.from_numpy(B[x])).numpy()
            B[out][...] = y + B[res1] if res1 >= 0 else y
        return self._op(out, fn)

    def attention(self, qkv, *, c_real, heads, name="attention"):
        h, w, c3 = self.shapes[qkv]
        assert c3 == 3 * c_real
        out = self.buf(h, w, c_real)

        def fn(B):
            n = B[qkv].shape[0]
            B[out][...] = poseformer_ref.torch_attention(B[qkv].reshape(n, h * w, c3), heads, torch.float64).reshape(n, h, w, c_real)
        return self._op(out, fn)

    def dcn3x3(self, x, offset_mask, weight, bias, *, relu=L.PP_RELU_NONE, name="dcn3x3"):
        h, w, _ = self.shapes[x]
        wt = np.asarray(weight, F64)
        out = self.buf(h, w, wt.shape[0])

        def fn(B):
            for i in range(B[x].shape[0]):
                B[out][i] = fairmot_ref.dcn3x3(B[x][i], B[offset_mask][i], wt, None if bias is None else np.asarray(bias, F64),
                                               relu == L.PP_RELU_LAST)
        return self._op(out, fn)

    def dwdeconv(self, x, weight, stride, *, res1=-1, name="dwdeconv"):
        h, w, c = self.shapes[x]
        wt = np.asarray(weight, F64)
        assert wt.shape[0] == c
        out = self.buf(h * stride, w * stride, c)

        def fn(B):
            for i in range(B[x].shape[0]):
                y = fairmot_ref.dwdeconv(B[x][i], wt, stride)
                B[out][i] = y + B[res1][i] if res1 >= 0 else y
        return self._op(out, fn)

    # ---- evaluation ------------------------------------------------------------------------------------------------------------
    def run(self, inputs, out_name="output"):
        """inputs: {buffer name: [n][h][w][c]} (a named buffer that an op later writes a slice of keeps the rest of what it is given).
        Returns (the named output [n][h][w][c] float64, [max |.| per sample of the buffer each op wrote, in op order])."""
        n = next(iter(inputs.values())).shape[0]
        B = [np.zeros((n,) + s, F64) for s in self.shapes]
        for name, arr in inputs.items():
            assert arr.shape == B[self.named[name]].shape, (name, arr.shape)
            B[self.named[name]][...] = arr
        maxima = []
        for out, fn in self.fns:
            fn(B)
            maxima.append(np.abs(B[out]).reshape(n, -1).max(1))
        return B[self.named[out_name]], maxima
