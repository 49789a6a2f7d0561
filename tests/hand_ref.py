"""CPU restatement of the hand stage.  TEST INFRASTRUCTURE ONLY.

  * `bilinear_up` / `bilinear_add`: PP_OP_BILINEAR_ADD (include/posepipe_hip.h) in numpy float32 -- the same products and
    sums in the same order, each rounded to float32, so the GPU op can be compared with `==`;
  * `HRNetV2Ref`: mmpose 0.x HRNet with multiscale_output, bilinear fuse upsampling and the resize_concat two-layer head
    (posepipeline_amd/models/hrnetv2.py states the architecture; UNPINNED, the mmpose hand configs are not in the reference
    tree), on the UNPADDED channel counts: every conv is oracle/conv_ref.c (fmaf chain over (kh, kw, cin)) on BN-folded
    weights, as in oracle/nets.py whose stem / block code this class inherits;
  * `hand_chain`: hand boxes -> oracle crop -> HRNetV2Ref -> oracle flip-merge + decode, what the wrapper test compares with.
"""
from __future__ import annotations

import numpy as np

from oracle import clib
from oracle import nets as onets
from oracle.nets import relu

F32 = np.float32


def _axis(n_out, u, n_src):
    """source rows and weights of output rows 0 .. n_out - 1 for the factor 2^u (exact in float32: dyadic fractions)"""
    i = np.arange(n_out, dtype=F32)
    s = np.maximum((i + F32(0.5)) * F32(2.0 ** -u) - F32(0.5), F32(0))
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_src - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def bilinear_up(x, u):
    """x [n][h][w][c] float32 -> [n][h << u][w << u][c]: ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11)"""
    x = np.asarray(x, F32)
    n, h, w, c = x.shape
    y0, y1, ly0, ly1 = _axis(h << u, u, h)
    x0, x1, lx0, lx1 = _axis(w << u, u, w)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    ly0, ly1 = ly0[None, :, None, None], ly1[None, :, None, None]
    r0, r1 = x[:, y0], x[:, y1]
    top = lx0 * r0[:, :, x0] + lx1 * r0[:, :, x1]
    bot = lx0 * r1[:, :, x0] + lx1 * r1[:, :, x1]
    out = ly0 * top + ly1 * bot
    assert out.dtype == F32
    return out


def bilinear_add(terms, res1=None, relu_last=False):
    """act(((res1 + B(t)) + B(t2)) + B(t3)); terms: [(array, up_log2), ...]"""
    y = None if res1 is None else np.asarray(res1, F32)
    for t, u in terms:
        b = bilinear_up(t, u)
        y = b if y is None else y + b
    return relu(y) if relu_last else y


class HRNetV2Ref(onets.HRNetRef):
    def __init__(self, sd, width=18, num_joints=21, stages=((1, 2), (4, 3), (3, 4)), blocks=4):
        super().__init__(sd, width, num_joints, stages, blocks)

    def module(self, xs, mp, n_out):
        n_br = len(xs)
        xs = list(xs)
        for b in range(n_br):
            for k in range(self.blocks):
                xs[b] = self.basic(xs[b], f"{mp}branches.{b}.{k}.")
        outs = []
        for i in range(n_out):
            y = 0
            for j in range(n_br):
                f = f"{mp}fuse_layers.{i}.{j}."
                if i == j:
                    t = xs[j]
                elif j > i:      # conv1x1 + BN, nn.Upsample(scale_factor=2^(j-i), mode='bilinear', align_corners=False)
                    t = bilinear_up(self.cb(xs[j], f + "0", f + "1", pad=0), j - i)
                else:
                    t = xs[j]
                    for k in range(i - j):
                        t = self.cb(t, f"{f}{k}.0", f"{f}{k}.1", stride=2)
                        if k != i - j - 1:
                            t = relu(t)
                y = y + t
            outs.append(relu(y))
        return outs

    def forward(self, x_nchw):
        """x [n][3][h][w] float32 -> heatmaps [n][K][h/4][w/4]."""
        x = np.ascontiguousarray(np.transpose(np.asarray(x_nchw, F32), (0, 2, 3, 1)))
        B = "backbone."
        x = relu(self.cb(x, B + "conv1", B + "bn1", stride=2))
        x = relu(self.cb(x, B + "conv2", B + "bn2", stride=2))
        for i in range(4):
            x = self.bottleneck(x, f"{B}layer1.{i}.", i == 0)
        ch = [self.width * 2 ** i for i in range(4)]
        ys, pre = [x], [256]
        for si, (n_mod, n_br) in enumerate(self.stages):
            cur = ch[:n_br]
            t = f"{B}transition{si + 1}."
            xs = []
            for i in range(n_br):
                if i < len(pre):
                    xs.append(relu(self.cb(ys[i], f"{t}{i}.0", f"{t}{i}.1")) if pre[i] != cur[i] else ys[i])
                else:
                    y = ys[-1]
                    for j in range(i + 1 - len(pre)):
                        y = relu(self.cb(y, f"{t}{i}.{j}.0", f"{t}{i}.{j}.1", stride=2))
                    xs.append(y)
            for m in range(n_mod):
                xs = self.module(xs, f"{B}stage{si + 2}.{m}.", n_br)       # multiscale_output: every module fuses to all branches
            ys, pre = xs, cur
        # resize_concat: bilinear (align_corners=False) to the first branch's size -- the identity for that branch -- and concatenate
        cat = np.ascontiguousarray(np.concatenate([ys[0]] + [bilinear_up(ys[i], i) for i in range(1, len(ys))], axis=3))
        sd = self.sd
        H = "keypoint_head.final_layer."
        scale = sd[H + "1.weight"].astype(np.float64) / np.sqrt(sd[H + "1.running_var"].astype(np.float64) + 1e-5)
        w0 = (sd[H + "0.weight"].astype(np.float64) * scale[:, None, None, None]).astype(F32)
        b0 = (sd[H + "1.bias"].astype(np.float64) + (sd[H + "0.bias"].astype(np.float64) - sd[H + "1.running_mean"].astype(np.float64)) * scale).astype(F32)
        y = relu(clib.conv2d_nhwc(cat, w0, b0))
        hm = clib.conv2d_nhwc(y, sd[H + "3.weight"], sd[H + "3.bias"])
        return np.ascontiguousarray(np.transpose(hm, (0, 3, 1, 2)))


def hand_chain(sd, spec, frames_bgr, boxes_xyxy, post, kernel=11):
    """The CPU chain of the hand wrapper: for every frame and each of its two boxes, oracle crop (mmpose 1.x hands the model
    the BGR frame and swaps ONCE, so the frame goes in where the body chain passes its RGB copy) -> HRNetV2Ref on the crop and
    its mirror image -> oracle flip-merge (identity permutation) + DARK (post 'unbiased', shifted flip map) or DARK-UDP decode.
    Returns float32 [T][42][3]."""
    from oracle import decode as odec
    from oracle import preprocess as opre
    model = HRNetV2Ref(sd, spec.width, spec.num_joints, spec.stages, spec.blocks_per_branch)
    size = (spec.in_w, spec.in_h)
    out = np.zeros((len(frames_bgr), 2 * spec.num_joints, 3), F32)
    for t, (fr, boxes) in enumerate(zip(frames_bgr, np.asarray(boxes_xyxy, np.float64))):
        for b, (x1, y1, x2, y2) in enumerate(boxes):
            tlwh = np.array([x1, y1, x2 - x1, y2 - y1])
            crop_fn = opre.top_down_input_udp if post == "udp" else opre.top_down_input
            x, c, s, _ = crop_fn(fr, tlwh, size)
            hm = model.forward(np.stack([x, x[:, :, ::-1]]))
            if post == "udp":
                k, _ = odec.decode_topdown_udp(hm[:1], hm[1:], [], c[None], s[None], kernel=kernel)
            else:
                k, _ = odec.decode_topdown(hm[:1], hm[1:], [], c[None], s[None], post_process=post, kernel=kernel, shift_heatmap=True)
            out[t, b * spec.num_joints:(b + 1) * spec.num_joints] = k[0]
    return out
