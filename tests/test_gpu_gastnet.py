"""GAST-Net lifting on the GPU: the two new ops alone, their per-sample maxima in front of a fp16-form convolution, the whole lift in
both numerics, the wrapper on the table shim with a checkpoint file, and the full-size program, against tests/gastnet_ref.py.

Tolerance (the rule of tests/test_gpu_poseformer.py): in each test `dev32` is the largest deviation, on that test's inputs and weights,
of the torch float32 CPU evaluation from the float64 reference; the GPU result must lie within FACTOR = 4 x dev32 of the float64
reference.  The measured ratios are printed and recorded in DESIGN_LOG.md 5p.
"""
import datetime
import os

import numpy as np
import pytest
import torch

from posepipeline_amd import _lib as L
from posepipeline_amd.models import gastnet as M
from posepipeline_amd.program import Net, ProgramBuilder
from posepipeline_amd.wrappers import gastnet as W
from tests import gastnet_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0
F32, F64 = np.float32, np.float64
SMALL = M.GastNetSpec(channels=16, filter_widths=(3, 3, 3), chunk=8)
FULL8 = M.GastNetSpec(chunk=8)


def _check(got, ref32, ref64, what):
    dev = float(np.abs(np.asarray(ref32, F64) - ref64).max())
    err = float(np.abs(np.asarray(got, F64) - ref64).max())
    assert dev > 0, what
    print(f"{what}: GPU vs float64 {err:.3e}, float32-on-CPU vs float64 (dev32) {dev:.3e}, ratio {err / dev:.2f} (bound {FACTOR:g}), "
          f"max |ref| {np.abs(ref64).max():.3g}")
    assert err <= FACTOR * dev, (what, err, dev, err / dev)


def _run(ctx, prog, x, numerics="exact", sentinel=None):
    """one forward of a program with "input" and "output"; sentinel: what the output buffer holds beforehand"""
    net = Net(ctx, prog, max_batch=x.shape[0], numerics=numerics)
    try:
        if sentinel is not None:
            h, w, c = prog.bufs[prog.named["output"]]
            ctx.h2d(net.buffer("output")[0], np.full((x.shape[0], h, w, c), sentinel, F32))
        return net.forward(x)
    finally:
        net.close()


# ---- 1. PP_OP_GRAPH_MIX alone ------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64; the float64 sum is rounded TO ODD (TwoSum gives the residual), so that
    the second rounding, to float32, is the rounding of the exact a * b + c (53 >= 24 + 2 bits)"""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def graph_mix_f32(x, mats, biases, masks, relu):
    """the documented order in float32: per output joint one fmaf chain from 0 over the mask's source joints ascending (h0 on the
    diagonal, h1 off it), then one add of the bias.  x (B, 17, w, 2 g c) -> (B, 17, w, g c)"""
    g, c = len(mats), mats[0].shape[2]
    out = np.empty(x.shape[:3] + (g * c,), F32)
    for q in range(g):
        h0, h1 = x[..., 2 * q * c:2 * q * c + c], x[..., 2 * q * c + c:2 * q * c + 2 * c]
        for j in range(17):
            acc = np.zeros(x.shape[:1] + x.shape[2:3] + (c,), F32)
            for i in np.flatnonzero(masks[q][j]):
                acc = fma32(np.broadcast_to(mats[q][j, i], acc.shape), (h0 if i == j else h1)[:, i], acc)
            acc = acc + biases[q]
            out[:, j, :, q * c:(q + 1) * c] = np.maximum(acc, 0) if relu else acc
    return out


@pytest.mark.parametrize("c,w,relu,off", [(16, 5, False, 0), (16, 70, True, 0), (20, 5, True, 8), (20, 70, False, 8)],
                         ids=["c16_w5", "c16_w70_relu", "c20_w5_relu_off8", "c20_w70_off8"])
def test_graph_mix_op(ctx, c, w, relu, off):
    """`==` against the float32 evaluation in the documented fmaf order: the op has no transcendental and one summation order, and
    fma32 above is an exact fmaf, so nothing is left to a tolerance.  70 time steps of 2 graphs x c / 4 float4 are more than one
    workgroup of 256 threads per sample, and at c = 20 waves straddle two graphs (their lanes carry different masks)."""
    rng = np.random.default_rng(100 * c + w)
    gm = M.graph_masks()
    masks = [gm["sym"], gm["con"]]
    mats = [np.where(m[:, :, None], rng.standard_normal((17, 17, c)), 0).astype(F32) for m in masks]
    biases = [rng.standard_normal(c).astype(F32) for _ in masks]
    x = rng.standard_normal((2, 17, w, 4 * c)).astype(F32)
    pb = ProgramBuilder()
    xin = pb.buf(17, w, 4 * c, name="input")
    kw = dict(relu=L.PP_RELU_LAST if relu else L.PP_RELU_NONE, name="mix")
    if off:
        pb.graph_mix(xin, mats, biases, masks, out=pb.buf(17, w, off + 2 * c + 4, name="output"), out_c_off=off, **kw)
    else:
        pb.mark_output(pb.graph_mix(xin, mats, biases, masks, **kw), "output")
    got = _run(ctx, pb.build(), x, sentinel=7.0)
    want = graph_mix_f32(x, mats, biases, masks, relu)
    mixed = got[..., off:off + 2 * c]
    print(f"graph_mix c={c} w={w}: max |GPU - float32 chain| {np.abs(mixed - want).max():.3e}, max |ref| {np.abs(want).max():.3g}")
    assert np.array_equal(mixed, want)
    assert (got[..., :off] == 7.0).all() and (got[..., off + 2 * c:] == 7.0).all()         # the other channels: untouched
    if relu:
        assert (mixed >= 0).all() and (mixed == 0).any()


# ---- 2. PP_OP_JOINT_ATTN alone -----------------------------------------------------------------------------------------------------
def _joint_attn_ref(real, heads, dtype):
    """real (B, 17, w, 3 c) numpy -> (B, 17, w, c): numpy in float64, torch on the CPU in float32"""
    b, j, w, c3 = real.shape
    c = c3 // 3
    q, k, v = (real[..., s * c:(s + 1) * c].reshape(b, j, w, heads, c // heads).transpose(0, 2, 3, 1, 4) for s in range(3))   # (B, w, heads, 17, hd)
    if dtype is F64:
        out = R.joint_attention(*(a.reshape((-1,) + a.shape[2:]).astype(F64) for a in (q, k, v))).reshape(q.shape)
    else:
        tq, tk, tv = (torch.from_numpy(np.ascontiguousarray(a)) for a in (q, k, v))
        out = torch.matmul(torch.softmax(torch.matmul(tq, tk.transpose(3, 4)), dim=4), tv).numpy()
    return out.transpose(0, 3, 1, 2, 4).reshape(b, j, w, c)


@pytest.mark.parametrize("hd,w,c_pad,off", [(4, 3, 8, 0), (4, 70, 0, 0), (128, 3, 0, 0), (128, 70, 8, 4)],
                         ids=["hd4_w3_pad8", "hd4_w70", "hd128_w3", "hd128_w70_pad8_off4"])
def test_joint_attn_op(ctx, hd, w, c_pad, off):
    """The 4 x dev32 rule, not `==`: exp is evaluated in double by the device's library and by numpy's, which need not round alike, and
    the quotient e / sum carries that on.  Sample 0, time step 0 holds, in head 0, a query row of zeros (equal logits: the plain mean of
    v) and, in head 1, a key 40 times the others (softmax ~ one-hot).  hd = 128 is the widest head of either published model; 70 time
    steps are more than one workgroup (4 or 2 time steps each)."""
    heads = 4
    c = heads * hd
    c_buf = c + c_pad
    rng = np.random.default_rng(10 * hd + w)
    qkv = rng.standard_normal((2, 17, w, 3, c_buf)).astype(F32)               # the padding channels hold garbage: never read
    qkv[..., :2, :] *= F32(hd ** -0.25)                                       # logits of order one at either head dim
    qkv[0, 5, 0, 0, 0:hd] = 0                                                 # head 0, query joint 5: equal logits
    qkv[0, 9, 0, 1, hd:2 * hd] = 40 * np.sign(qkv[0, 3, 0, 0, hd:2 * hd])     # head 1, key joint 9 dominates query joint 3 (logit ~ 40 sum |q|)
    real = np.ascontiguousarray(qkv[..., :c]).reshape(2, 17, w, 3 * c)
    pb = ProgramBuilder()
    xin = pb.buf(17, w, 3 * c_buf, name="input")
    if off:
        pb.joint_attention(xin, c_real=c, heads=heads, out=pb.buf(17, w, off + c_buf + 4, name="output"), out_c_off=off)
    else:
        pb.mark_output(pb.joint_attention(xin, c_real=c, heads=heads), "output")
    got = _run(ctx, pb.build(), qkv.reshape(2, 17, w, 3 * c_buf), sentinel=7.0)
    ref64, ref32 = _joint_attn_ref(real, heads, F64), _joint_attn_ref(real, heads, F32)
    _check(got[..., off:off + c], ref32, ref64, f"joint_attn hd={hd} w={w} c_buf={c_buf} off={off}")
    v = real[..., 2 * c:].astype(F64)
    assert np.abs(ref64[0, 5, 0, :hd] - v[0, :, 0, :hd].mean(0)).max() < 1e-12                       # the equal-logit row: the mean of v
    assert np.abs(ref64[0, 3, 0, hd:2 * hd] - v[0, 9, 0, hd:2 * hd]).max() < 1e-6                    # the dominant row: v of joint 9
    assert np.abs(got[0, 3, 0, off + hd:off + 2 * hd] - v[0, 9, 0, hd:2 * hd]).max() < 1e-5
    assert not got[..., off + c:off + c_buf].any()                                                  # padding channels: exact zeros
    assert (got[..., :off] == 7.0).all() and (got[..., off + c_buf:] == 7.0).all()                   # beyond the slice: untouched
    assert np.isfinite(got).all()


# ---- 3. per-sample maxima of both ops in front of a fp16-form convolution ----------------------------------------------------------
def _amax_program(kind, rng):
    pb = ProgramBuilder()
    if kind == "graph_mix":
        gm = M.graph_masks()
        masks = [gm["sym"], gm["con"]]
        mats = [np.where(m[:, :, None], rng.standard_normal((17, 17, 32)) / 2, 0).astype(F32) for m in masks]
        y = pb.graph_mix(pb.buf(17, 6, 128, name="input"), mats, [np.zeros(32, F32)] * 2, masks, name="mix")
    else:
        y = pb.joint_attention(pb.buf(17, 6, 192, name="input"), c_real=64, heads=4, name="attn")
    wt = (rng.standard_normal((128, 64, 1, 1)) / 8).astype(F32)
    pb.conv(y, wt, None, out=pb.buf(17, 6, 128, name="output"), name="reader")
    return pb.build(), wt


@pytest.mark.parametrize("kind", ["graph_mix", "joint_attn"])
def test_ops_feed_the_fp16_form(ctx, kind):
    """producer op -> 1x1 convolution on the split product kernel in the fp16 form: the reader scales each sample by a power of two
    from the maxima the net takes behind the op (pp_amax.h).  Samples 2^40 apart in magnitude give, together, bit for bit what each
    gives alone and what a fresh net gives after a run on other data (a maximum that is stale, shared between samples or missing
    changes bits or overflows float16); and each sample is as close to float64, relative to its own range, as float32 is."""
    rng = np.random.default_rng(17)
    prog, wt = _amax_program(kind, rng)
    c_in = prog.bufs[prog.named["input"]][2]
    x = rng.standard_normal((2, 17, 6, c_in)).astype(F32)
    if kind == "graph_mix":
        x[0] *= F32(2.0 ** 20)
        x[1] *= F32(2.0 ** -20)
    else:                                   # the magnitude of an attention output is that of v
        x[0, ..., 128:] *= F32(2.0 ** 20)
        x[1, ..., 128:] *= F32(2.0 ** -20)
    net = Net(ctx, prog, max_batch=2, numerics="split_f16")
    try:
        assert net.split_kind == "split_f16" and net.conv_kinds().tolist() == [0, 2]
        both = net.forward(x)
        alone = [net.forward(x[i:i + 1])[0] for i in (0, 1)]
        swapped = net.forward(x[::-1].copy())
        again = net.forward(x)
    finally:
        net.close()
    assert np.isfinite(both).all()
    for i in (0, 1):
        assert np.array_equal(both[i], alone[i]) and np.array_equal(both[i], swapped[1 - i]), i
    assert np.array_equal(both, again)
    exact = _run(ctx, prog, x, numerics="exact")
    x64 = x.astype(F64)
    if kind == "graph_mix":
        op = prog.ops[0]
        mats = prog.blob[op.w_off:op.w_off + 2 * 289 * 32].reshape(2, 17, 17, 32).astype(F64)
        eye = np.eye(17)[:, :, None]
        mid = np.concatenate([np.einsum("jic,bitc->bjtc", mats[q] * eye, x64[..., 64 * q:64 * q + 32]) +
                              np.einsum("jic,bitc->bjtc", mats[q] * (1 - eye), x64[..., 64 * q + 32:64 * q + 64]) for q in (0, 1)], -1)
    else:
        mid = _joint_attn_ref(x, 4, F64)
    ref64 = mid @ wt[:, :, 0, 0].astype(F64).T
    for i in (0, 1):
        rng_i = np.abs(ref64[i]).max()
        e_split, e_exact = np.abs(both[i] - ref64[i]).max() / rng_i, np.abs(exact[i] - ref64[i]).max() / rng_i
        print(f"{kind} -> fp16-form reader, sample {i}: error / range split {e_split:.3e}, exact {e_exact:.3e}")
        assert e_split <= 1.5 * e_exact + 1e-7, (i, e_split, e_exact)


# ---- 4. the lift -------------------------------------------------------------------------------------------------------------------
def _ref_lift(x, sd, spec, flip, dtype):
    """whole-clip reference of the lifter: edge padding, one dilated pass (float64: numpy; float32: torch on the CPU), flip merge"""
    xp = np.pad(np.asarray(x, F32), ((spec.pad, spec.pad), (0, 0), (0, 0)), mode="edge")
    if dtype is F64:
        sd64 = R.as_dtype(sd, F64)
        fwd = lambda a: R.forward_np(a[None].astype(F64), sd64, spec.filter_widths, spec.heads)[0]         # noqa: E731
    else:
        fwd = lambda a: R.torch_forward(a[None], sd, spec.filter_widths, spec.channels, torch.float32, spec.heads)[0]   # noqa: E731
    y = fwd(xp)
    if flip:
        y = (y + W.mirror_output(fwd(W.mirror_input(xp)))) / y.dtype.type(2)
    return y


@pytest.fixture(scope="module")
def sd_small():
    return M.synth_params(M.gastnet_param_shapes(SMALL), seed=3)


@pytest.fixture(scope="module")
def clip(sd_small):
    """one seeded clip of 11 valid frames (one full chunk of 8 and a ragged one of 3) and its references, computed once"""
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (11, 17, 2)).astype(F32)
    refs = {flip: (_ref_lift(x, sd_small, SMALL, flip, F64), _ref_lift(x, sd_small, SMALL, flip, F32)) for flip in (False, True)}
    x.setflags(write=False)
    for a, b in refs.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return x, refs


@pytest.mark.parametrize("numerics", ["exact", "split"])
@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
def test_lift(ctx, sd_small, clip, numerics, flip):
    x, refs = clip
    ref64, ref32 = refs[flip]
    lf = W.GastNetLifter(numerics=numerics, ctx=ctx, state_dict=sd_small, spec=SMALL, flip_augment=flip)
    try:
        assert lf.net.numerics == numerics and lf.net.max_batch == 2
        got = lf.lift(x)
        assert got.shape == (11, 17, 3) and got.dtype == F32 and lf.stage_ms is None
        _check(got, ref32, ref64, f"lift 11 frames, channels 16, {numerics}, flip {flip}")
        assert np.array_equal(lf.lift(x), got), "two runs differ"
        # a frame's result does not depend on the chunk it falls in: the clip without its first frame shifts every chunk
        if numerics == "exact":
            assert np.array_equal(lf.lift(np.concatenate([x[:1], x]))[2:], got[1:])
        timed = lf.lift(x, timed=True)
        assert np.array_equal(timed, got) and set(lf.stage_ms) == {"upload", "program", "post"} and lf.stage_ms["program"] > 0, lf.stage_ms
        with pytest.raises(ValueError, match="17"):
            lf.lift(np.zeros((4, 16, 2), F32))
        with pytest.raises(ValueError, match="no valid frame"):
            lf.lift(np.zeros((0, 17, 2), F32))
    finally:
        lf.close()


# ---- 5. the full-size program ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd_full():
    return M.synth_params(M.gastnet_param_shapes(M.GastNetSpec()), seed=7)


@pytest.mark.parametrize("numerics", ["exact", "split"])
def test_full_size_program(ctx, sd_full, numerics):
    """the published rf = 27 model (channels 128: heads of 32, 64 and 128 channels, the 1536 -> 1024 cat_conv) on one chunk of 8 frames;
    in split numerics the wide 1x1 convolutions run on the split kernels, behind the two ops' maxima"""
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, (8, 17, 2)).astype(F32)
    lf = W.GastNetLifter(numerics=numerics, ctx=ctx, state_dict=sd_full, spec=FULL8, flip_augment=True)
    try:
        names, kinds = lf.net.prog.op_names, lf.net.conv_kinds()
        op = lf.net.prog.ops[names.index("layers_graph_conv.2.cat_conv")]
        assert (op.cin, op.cout) == (1536, 1024)
        att = lf.net.prog.ops[names.index("layers_graph_conv.2.global_graph_layer.attn")]
        assert att.type == L.PP_OP_JOINT_ATTN and att.cin // att.stride == 128
        print(f"{numerics}: {len(names)} ops, {int((kinds == 2).sum())} convolutions on the split kernels, {int((kinds == 1).sum())} on float32 MFMA")
        if numerics == "split":
            assert kinds[names.index("layers_graph_conv.2.cat_conv")] == 2
        got = lf.lift(x)
    finally:
        lf.close()
    _check(got, _ref_lift(x, sd_full, FULL8, True, F32), _ref_lift(x, sd_full, FULL8, True, F64), f"full-size lift, 8 frames, {numerics}")


# ---- 6. the wrapper on the table shim, from a checkpoint file ----------------------------------------------------------------------
def test_wrapper_through_the_tables(sd_full, tmp_path, monkeypatch):
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    monkeypatch.delenv("POSEPIPE_SYNTHETIC_WEIGHTS", raising=False)
    os.makedirs(tmp_path / "gastnet")
    torch.save({"model_pos": {"module." + k: torch.from_numpy(v) for k, v in sd_full.items()}}, str(tmp_path / "gastnet" / "27_frame_model.bin"))
    from posepipeline_amd import djshim, pipeline as pl
    djshim.reset()
    W._cache.clear()
    rng = np.random.default_rng(9)
    height, width, n = 480, 640, 12
    kp = np.empty((n, 17, 3), F32)
    kp[..., :2] = ((320, 240) + rng.uniform(-0.3, 0.3, (n, 17, 2)) * (width, height)).astype(F32)
    kp[..., 2] = 0.9
    kp[4] = 0                                        # no detection
    kp[7, 16, 2] = 0.1                               # COCO right ankle = H36M joint 3 below the threshold: revise_kpts, 3 <- 2
    vkey = {"video_project": "test", "filename": "gast"}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 10, 18)})
    pl.VideoInfo().insert1({**vkey, "timestamps": [], "delta_time": [], "fps": 30.0, "height": height, "width": width, "num_frames": n})
    key = {**vkey, "tracking_method": 5, "video_subject_id": 0, "top_down_method": 0, "lifting_method": 0}
    pl.TopDownPerson().insert1({k: v for k, v in key.items() if k != "lifting_method"} | {"keypoints": kp})
    pl.LiftingMethod().insert1(key)
    try:
        pl.LiftingPerson().make(dict(key))           # the "GastNet" branch: the checkpoint file is there
        k3, valid = (pl.LiftingPerson & key).fetch1("keypoints_3d", "keypoints_valid")
        k3, valid = np.asarray(k3), list(valid)
        assert valid == [i != 4 for i in range(n)]
        assert k3.shape == (n, 17, 3) and k3.dtype == F64 and not k3[4].any() and all(k3[i].any() for i in range(n) if i != 4)
        idx = [i for i in range(n) if i != 4]
        h36m = W.coco_h36m(kp[..., :2])
        h36m[7, 3] = h36m[7, 2]
        x = W.normalize_screen_coordinates(h36m[idx], w=width, h=height).astype(F32)
        spec = M.GastNetSpec()
        sd = W.load_state_dict()
        ref32 = W.camera_to_world(_ref_lift(x, sd, spec, True, F32))
        _check(k3[idx], ref32, _rot64(_ref_lift(x, sd, spec, True, F64)), "process_gastnet, 11 valid frames of 12")
    finally:
        for lf in W._cache.values():
            lf.close()
        W._cache.clear()
        djshim.reset()


def _rot64(v):
    q = W.CAMERA_QUATERNION.astype(F64)
    qv = np.broadcast_to(q[1:], v.shape)
    uv = np.cross(qv, v)
    return v + 2 * (q[0] * uv + np.cross(qv, uv))
