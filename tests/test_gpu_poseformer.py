"""PoseFormer lifting on the GPU: the spatial kernel, the attention op, the whole lift in both numerics, the wrapper on the table shim
and the checkpoint file, against tests/poseformer_ref.py.

Tolerance: in each test `dev32` is the largest deviation, on that test's inputs and weights, of the torch float32 CPU evaluation from
the float64 reference; the GPU result must lie within FACTOR = 4 x dev32 of the float64 reference (the margin tests/test_gpu_tracktor.py
gives ECC over its float32 deviation: another summation order is a float32 evaluation like torch's, not a less accurate one).  The
measured ratios are printed and recorded in DESIGN_LOG.md 5k.
"""
import datetime
import os

import numpy as np
import pytest
import torch

from posepipeline_amd import _lib as L
from posepipeline_amd.models import poseformer as M
from posepipeline_amd.wrappers import poseformer as W
from tests import poseformer_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SPEC = M.PoseFormerSpec()
MAX_WINDOWS = 8
N_LONG = MAX_WINDOWS + 83          # 11 windows: one full batch of 8 and a ragged one of 3


def _check(got, ref32, ref64, what):
    dev = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    assert dev > 0, what
    print(f"{what}: GPU vs float64 {err:.3e}, float32-on-CPU vs float64 (dev32) {dev:.3e}, ratio {err / dev:.2f} (bound {FACTOR:g}), "
          f"max |ref| {np.abs(ref64).max():.3g}")
    assert err <= FACTOR * dev, (what, err, dev, err / dev)


@pytest.fixture(scope="module")
def sd():
    return M.synth_params(M.poseformer_param_shapes(SPEC), seed=11)


@pytest.fixture(scope="module")
def clip(sd):
    """one seeded clip and its references, computed once: x [91][17][2] float32, per window float64 and torch-float32 results"""
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (N_LONG, 17, 2)).astype(np.float32)
    ref64 = R.forward_clip(x.astype(np.float64), R.as_dtype(sd, np.float64))
    ref32 = R.torch_forward_windows(x, sd, torch.float32)
    for a in (x, ref64, ref32):
        a.setflags(write=False)
    return x, ref64, ref32


_lifters = {}


def _lifter(ctx, sd, numerics, channel_pad=0):
    """one resident model per form, built inside a test (under the suite's numerics setting) and shared by the tests of this module"""
    if (numerics, channel_pad) not in _lifters:
        _lifters[numerics, channel_pad] = W.PoseFormerLifter(max_windows=MAX_WINDOWS, numerics=numerics, ctx=ctx, state_dict=sd,
                                                             channel_pad=channel_pad)
    return _lifters[numerics, channel_pad]


@pytest.fixture(scope="module", autouse=True)
def _close_lifters():
    yield
    for lf in _lifters.values():
        lf.close()
    _lifters.clear()


# ---- 1. the spatial kernel ---------------------------------------------------------------------------------------------------------
def _spatial(ctx, d_params, x):
    n = x.shape[0]
    d_feat = ctx.malloc(n * 544 * 4)
    try:
        L.check(ctx.lib.pp_poseformer_spatial(ctx.handle, L.ptr(d_params), L.ptr(np.ascontiguousarray(x)), n, L.PP_MEM_HOST, L.ptr(d_feat)),
                "pp_poseformer_spatial")
        out = np.empty((n, 544), np.float32)
        ctx.d2h(out, d_feat)
    finally:
        ctx.free(d_feat)
    return out


def test_spatial_kernel(ctx, sd):
    block = M.spatial_param_block(SPEC, sd)
    assert block.size == ctx.lib.pp_poseformer_spatial_param_floats() == 34880
    d_params = ctx.malloc(block.nbytes)
    try:
        ctx.h2d(d_params, block)
        rng = np.random.default_rng(3)
        x = rng.uniform(0, 1, (130, 17, 2)).astype(np.float32)
        ref64 = R.spatial_np(x.astype(np.float64), R.as_dtype(sd, np.float64))
        ref32 = R.torch_spatial(x, sd, torch.float32)
        big = _spatial(ctx, d_params, x)
        for n in (1, 7, 130):
            got = big if n == 130 else _spatial(ctx, d_params, x[:n])
            assert got.shape == (n, 544)
            _check(got, ref32[:n], ref64[:n], f"spatial kernel, {n} frames")
        # a frame's features do not depend on the call it is part of
        for k in (0, 64, 129):
            assert np.array_equal(_spatial(ctx, d_params, x[k:k + 1])[0], big[k]), k
        assert np.array_equal(_spatial(ctx, d_params, x[:7]), big[:7])
        # more frames than the feature index can hold: refused before anything is read
        assert ctx.lib.pp_poseformer_spatial(ctx.handle, L.ptr(d_params), L.ptr(x), 4_000_000, L.PP_MEM_HOST, L.ptr(d_params)) == -1
        assert "frames in one call" in L.last_error()
    finally:
        ctx.free(d_params)


# ---- 2. the attention op -----------------------------------------------------------------------------------------------------------
def _attention(ctx, qkv, heads, c_real):
    b, t, c3 = qkv.shape
    c_buf = c3 // 3
    d_in, d_out = ctx.malloc(qkv.nbytes), ctx.malloc(b * t * c_buf * 4)
    try:
        ctx.h2d(d_in, qkv)
        ctx.h2d(d_out, np.full((b, t, c_buf), 7.0, np.float32))
        L.check(ctx.lib.pp_attention_f32(ctx.handle, L.ptr(d_in), b, t, heads, c_real, c_buf, L.ptr(d_out)), "pp_attention_f32")
        out = np.empty((b, t, c_buf), np.float32)
        ctx.d2h(out, d_out)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return out


def _attention_case(ctx, b, t, heads, hd, c_buf, scale_to=None):
    c = heads * hd
    rng = np.random.default_rng(b * 1000 + t * 10 + hd)
    qkv = rng.standard_normal((b, t, 3, c_buf)).astype(np.float32)          # the padding channels hold garbage: never read
    real = np.ascontiguousarray(qkv[..., :c]).reshape(b, t, 3 * c)
    if scale_to is not None:
        q, k = (real[..., s * c:(s + 1) * c].reshape(b, t, heads, hd).astype(np.float64) for s in (0, 1))
        peak = np.abs(np.einsum("bihd,bjhd->bhij", q, k)).max() * hd ** -0.5
        f = np.float32(np.sqrt(scale_to / peak) * 1.01)
        qkv[:, :, :2, :c] *= f
        real = np.ascontiguousarray(qkv[..., :c]).reshape(b, t, 3 * c)
        q, k = (real[..., s * c:(s + 1) * c].reshape(b, t, heads, hd).astype(np.float64) for s in (0, 1))
        scores = np.einsum("bihd,bjhd->bhij", q, k) * hd ** -0.5
        assert scores.max() >= scale_to or scores.min() <= -scale_to, (scores.min(), scores.max())
    got = _attention(ctx, qkv.reshape(b, t, 3 * c_buf), heads, c)
    ref64 = R.attention_np(real.astype(np.float64), heads)
    ref32 = R.torch_attention(real, heads, torch.float32)
    assert np.abs(ref64 - R.torch_attention(real.astype(np.float64), heads, torch.float64)).max() <= 1e-12
    _check(got[..., :c], ref32, ref64, f"attention b={b} t={t} heads={heads} hd={hd} c_buf={c_buf}" + (f" scores to {scale_to:g}" if scale_to else ""))
    assert not got[..., c:].any()                     # exact zeros beyond the real channels, whatever the buffer held


@pytest.mark.parametrize("b,t,heads,hd,c_buf", [(3, 81, 8, 68, 640), (5, 17, 8, 4, 32), (2, 5, 1, 4, 8)],
                         ids=["temporal_81x8x68_of640", "spatial_17x8x4", "tiny_5x1x4_of8"])
def test_attention_op(ctx, b, t, heads, hd, c_buf):
    _attention_case(ctx, b, t, heads, hd, c_buf)


def test_attention_op_large_scores(ctx):
    """q and k scaled until the scores reach +-40: exp of the raw scores would lose everything but the row maximum's neighbours to
    rounding or overflow in other rows; the row maximum is subtracted first"""
    _attention_case(ctx, 2, 81, 8, 68, 544, scale_to=40.0)


def test_attention_argument_errors(ctx):
    d = ctx.malloc(1 << 16)
    try:
        for b, t, heads, c_real, c_buf in ((1, 129, 1, 4, 4), (1, 8, 1, 132, 132), (1, 8, 1, 6, 8), (1, 8, 2, 8, 6), (1, 8, 3, 8, 8)):
            rc = ctx.lib.pp_attention_f32(ctx.handle, L.ptr(d), b, t, heads, c_real, c_buf, L.ptr(d))
            assert rc == -1, (t, heads, c_real, c_buf, L.last_error())
    finally:
        ctx.free(d)


# ---- 3. the lift -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numerics,channel_pad", [(None, 0), ("split", 0), ("split", 128)], ids=["suite_numerics", "split", "split_padded"])
def test_lift(ctx, sd, clip, numerics, channel_pad):
    """the lifter's form (the real channels) in the suite's numerics and in split numerics, where fc2 alone is eligible for the split
    kernels; and the padded program in split numerics, where every Linear layer is and the padding channels must stay zeros"""
    x, ref64, ref32 = clip
    lf = _lifter(ctx, sd, numerics, channel_pad)
    kinds = lf.net.conv_kinds()
    assert lf.net.prog.bufs[lf.net.prog.named["input"]] == (1, 81, 544 + channel_pad * 3 // 4)
    print(f"numerics {lf.net.numerics} ({lf.net.split_kind}), input {lf.net.prog.bufs[lf.net.prog.named['input']]}, conv kinds {kinds[kinds > 0].tolist()}")
    if numerics == "split":
        assert lf.net.numerics == "split"
        want = [2] * 16 if channel_pad else [1, 1, 1, 2] * 4         # qkv, proj, fc1, fc2 per block
        assert kinds[kinds > 0].tolist() == want, kinds
    results = {}
    for n in (81, 84, N_LONG):
        got = lf.lift(x[:n])
        assert got.shape == (n - 80, 17, 3) and got.dtype == np.float32
        _check(got, ref32[:n - 80], ref64[:n - 80], f"lift N={n} ({lf.net.numerics})")
        assert np.array_equal(lf.lift(x[:n]), got), f"two runs differ, N={n}"
        results[n] = got
    long = results[N_LONG]
    # what a window's sample holds does not depend on the clip around it or on the batch it shares
    assert np.array_equal(results[81][0], long[0]) and np.array_equal(results[84], long[:4])
    for i in (3, 7, 8, 10):        # the last of the first batch, the first and last of the ragged one
        assert np.array_equal(lf.lift(x[i:i + 81])[0], long[i]), i


def test_lift_argument_errors(ctx, sd):
    lf = _lifter(ctx, sd, None)
    nm, po = lf.net.prog.named, lf.net.prog.param_offsets
    x = np.zeros((90, 17, 2), np.float32)
    out = np.zeros((10, 51), np.float32)
    args = lambda **kw: [lf.net.handle, kw.get("inb", nm["input"]), nm["output"], kw.get("sp", po["spatial_params"]), po["temporal_pos"],   # noqa: E731
                         kw.get("hd", po["head_params"]), L.ptr(x), kw.get("n", 90), L.ptr(out), kw.get("mem", L.PP_MEM_HOST), None]
    assert ctx.lib.pp_poseformer_lift(*args(n=80)) == -1 and "receptive field" in L.last_error()
    assert ctx.lib.pp_poseformer_lift(*args(mem=7)) == -1
    assert ctx.lib.pp_poseformer_lift(*args(inb=99)) == -1
    assert ctx.lib.pp_poseformer_lift(*args(hd=lf.net.prog.blob.size - 100)) == -1 and "out of blob" in L.last_error()
    assert ctx.lib.pp_poseformer_lift(*args(sp=2)) == -1
    assert ctx.lib.pp_poseformer_lift(*args()) == 0


def test_stage_times_are_reported(ctx, sd, clip):
    x = clip[0]
    lf = _lifter(ctx, sd, None)
    plain = lf.lift(x[:84])
    assert lf.stage_ms is None
    timed = lf.lift(x[:84], timed=True)
    assert np.array_equal(plain, timed) and lf.stage_ms.shape == (4,) and (lf.stage_ms > 0).all(), lf.stage_ms


# ---- 4. the wrapper on the table shim ----------------------------------------------------------------------------------------------
def test_wrapper_through_the_tables(monkeypatch):
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("PIPELINE_3RDPARTY", raising=False)
    from posepipeline_amd import djshim, pipeline as pl
    djshim.reset()
    W._cache.clear()
    rng = np.random.default_rng(9)
    height, width, n = 480, 640, 90
    kp = np.empty((n, 17, 3), np.float32)
    kp[..., :2] = ((320, 240) + rng.uniform(-0.3, 0.3, (n, 17, 2)) * (width, height)).astype(np.float32)
    kp[..., 2] = 0.9
    vkey = {"video_project": "test", "filename": "lift"}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 10, 18)})
    pl.VideoInfo().insert1({**vkey, "timestamps": [], "delta_time": [], "fps": 30.0, "height": height, "width": width, "num_frames": n})
    key = {**vkey, "tracking_method": 5, "video_subject_id": 0, "top_down_method": 0}
    pl.TopDownPerson().insert1({**key, "keypoints": kp})
    try:
        res = W.process_liftformer(key)
        assert res is key
        k3 = res["keypoints_3d"]
        assert k3.shape == (n, 17, 3) and k3.dtype == np.float64
        assert not k3[:40].any() and not k3[50:].any() and k3[40:50].any()
        sd = W.load_state_dict()
        x = W.normalize(W.coco_h36m(kp[..., :2]), height, width).astype(np.float32)
        ref64 = R.forward_clip(x.astype(np.float64), R.as_dtype(sd, np.float64))
        ref32 = R.torch_forward_windows(x, sd, torch.float32)
        _check(k3[40:50], ref32, ref64, "process_liftformer rows 40..49")
    finally:
        for lf in W._cache.values():
            lf.close()
        W._cache.clear()
        djshim.reset()


# ---- 5. the checkpoint file --------------------------------------------------------------------------------------------------------
def test_checkpoint_file(ctx, sd, clip, tmp_path, monkeypatch):
    x = clip[0][:84]
    want = _lifter(ctx, sd, None).lift(x)
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    monkeypatch.delenv("POSEPIPE_SYNTHETIC_WEIGHTS", raising=False)
    os.makedirs(tmp_path / "poseformer")
    torch.save({"model_pos": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, str(tmp_path / "poseformer" / "detected81f.bin"))
    lf = W.PoseFormerLifter(max_windows=MAX_WINDOWS, ctx=ctx)
    try:
        assert np.array_equal(lf.lift(x), want)
    finally:
        lf.close()
