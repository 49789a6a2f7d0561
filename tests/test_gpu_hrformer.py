"""HRFormer on the GPU: the three new ops and PP_OP_GELU_ADD one by one, the tiny network, the default numerics and the wrapper /
table path, against tests/hrformer_ref.py.

Tolerance of everything that is not bit-exact (LayerNorm, GELU, attention, the network): the GPU result is compared with the
float64 reference, and the bound is FACTOR = 4 times the deviation of the SAME reference evaluated in float32 on the CPU from
the float64 one, measured here per case as max abs.  The factor covers another, equally long, summation order.  The observed
ratios are printed and recorded in DESIGN_LOG.md.
"""
import datetime

import numpy as np
import pytest
import torch

from posepipeline_amd import _lib as L
from posepipeline_amd import ops
from posepipeline_amd.models import hrformer as M
from posepipeline_amd.models import hrnet, synth
from posepipeline_amd.program import Net, ProgramBuilder
from tests import hrformer_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def _bound(ref32, ref64, what):
    dev = float(np.abs(np.asarray(ref32, np.float64) - np.asarray(ref64, np.float64)).max())
    assert dev > 0, what
    return dev


def _check(got, ref32, ref64, what):
    dev = _bound(ref32, ref64, what)
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64)).max())
    print(f"{what}: GPU vs float64 {err:.3e}, float32-on-CPU vs float64 {dev:.3e}, ratio {err / dev:.2f} (bound {FACTOR:g})")
    assert err <= FACTOR * dev, (what, err, dev, err / dev)
    return err / dev


def _one_op(ctx, n, in_dims, build, x, out_fill=None):
    """a one-op program: input buffer -> op -> output buffer; returns the output [n][h][w][c]"""
    pb = ProgramBuilder()
    xin = pb.buf(*in_dims, name="x")
    out = build(pb, xin)
    pb.vbufs[out].pinned = True
    pb.named["y"] = out
    prog = pb.build()
    assert len(prog.ops) == 1
    net = Net(ctx, prog, max_batch=n)
    ctx.h2d(net.buffer("x")[0], np.ascontiguousarray(x, np.float32))
    if out_fill is not None:
        ctx.h2d(net.buffer("y")[0], np.ascontiguousarray(out_fill, np.float32))
    net.run(n)
    y = net.read("y", n)
    net.close()
    return y, prog.ops[0]


# ---- 1. depthwise 3x3 --------------------------------------------------------------------------------------------------------------
DW_CASES = [
    (1, 5, 7, 8, 8, 1, None),           # one block
    (3, 9, 10, 80, 78, 1, None),        # 78 real channels of 80
    (2, 7, 9, 156, 156, 2, "relu"),     # odd size, output 4x5
    (2, 12, 9, 312, 312, 2, None),      # several blocks
]


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "n%d_%dx%dx%d_s%d" % (c[0], c[1], c[2], c[3], c[5]))
def test_dwconv3x3_bit_exact(ctx, case):
    n, h, w, cb, c, stride, act = case
    rng = np.random.default_rng(h * 100 + w + cb)
    x = (rng.standard_normal((n, h, w, cb)) * 2).astype(np.float32)
    wt = rng.normal(0, 0.4, (c, 1, 3, 3)).astype(np.float32)
    b = rng.normal(0, 0.3, c).astype(np.float32)
    code = {None: L.PP_RELU_NONE, "relu": L.PP_RELU_LAST}[act]
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    got, op = _one_op(ctx, n, (h, w, cb), lambda pb, xin: pb.dwconv3x3(xin, wt, b, stride=stride, act=code), x,
                      out_fill=np.full((n, ho, wo, cb), 7.0))
    assert op.type == L.PP_OP_DWCONV3X3 == 11 and got.shape == (n, ho, wo, cb)
    want = R.dwconv3x3_np(x[..., :c], wt, b, stride=stride, act=act)
    assert np.array_equal(got[..., :c], want), np.abs(got[..., :c] - want).max()
    assert not got[..., c:].any()                         # zero weights and biases: the padding channels are zeros
    if act == "relu":
        assert (want == 0).any() and (want > 0).any()


def test_dwconv3x3_gelu_on_input_and_output(ctx):
    """the FFN's form (tiled kernel: 9x10 is 2x2 tiles, 24 channels are one full and one half channel group)"""
    n, h, w, c = 2, 9, 10, 24
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((n, h, w, c)) * 2).astype(np.float32)
    wt = rng.normal(0, 0.4, (c, 1, 3, 3)).astype(np.float32)
    b = rng.normal(0, 0.3, c).astype(np.float32)
    got, op = _one_op(ctx, n, (h, w, c), lambda pb, xin: pb.dwconv3x3(xin, wt, b, act=L.PP_ACT_GELU, gelu_in=True), x)
    assert op.pad_end == L.PP_DW_GELU_IN and op.relu == L.PP_ACT_GELU
    ref = {dt: R.dwconv3x3_t(torch.from_numpy(x).to(dt), torch.from_numpy(wt), torch.from_numpy(b), act="gelu", gelu_in=True).numpy()
           for dt in (torch.float32, torch.float64)}
    _check(got, ref[torch.float32], ref[torch.float64], "dwconv3x3 GELU in / out")
    # without the input GELU the tiled and the direct kernel are the same arithmetic: bit-equal to numpy through GELU-free paths
    plain, _ = _one_op(ctx, n, (h, w, c), lambda pb, xin: pb.dwconv3x3(xin, wt, b), x)
    assert np.array_equal(plain, R.dwconv3x3_np(x, wt, b))


# ---- 2. LayerNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb,c,offset", [(80, 78, 0.0), (156, 156, 0.0), (624, 624, 0.0), (80, 78, 100.0)],
                         ids=["78of80", "156", "624", "78of80_offset100"])
def test_layernorm_op(ctx, cb, c, offset):
    n, h, w = 2, 9, 10
    rng = np.random.default_rng(cb + int(offset))
    x = (rng.standard_normal((n, h, w, cb)) + offset).astype(np.float32)      # the padding channels hold garbage: ignored, zeroed
    g = rng.uniform(0.5, 1.5, c).astype(np.float32)
    b = rng.normal(0, 0.2, c).astype(np.float32)
    got, op = _one_op(ctx, n, (h, w, cb), lambda pb, xin: pb.layernorm(xin, g, b, eps=1e-6), x, out_fill=np.full((n, h, w, cb), 7.0))
    assert op.type == L.PP_OP_LAYERNORM == 12 and (op.cin, op.cout) == (c, cb)
    ref = {dt: R.layernorm(torch.from_numpy(x[..., :c]).to(dt), torch.from_numpy(g).to(dt), torch.from_numpy(b).to(dt)).numpy()
           for dt in (torch.float32, torch.float64)}
    _check(got[..., :c], ref[torch.float32], ref[torch.float64], f"layernorm c={c} of {cb}, offset {offset:g}")
    assert not got[..., c:].any()
    if offset:      # a one-pass variance (E[x^2] - mean^2 in float32) is off by ~1e-3 here
        assert np.abs(got[..., :c] - ref[torch.float64]).max() < 1e-4


# ---- 3. window attention -----------------------------------------------------------------------------------------------------------
ATTN_CASES = [
    (1, 7, 7, 8, 1),         # one window, no padding
    (2, 9, 10, 78, 2),       # pad_h = 5 split 2 / 3, pad_w = 4, head dim 39, 78 of 80 channels
    (2, 18, 24, 156, 4),
    (1, 12, 9, 624, 16),
    (1, 3, 2, 24, 4),        # the map is smaller than a window
]


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "n%d_%dx%d_c%d_h%d" % c)
def test_window_attention_op(ctx, case):
    n, h, w, c, heads = case
    cb = (c + 3) // 4 * 4
    rng = np.random.default_rng(h * 1000 + w * 10 + heads)
    qkv = rng.standard_normal((n, h, w, 3, c)).astype(np.float32)
    bias = rng.standard_normal(3 * c).astype(np.float32)                     # non-zero: zero keys for the padding fail
    table = rng.standard_normal((169, heads)).astype(np.float32)              # asymmetric: a transposed index fails
    x = (rng.standard_normal((n, h, w, 3, cb)) * 50).astype(np.float32)       # garbage in the padding channels: never read
    x[..., :c] = qkv
    got, op = _one_op(ctx, n, (h, w, 3 * cb), lambda pb, xin: pb.window_attention(xin, table, bias, c_real=c, heads=heads),
                      x.reshape(n, h, w, 3 * cb), out_fill=np.full((n, h, w, cb), 7.0))
    assert op.type == L.PP_OP_WINDOW_ATTN == 13 and (op.cin, op.cout, op.stride) == (c, cb, heads)
    ref = {dt: R.attn_closed_form(torch.from_numpy(qkv.reshape(n, h, w, 3 * c)).to(dt), torch.from_numpy(bias).to(dt),
                                  torch.from_numpy(table).to(dt), heads).numpy() for dt in (torch.float32, torch.float64)}
    _check(got[..., :c], ref[torch.float32], ref[torch.float64], "window attention %s" % (case,))
    assert not got[..., c:].any()


def test_gelu_add_op(ctx):
    n, h, w, c = 2, 9, 10, 80
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((n, h, w, c)) * 2).astype(np.float32)
    r = rng.standard_normal((n, h, w, c)).astype(np.float32)
    pb = ProgramBuilder()
    xin, rin = pb.buf(h, w, c, name="x"), pb.buf(h, w, c, name="r")
    out = pb.gelu_add(xin, res1=rin)
    pb.vbufs[out].pinned = True
    pb.named["y"] = out
    net = Net(ctx, pb.build(), max_batch=n)
    ctx.h2d(net.buffer("x")[0], x)
    ctx.h2d(net.buffer("r")[0], r)
    net.run(n)
    got = net.read("y", n)
    net.close()
    ref = {dt: (torch.from_numpy(r).to(dt) + R.gelu(torch.from_numpy(x).to(dt))).numpy() for dt in (torch.float32, torch.float64)}
    _check(got, ref[torch.float32], ref[torch.float64], "gelu_add")
    # GELU in double, one rounding, one float32 add: the value is reproducible
    assert np.array_equal(got, (r + R.gelu_f32_of_f64(x)).astype(np.float32))


def test_new_ops_are_validated(ctx):
    pb = ProgramBuilder()
    x = pb.buf(9, 10, 24, name="x")
    pb.window_attention(x, np.ones((169, 2), np.float32), np.zeros(24, np.float32), c_real=8, heads=2)
    prog = pb.build()
    prog.ops[0].kh = 5
    with pytest.raises(L.PosePipeHipError, match="window_attn"):
        Net(ctx, prog, max_batch=1)
    pb = ProgramBuilder()
    x = pb.buf(9, 10, 8, name="x")
    pb.dwconv3x3(x, np.ones((8, 1, 3, 3), np.float32), None, stride=2)
    prog = pb.build()
    prog.ops[0].pad_end = L.PP_DW_GELU_IN                   # GELU on the input is the stride-1 form
    with pytest.raises(L.PosePipeHipError, match="dwconv3x3"):
        Net(ctx, prog, max_batch=1)
    pb = ProgramBuilder()
    x = pb.buf(9, 10, 8, name="x")
    pb.layernorm(x, np.ones(6, np.float32), np.zeros(6, np.float32))
    prog = pb.build()
    prog.ops[0].cin = 12
    with pytest.raises(L.PosePipeHipError, match="layernorm"):
        Net(ctx, prog, max_batch=1)


# ---- 4. the tiny network -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """spec, parameters, input and the reference heat-maps in float64 and float32 (computed once, never modified)"""
    spec = R.tiny_spec()
    sd = M.synth_params(spec, seed=4)
    x = np.random.default_rng(0).standard_normal((3, 3, spec.in_h, spec.in_w)).astype(np.float32)
    ref64 = R.HRFormerRef(sd, spec, torch.float64).forward(x)
    ref32 = R.HRFormerRef(sd, spec, torch.float32).forward(x)
    ref64.setflags(write=False)
    ref32.setflags(write=False)
    return spec, sd, x, ref64, ref32


def _nhwc4(x):
    xin = np.zeros((x.shape[0], x.shape[2], x.shape[3], 4), np.float32)
    xin[..., :3] = np.transpose(x, (0, 2, 3, 1))
    return xin


def test_tiny_network_vs_float64(ctx, tiny):
    spec, sd, x, ref64, ref32 = tiny
    assert np.isfinite(ref64).all() and np.abs(ref64).max() > 1e-3 and np.ptp(ref64) > 1e-3
    net = Net(ctx, M.build_hrformer_program(spec, sd), max_batch=3)
    assert net.numerics == "exact"
    hm = net.forward(_nhwc4(x)).reshape(3, spec.num_joints, *spec.heatmap_hw)
    net.close()
    _check(hm, ref32, ref64, "tiny HRFormer heat-maps")


# ---- 5. default numerics -----------------------------------------------------------------------------------------------------------
CS = np.array([[960.0, 540.0, 1.5, 2.0], [300.5, 700.25, 1.2, 1.6], [1700.0, 400.0, 2.1, 2.8], [1020.0, 750.0, 3.0, 4.0]], np.float32)


def _split_vs_exact(ctx, spec, seed):
    sd = M.synth_params(spec, seed=seed, smooth=True)
    prog = M.build_hrformer_program(spec, sd)
    n = 4
    x = synth.blob_crops(np.random.default_rng(5), n, spec.in_h, spec.in_w)
    kps, hms = {}, {}
    for numerics in ("exact", "split"):
        net = Net(ctx, prog, max_batch=2 * n, numerics=numerics)
        assert net.numerics == numerics and (numerics == "split") == bool((net.conv_kinds() == 2).any())
        td = ops.TopDown(net, 17, flip_perm=hrnet.flip_perm(17), shift_heatmap=True, post="default", blur_kernel=17)
        kps[numerics] = td.run_precropped(x, CS)
        hms[numerics] = net.read("output", 2 * n)
        td.close()
        net.close()
    assert np.isfinite(hms["exact"]).all() and np.ptp(hms["exact"]) > 1e-3
    assert not np.array_equal(hms["split"], hms["exact"]), "the split kernels did not run"
    d = np.abs(kps["split"][:, :, :2] - kps["exact"][:, :, :2]).max(axis=2)
    gap = np.abs(hms["split"] - hms["exact"]).max() / np.abs(hms["exact"]).max()
    print(f"HRFormer {spec.in_h}x{spec.in_w} split vs exact: {d.size} joints, max deviation {d.max():.2e} px, heat-maps {gap:.2e} of range")
    return d


def test_default_numerics_vs_exact_tiny(ctx):
    d = _split_vs_exact(ctx, R.tiny_spec(), seed=11)
    assert d.max() <= 1e-3, d


def test_default_numerics_vs_exact_full_size(ctx):
    """The project's contract (BASELINE.json): decoded key points within 1e-3 px of the exact kernels, full-size net."""
    d = _split_vs_exact(ctx, M.hrformer_base_384x288(), seed=11)
    assert d.max() <= 1e-3, d


# ---- 6. wrapper and table ----------------------------------------------------------------------------------------------------------
CLIP_SEED = 107      # picked on the CPU, from the float64 reference alone, so that every joint of every frame passes the decode guard


def make_clip(tmp_path, seed=CLIP_SEED, n=6):
    """a short synthetic clip on the table shim with one tracked person, absent in the first frames"""
    from posepipeline_amd import djshim, pipeline as pl, video
    from tests.test_gpu_pipeline import synth_clip
    djshim.reset()
    frames, boxes = synth_clip(np.random.default_rng(seed), n, 240, 320)
    path = str(tmp_path / "clip.ppvid")
    video.write_ppvid(path, frames, fps=30.0)
    vkey = {"video_project": "test", "filename": "hrformer_clip"}
    pl.Video().insert1({**vkey, "video": path, "start_time": datetime.datetime(2024, 1, 1)})
    tracks = [[{"track_id": 1, "tlbr": np.r_[b[:2], b[:2] + b[2:]], "tlhw": b, "confidence": 0.9}] for b in boxes]
    for t in (0, 1, 2, 3, 4):      # PersonBbox fills two frames backwards from frame 5: frames 0 - 2 stay absent (NaN rows)
        tracks[t] = []
    tkey = {**vkey, "tracking_method": 5}
    pl.TrackingBboxMethod().insert1(tkey)
    pl.TrackingBbox().insert1({**tkey, "tracks": tracks, "num_tracks": 1})
    pl.PersonBboxValid().insert1({**tkey, "video_subject_id": 0, "keep_tracks": [1]})
    pl.PersonBbox().populate(tkey)
    bbox = (pl.PersonBbox & tkey).fetch1("bbox")
    return frames, bbox, {**tkey, "video_subject_id": 0}


def merged_f64(hm2, shift=True):
    """flip-merge of one person's maps [2][K][h][w] (plain, mirrored) in float64"""
    perm = hrnet.flip_perm(hm2.shape[1])
    back = hm2[1][perm][..., ::-1].copy()
    if shift:
        back[..., 1:] = back[..., :-1].copy()
    return (hm2[0] + back) * 0.5


def decode_margin(m):
    """per joint of a merged map [K][h][w]: the smallest of the top-2 gap and, where the 'default' decode takes them, the two
    neighbour differences whose SIGN it uses"""
    k, h, w = m.shape
    out = np.empty(k)
    for j in range(k):
        flat = np.sort(m[j].ravel())
        gap = flat[-1] - flat[-2]
        py, px = np.unravel_index(np.argmax(m[j]), (h, w))
        if 1 < px < w - 1 and 1 < py < h - 1:
            gap = min(gap, abs(m[j][py][px + 1] - m[j][py][px - 1]), abs(m[j][py + 1][px] - m[j][py - 1][px]))
        out[j] = gap
    return out


def clip_reference(frames, bbox, spec, sd):
    """CPU chain + the guard's figures: (keypoints, smallest decode margin over all joints of all frames, float32-vs-float64
    deviation of the reference's heat-maps on these crops)"""
    from oracle import preprocess as opre
    ref, maps = R.topdown_chain(sd, spec, frames, bbox)
    m32 = R.HRFormerRef(sd, spec, torch.float32)
    margin, dev = np.inf, 0.0
    for fr, bb, hm in zip(frames, bbox, maps):
        if hm is None:
            continue
        x, _, _, _ = opre.top_down_input(fr[:, :, ::-1], bb, (spec.in_w, spec.in_h))
        dev = max(dev, float(np.abs(m32.forward(np.stack([x, x[:, :, ::-1]])) - hm).max()))
        margin = min(margin, float(decode_margin(merged_f64(hm)).min()))
    return ref, margin, dev


def test_hrformer_method_through_wrapper_and_table(ctx, tmp_path, monkeypatch):
    """`mmpose_top_down_person(key, "HRFormer_COCO")` and TopDownPerson row 3 on the table shim, tiny spec, against the CPU chain
    oracle crop -> hrformer_ref (float64) -> oracle flip-merge + 'default' decode."""
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    from posepipeline_amd import djshim, pipeline as pl
    from posepipeline_amd.wrappers import mmpose as wmm
    frames, bbox, pkey = make_clip(tmp_path)
    spec = R.tiny_spec()
    sd = M.synth_params(spec, seed=1)                     # what `_model` builds under POSEPIPE_SYNTHETIC_WEIGHTS
    ref, margin, dev = clip_reference(frames, bbox, spec, sd)
    # the 'default' decode takes an arg-max and two signs: EVERY joint of every frame must be decided by the reference alone
    print(f"decode guard: smallest margin {margin:.3e}, float32-vs-float64 deviation {dev:.3e}, ratio {margin / dev:.0f}")
    assert margin > 100 * dev, (margin, dev)
    monkeypatch.setitem(wmm._METHODS, "HRFormer_COCO", (lambda k: R.tiny_spec(k),) + wmm._METHODS["HRFormer_COCO"][1:])
    wmm._cache.clear()
    kp = wmm.mmpose_top_down_person(pkey, method="HRFormer_COCO")
    n = len(bbox)
    assert kp.shape == (n, 17, 3) and kp.dtype == np.float64
    absent = np.isnan(bbox).any(axis=1)
    assert absent.any() and not absent.all() and not kp[absent].any()
    ok = ~absent
    err = np.abs(kp[ok][:, :, :2] - ref[ok][:, :, :2]).max()
    print(f"wrapper vs CPU chain: {ok.sum() * 17} joints, max deviation {err:.2e} px")
    assert err <= 1e-3, err
    assert np.abs(kp[ok][:, :, 2] - ref[ok][:, :, 2]).max() <= FACTOR * dev
    _, net, _, _ = wmm._cache[("HRFormer_COCO", 0)]
    assert isinstance(net.prog, type(M.build_hrformer_program(spec, sd))) and L.PP_OP_WINDOW_ATTN in [op.type for op in net.prog.ops]
    # the same through the table layer: lookup row 3 -> TopDownPerson
    tdkey = {**pkey, "top_down_method": 3}
    pl.TopDownMethod().insert1(tdkey)
    pl.TopDownPerson().populate(tdkey)
    assert np.array_equal((pl.TopDownPerson & tdkey).fetch1("keypoints"), kp)
    wmm._cache.clear()
    djshim.reset()
