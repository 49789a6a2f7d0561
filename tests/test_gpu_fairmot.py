"""FairMOT stage on the GPU against tests/fairmot_ref.py.

Tolerances follow the project's convention: a GPU result is compared with the FLOAT64 reference, and the bound is FACTOR = 4 times
the deviation of the same reference evaluated in float32 on the CPU from float64 (float32 evaluations in another order).  The
deviation is computed here from the reference alone and asserted positive; the observed ratios are printed (DESIGN_LOG.md 5l).
Integer and selection steps (pre-processing, the transposed convolution, the decode's indices, boxes and scores) are bit-equal.

The 608 x 1088 pass: a float64 forward of the whole network on the CPU takes minutes at that size, so the full-size test holds
the LAST deformable convolution (64 -> 64 at 152 x 272: the largest grid of the DCN kernel) and the four head maps to float64 from
the maps the GPU left in front of them, and the whole pass in split numerics to the exact one; the whole network against float64
from the image is the 64 x 96 test.  The end-to-end tests compare with tests/golden/fairmot_e2e.npz, which
tests/golden/make_goldens_fairmot.py computed with the float64 chain (pre-processing -> float64 network -> decode ->
JDETrackerRef) at full network size."""
import os

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd import ops, video
from posepipeline_amd.models import dla
from posepipeline_amd.program import Net, ProgramBuilder
from tests import fairmot_ref as R

pytestmark = pytest.mark.gpu
FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "fairmot_e2e.npz")


def _bound(ref32, ref64, what):
    dev = float(np.abs(ref32.astype(np.float64) - ref64).max())
    assert dev > 0, what
    return FACTOR * dev, dev


def _check(got, ref32, ref64, what):
    bound, dev = _bound(ref32, ref64, what)
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{what}: GPU error {err:.3e}, float32-on-CPU deviation {dev:.3e}, ratio {err / dev:.2f}")
    assert err <= bound, (what, err, dev)
    return err / dev


# ---- PP_OP_DCN3X3 -----------------------------------------------------------------------------------------------------------------
def _dcn_net(ctx, h, w, cin, wt, b, relu):
    pb = ProgramBuilder()
    x = pb.buf(h, w, cin, name="x")
    om = pb.buf(h, w, 27, name="om")
    pb.mark_output(pb.dcn3x3(x, om, wt, b, relu=L.PP_RELU_LAST if relu else L.PP_RELU_NONE), "y")
    pb.mark_output(pb.conv(x, wt, b, pad=1, relu=L.PP_RELU_LAST if relu else L.PP_RELU_NONE), "conv")
    return Net(ctx, pb.build(), 1, numerics="exact")


def _offset_fields(rng, h, w):
    """name -> [h][w][27] float32"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = {}
    logits = lambda: rng.standard_normal((h, w, 9)).astype(np.float32)
    z = np.zeros((h, w, 27), np.float32)
    z[..., 18:] = logits()
    out["zero"] = z
    f = np.zeros((h, w, 27), np.float32)
    f[..., :18] = rng.uniform(-2, 2, (h, w, 18))
    f[..., 18:] = logits()
    out["fractional"] = f
    i = np.zeros((h, w, 27), np.float32)
    i[..., :18] = rng.integers(-2, 3, (h, w, 18))
    i[..., 18:] = logits()
    out["integer"] = i
    big = f.copy()                                   # whole taps outside, on both sides
    big[..., :18] += (rng.choice([-1.0, 0.0, 1.0], (h, w, 18)) * (max(h, w) + 5)).astype(np.float32)
    out["outside"] = big
    band = f.copy()                                  # samples in the bands (-1, 0) and (h - 1, h) / (w - 1, w)
    for k in range(9):
        ti = rng.choice(2, (h, w))
        ty = np.where(ti == 0, rng.uniform(-0.999, -0.001, (h, w)), rng.uniform(h - 0.999, h - 0.001, (h, w)))
        tx = np.where(rng.choice(2, (h, w)) == 0, rng.uniform(-0.999, -0.001, (h, w)), rng.uniform(w - 0.999, w - 0.001, (h, w)))
        use_y = rng.choice(2, (h, w)) == 0
        band[..., 2 * k] = np.where(use_y, ty - (yy - 1 + k // 3), band[..., 2 * k])
        band[..., 2 * k + 1] = np.where(~use_y, tx - (xx - 1 + k % 3), band[..., 2 * k + 1])
    out["bands"] = band.astype(np.float32)
    sat = f.copy()
    sat[..., 18:] = rng.choice([-30.0, 30.0], (h, w, 9))
    out["logits +-30"] = sat
    on = np.zeros((h, w, 27), np.float32)
    on[..., 18:] = 30.0
    out["zero, logits +30"] = on
    return out


@pytest.mark.parametrize("h,w,cin,cout", [(19, 34, 64, 64), (7, 5, 8, 24), (9, 70, 128, 64)])
def test_dcn3x3_against_float64(ctx, h, w, cin, cout):
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.standard_normal((h, w, cin)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    nets = {relu: _dcn_net(ctx, h, w, cin, wt, b, relu) for relu in (False, True)}
    ratios = []
    for n, (name, om) in enumerate(_offset_fields(rng, h, w).items()):
        for relu in (False, True):
            net = nets[relu]
            ctx.h2d(net.buffer("x")[0], x)
            ctx.h2d(net.buffer("om")[0], om)
            net.run(1)
            got = net.read("y", 1)[0]
            net.run(1)
            assert np.array_equal(got, net.read("y", 1)[0]), "two runs differ"
            ref64 = R.dcn3x3(x, om, wt, b, relu, np.float64)
            ref32 = R.dcn3x3(x, om, wt, b, relu, np.float32)
            ratios.append(_check(got, ref32, ref64, f"dcn3x3 {h}x{w} {cin}->{cout} {name} relu={relu}"))
            if name == "zero, logits +30":         # sigmoid(30) rounds to 1: an ordinary convolution
                conv = net.read("conv", 1)[0]
                bound, _ = _bound(ref32, ref64, name)
                assert np.abs(got.astype(np.float64) - conv).max() <= bound
                assert np.abs(conv.astype(np.float64) - ref64).max() <= bound
            if name == "outside":
                assert (np.abs(ref64 - (np.maximum(b, 0) if relu else b)).max(-1) > 0).any()       # not every pixel lost all taps
    print("dcn3x3 worst ratio", max(ratios))


# ---- PP_OP_DWDECONV ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,c", [(5, 7, 8), (3, 4, 64)])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_dwdeconv_is_bit_equal_to_the_float32_restatement(ctx, h, w, c, s):
    rng = np.random.default_rng(s * 100 + c)
    x = rng.standard_normal((h, w, c)).astype(np.float32)
    wt = rng.standard_normal((c, 1, 2 * s, 2 * s)).astype(np.float32)
    res = rng.standard_normal((h * s, w * s, c)).astype(np.float32)
    pb = ProgramBuilder()
    xi = pb.buf(h, w, c, name="x")
    ri = pb.buf(h * s, w * s, c, name="res")
    pb.mark_output(pb.dwdeconv(xi, wt, s), "y")
    pb.mark_output(pb.dwdeconv(xi, wt, s, res1=ri), "y_res")
    net = Net(ctx, pb.build(), 1, numerics="exact")
    ctx.h2d(net.buffer("x")[0], x)
    ctx.h2d(net.buffer("res")[0], res)
    net.run(1)
    ref = R.dwdeconv(x, wt, s, np.float32)
    assert ref.dtype == np.float32 and np.array_equal(net.read("y", 1)[0], ref)
    assert np.array_equal(net.read("y_res", 1)[0], ref + res)          # the fused add = the two steps done separately


# ---- pp_fairmot_preprocess --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1080, 1920), (48, 64), (90, 50)])
def test_preprocess_is_bit_equal(ctx, h, w):
    rng = np.random.default_rng(h)
    n = 1 if h == 1080 else 2
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    hp, wp = ops.fairmot_input_size(h, w)[:2]
    out = ctx.malloc(n * hp * wp * 16)
    try:
        ops.fairmot_preprocess(ctx, frames, out)
        got = np.empty((n, hp, wp, 4), np.float32)
        ctx.d2h(got, out)
    finally:
        ctx.free(out)
    for f in range(n):
        assert np.array_equal(got[f], R.preprocess(frames[f])), (h, w, f)


# ---- pp_fairmot_decode ------------------------------------------------------------------------------------------------------------
def _decode_case(rng, h, w, kind):
    hm = rng.uniform(-6, 1, (h, w, 1)).astype(np.float32)
    if kind == "ties":
        for y, x in ((2, 3), (5, 9), (8, 15), (h - 3, 4)):
            hm[y, x] = 2.5
    elif kind == "plateau":
        hm[4, 6:9] = 3.0
        hm[5, 6] = 3.0
    elif kind == "borders":
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0), (h - 1, w // 2 + 1), (h // 2 + 1, w - 1)):
            hm[y, x] = 4.0 + 0.01 * (y + x)
    wh = rng.uniform(0.5, 6, (h, w, 4)).astype(np.float32)
    reg = rng.uniform(0, 1, (h, w, 2)).astype(np.float32)
    idm = rng.standard_normal((h, w, 128)).astype(np.float32)
    return hm, wh, reg, idm


@pytest.mark.parametrize("h,w", [(12, 20), (19, 34)])
@pytest.mark.parametrize("K", [16, 100])
def test_decode(ctx, h, w, K):
    rng = np.random.default_rng(h * K)
    cases = [_decode_case(rng, h, w, kind) for kind in ("random", "ties", "plateau", "borders")]
    s = R.sigmoid(cases[0][0].reshape(-1), np.float32)       # the random case: pairwise distinct scores among all peaks
    _, _, inds0 = R.decode(*cases[0], h * w)
    peaks = inds0[inds0 >= 0]
    assert len(np.unique(s[peaks])) == len(peaks)
    n = len(cases)
    maps = [np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in range(4)]
    dev = [ctx.malloc(m.nbytes) for m in maps]
    try:
        for d, m in zip(dev, maps):
            ctx.h2d(d, m)
        dets, feats, inds = ops.fairmot_decode(ctx, dev[0], dev[1], dev[2], dev[3], n, h, w, K)
    finally:
        for d in dev:
            ctx.free(d)
    for f, kind in enumerate(("random", "ties", "plateau", "borders")):
        rd, rf64, ri = R.decode(*cases[f], K, np.float64)
        _, rf32, _ = R.decode(*cases[f], K, np.float32)
        assert inds[f].tolist() == ri.tolist(), kind
        assert np.array_equal(dets[f], rd), kind
        _check(feats[f], rf32, rf64, f"decode {h}x{w} K={K} {kind} embeddings")
        if kind == "ties":
            tied = [i for i in ri.tolist() if i >= 0 and cases[f][0].reshape(-1)[i] == np.float32(2.5)]
            assert len(tied) >= 2 and tied == sorted(tied)
        if kind == "plateau":
            assert {4 * w + 6, 4 * w + 7, 4 * w + 8, 5 * w + 6} <= set(ri.tolist())
        if kind == "borders":
            assert {0, w - 1, (h - 1) * w, h * w - 1} <= set(ri.tolist())
    if K == 100 and h == 12:
        assert (inds == -1).any() and not dets[inds == -1].any() and not feats[inds == -1].any()      # fewer peaks than K


# ---- network ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    return dla.synth_dla34_state_dict(dla.dla34_param_shapes(), 11)


def _image(rng, h, w):
    x = np.zeros((1, h, w, 4), np.float32)
    x[0, ..., :3] = rng.integers(0, 256, (h, w, 3)).astype(np.float32) / np.float32(255)
    return x


def _rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(a).max())


def test_network_64x96_against_float64_and_split_against_exact(ctx, seeded):
    x = _image(np.random.default_rng(8), 64, 96)
    ref64 = R.Dla34Ref(seeded, np.float64).forward(x[0])
    ref32 = R.Dla34Ref(seeded, np.float32).forward(x[0])
    prog = dla.build_dla34_program(seeded, 64, 96)
    exact = Net(ctx, prog, 1, numerics="exact")
    exact.forward(x, out_name="hm")
    got = {k: exact.read(k, 1)[0] for k, _ in dla.HEADS}
    for k, _ in dla.HEADS:
        _check(got[k], ref32[k], ref64[k], f"DLA-34 64x96 exact head {k}")
    split = Net(ctx, prog, 1, numerics="split")
    assert (split.conv_kinds() == 2).any()
    split.forward(x, out_name="hm")
    for k, _ in dla.HEADS:
        r = _rel(got[k], split.read(k, 1)[0])
        print(f"DLA-34 64x96 split vs exact head {k}: {r:.2e}")
        assert r <= 2e-5, (k, r)


def test_network_full_size_pass(ctx, seeded):
    keep = ("ida_up.up_2", "ida_up.node_2.conv.conv_offset_mask", "ida_up.node_2.conv")
    prog = dla.build_dla34_program(seeded, 608, 1088, keep=keep)
    x = _image(np.random.default_rng(9), 608, 1088)
    exact = Net(ctx, prog, 1, numerics="exact")
    exact.forward(x, out_name="hm")
    xin, om, feat = (exact.read(k, 1)[0] for k in keep)
    got = {k: exact.read(k, 1)[0] for k, _ in dla.HEADS}
    assert feat.shape == (152, 272, 64) and np.isfinite(feat).all()
    wf, bf = R.fold_bn(*[seeded["ida_up.node_2." + k] for k in ("conv.weight", "conv.bias", "actf.0.weight", "actf.0.bias",
                                                                  "actf.0.running_mean", "actf.0.running_var")])
    _check(feat, R.dcn3x3(xin, om, wf, bf, True, np.float32), R.dcn3x3(xin, om, wf, bf, True, np.float64), "full-size DCN 64->64 at 152x272")
    for k, _ in dla.HEADS:
        h64, h32 = [R.conv2d(np.maximum(R.conv2d(feat, seeded[k + ".0.weight"], seeded[k + ".0.bias"], 1, 1, dt), 0),
                             seeded[k + ".2.weight"], seeded[k + ".2.bias"], 1, 0, dt) for dt in (np.float64, np.float32)]
        _check(got[k], h32, h64, f"full-size head {k}")
    n_cand = int((R.sigmoid(got["hm"], np.float32) > 0.2).sum())
    print("full-size pass: cells with sigmoid(hm) > 0.2:", n_cand)
    del exact
    split = Net(ctx, dla.build_dla34_program(seeded, 608, 1088), 1, numerics="split")
    split.forward(x, out_name="hm")
    for k, _ in dla.HEADS:
        r = _rel(got[k], split.read(k, 1)[0])
        print(f"DLA-34 608x1088 split vs exact head {k}: {r:.2e}")
        assert r <= 2e-5, (k, r)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def synthetic(monkeypatch, tmp_path):
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path / "no_checkpoints"))
    from posepipeline_amd.wrappers import fairmot as w
    w._cache.clear()
    yield w
    w._cache.clear()


def _rows(tracks):
    return [[(t["track_id"], t["tlhw"], t["confidence"]) for t in fr] for fr in tracks]


def test_wrapper_and_table_row_against_the_reference_chain(ctx, synthetic, tmp_path):
    """tests/golden/fairmot_e2e.npz: per frame the ids, tlwh (source pixels) and scores of the float64 chain and of the same chain
    with the network in float32 (their difference, times FACTOR, bounds boxes and scores).  The generator asserts that no
    candidate's score of either chain is within 1e-3 of conf_thres = 0.2 (float32 noise of a score is 1e-6), so the candidate sets
    are equal.  Comparison rule for ids: a track id is the rank of its first detection's score among the frame's new tracks, and
    the seeded network gives some candidates scores 1e-6 apart, inside float32 noise, so two evaluations may number the same
    tracks differently; the tracks are therefore matched to the reference's by their first box (fairmot_ref.relabel, one to one)
    and must then carry the matched id in EVERY frame."""
    g = np.load(GOLDEN)
    frames = R.rectangles_clip(6, 64, 96, seed=int(g["seed"]))
    path = str(tmp_path / "clip.ppvid")
    video.write_ppvid(path, frames, 30.0)
    got = _rows(synthetic.fairmot_bounding_boxes(path))
    assert len(got) == 6
    ref = [[(int(i), b, float(s)) for i, b, s in zip(g[f"ids{f}"], g[f"tlwh64_{f}"], g[f"score64_{f}"])] for f in range(6)]
    same_numbering = [[r[0] for r in fr] for fr in got] == [[r[0] for r in fr] for fr in ref]
    print("end to end: ids numbered as the reference's without relabelling:", same_numbering)
    matched = R.relabel(got, ref)
    n_boxes = 0
    for f in range(6):
        ids, b64, b32, s64, s32 = (g[f"{k}{f}"] for k in ("ids", "tlwh64_", "tlwh32_", "score64_", "score32_"))
        by_id = {r[0]: r for r in matched[f]}
        assert sorted(by_id) == sorted(ids.tolist()) and len(by_id) == len(matched[f]), f
        if len(ids):
            n_boxes += len(ids)
            _check(np.array([by_id[i][1] for i in ids.tolist()]), b32, b64, f"end to end frame {f} boxes")
            if np.abs(s32 - s64).max() > 0:
                _check(np.array([by_id[i][2] for i in ids.tolist()]), s32, s64, f"end to end frame {f} scores")
    assert n_boxes > 0
    # the table row gives the same tracks, and a second call starts ids at 1 again
    import datetime
    from posepipeline_amd import djshim, pipeline as pl
    djshim.reset()
    try:
        tkey = {"video_project": "p", "filename": "f", "tracking_method": 2}
        pl.Video().insert1({"video_project": "p", "filename": "f", "video": path, "start_time": datetime.datetime(2024, 5, 1)})
        pl.TrackingBboxMethod().insert1(tkey)
        pl.TrackingBbox().populate()
        tracks, num = (pl.TrackingBbox & tkey).fetch1("tracks", "num_tracks")
    finally:
        djshim.reset()
    again = _rows(tracks)
    assert [[r[0] for r in fr] for fr in again] == [[r[0] for r in fr] for fr in got]
    assert all(np.array_equal(a[1], b[1]) and a[2] == b[2] for fa, fb in zip(again, got) for a, b in zip(fa, fb))
    all_ids = sorted({r[0] for fr in got for r in fr})
    assert num == len(all_ids) and all_ids[0] == 1


def test_portrait_clip_returns_boxes_in_source_pixels(ctx, synthetic, tmp_path):
    frames = R.rectangles_clip(3, 96, 64, seed=3)
    path = str(tmp_path / "portrait.ppvid")
    video.write_ppvid(path, frames, 30.0)
    tracks = synthetic.fairmot_bounding_boxes(path)
    assert len(tracks) == 3 and ops.fairmot_input_size(96, 64)[:2] == (1088, 608)
    boxes = np.array([t["tlbr"] for fr in tracks for t in fr]).reshape(-1, 4)
    assert len(boxes) > 0
    for fr in tracks:
        for t in fr:
            assert isinstance(t["track_id"], int) and isinstance(t["confidence"], float) and t["confidence"] > 0.2
            np.testing.assert_allclose(t["tlbr"], np.r_[t["tlhw"][:2], t["tlhw"][:2] + t["tlhw"][2:]], rtol=0, atol=1e-9)
    # frame 1 activates every detection at once, in detection order: its boxes are the detector's boxes of the 1920 x 1080 frame
    # times (64 / 1920, 96 / 1080)
    ctx2, det = next(iter(synthetic._cache.values()))
    dets, _ = det.run(frames[:1])[0]
    assert len(dets) == len(tracks[0]) > 0
    want = dets[:, :4].astype(np.float64) * np.array([64 / 1920, 96 / 1080] * 2)
    np.testing.assert_allclose(np.array([t["tlbr"] for t in tracks[0]]), want, rtol=0, atol=1e-9)
    assert [t["confidence"] for t in tracks[0]] == [float(s) for s in dets[:, 4]]
    assert sorted({t["track_id"] for t in tracks[0]})[0] == 1
