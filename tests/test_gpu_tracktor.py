"""The Tracktor method on the GPU against tests/tracktor_ref.py: the ECC kernels (csrc/ecc.hip), the RoI-head regression of given
boxes (pp_detector_regress) and the wrapper / table path end to end.

ECC tolerance: the GPU result is compared with the float64 reference on the float64 (analytic) images; the bound is FACTOR = 4
times the deviation of the SAME reference fed the float32-rounded images from that -- the convention of tests/test_gpu_hrformer.py.
The kernel reads float32 images and keeps float32 gradients; everything after is float64, as in the reference.  The observed
ratios are printed and recorded in DESIGN_LOG.md."""
import datetime
import functools

import numpy as np
import pytest

from oracle import detector as odet
from oracle import reid_mm as orm
from posepipeline_amd import _lib as L
from posepipeline_amd import ops
from posepipeline_amd.models import faster_rcnn as fr
from posepipeline_amd.models import reid_r50, synth
from tests import tracktor_ref as R
from tests.test_gpu_detector import synth_frame

pytestmark = pytest.mark.gpu

FACTOR = 4.0
MOTIONS, SHAPES = R.ECC_MOTIONS, R.ECC_SHAPES
IDENT = np.array([[1.0, 0, 0], [0, 1.0, 0]])


@functools.lru_cache(maxsize=None)
def ecc_case(h, w):
    """three (template, image) pairs of one shape: float64 images, and the float64 reference's result at 5 fixed iterations and at
    the configured rule, on the float64 and on the float32-rounded images"""
    pairs = R.ecc_test_pairs(h, w)
    out = dict(pairs=pairs)
    for name, (iters, eps) in (("fixed", (5, 0.0)), ("rule", (100, 1e-5))):
        out[name + "64"] = [R.ecc_euclidean(t, i, iters, eps) for t, i in pairs]
        out[name + "32"] = [R.ecc_euclidean(t.astype(np.float32), i.astype(np.float32), iters, eps) for t, i in pairs]
    return out


def run_ecc(ctx, images, pairs, iters, eps):
    imgs = np.ascontiguousarray(np.stack(images), np.float32)
    n, h, w = imgs.shape
    d = ctx.malloc(imgs.nbytes)
    try:
        ctx.h2d(d, imgs)
        return ops.ecc_euclidean(ctx, d, n, h, w, pairs, iters, eps)
    finally:
        ctx.free(d)


def interleaved(case):
    return [x for t, i in case["pairs"] for x in (t, i)], [(2 * k, 2 * k + 1) for k in range(len(case["pairs"]))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ecc_fixed_iterations_against_float64(ctx, shape):
    case = ecc_case(*shape)
    images, pairs = interleaved(case)
    warp, rho, iters, status = run_ecc(ctx, images, pairs, 5, 0.0)
    again = run_ecc(ctx, images, pairs, 5, 0.0)
    for a, b in zip((warp, rho, iters, status), again):
        assert a.tobytes() == b.tobytes(), "two runs differ"
    assert list(iters) == [5, 5, 5] and list(status) == [L.PP_ECC_OK] * 3
    for k, (r64, r32) in enumerate(zip(case["fixed64"], case["fixed32"])):
        assert r64[2] == 5 and r64[3] == R.ECC_OK
        for what, got, a64, a32 in (("warp", warp[k], r64[0], r32[0]), ("rho", rho[k], r64[1], r32[1])):
            dev = float(np.abs(np.asarray(a32) - np.asarray(a64)).max())
            err = float(np.abs(np.asarray(got) - np.asarray(a64)).max())
            print(f"ECC {shape[0]}x{shape[1]} pair {k} {what}: GPU vs float64 {err:.3e}, float32 images vs float64 {dev:.3e}, "
                  f"ratio {err / dev:.2f} (bound {FACTOR:g})")
            assert dev > 0 and err <= FACTOR * dev, (what, k, err, dev)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ecc_configured_rule_recovers_the_motion(ctx, shape):
    case = ecc_case(*shape)
    images, pairs = interleaved(case)
    warp, rho, iters, status = run_ecc(ctx, images, pairs, 100, 1e-5)
    assert list(status) == [L.PP_ECC_OK] * 3
    for k, (m, r64) in enumerate(zip(MOTIONS, case["rule64"])):
        th, t = float(np.arcsin(warp[k][1, 0])), warp[k][:, 2]
        print(f"ECC {shape[0]}x{shape[1]} pair {k}: {iters[k]} iterations (reference {r64[2]}), off the truth by "
              f"{np.abs(t - m[1:]).max():.2e} px, {abs(th - m[0]):.2e} rad; rho {rho[k]:.6f}")
        assert abs(int(iters[k]) - r64[2]) <= 1, (k, iters[k], r64[2])
        assert np.abs(t - m[1:]).max() <= 0.02 and abs(th - m[0]) <= 2e-4, (k, warp[k], m)
        assert warp[k][0, 0] == warp[k][1, 1] and warp[k][0, 1] == -warp[k][1, 0]
    # degenerate pairs in the same call: identical images -> the identity in 2 iterations; a constant input image -> the NaN
    # status; neither touches the other pairs
    h, w = shape
    const = np.full((h, w), 0.3, np.float32)
    images2 = images + [const]
    pairs2 = pairs[:1] + [(1, 1)] + pairs[1:2] + [(0, len(images))] + pairs[2:]
    warp2, rho2, iters2, status2 = run_ecc(ctx, images2, pairs2, 100, 1e-5)
    assert list(status2) == [L.PP_ECC_OK, L.PP_ECC_OK, L.PP_ECC_OK, L.PP_ECC_NAN, L.PP_ECC_OK]
    assert iters2[1] == 2 and np.abs(warp2[1] - IDENT).max() <= 1e-12 and abs(rho2[1] - 1) <= 1e-12
    assert np.isnan(rho2[3]) and iters2[3] == 1 and np.array_equal(warp2[3], IDENT)
    keep = [0, 2, 4]
    assert warp2[keep].tobytes() == warp.tobytes() and rho2[keep].tobytes() == rho.tobytes() and list(iters2[keep]) == list(iters)


def test_gray_from_nhwc4_bit_exact(ctx):
    x = np.random.default_rng(3).standard_normal((2, 33, 50, 4)).astype(np.float32)
    d_x, d_g = ctx.malloc(x.nbytes), ctx.malloc(2 * 33 * 50 * 4)
    ctx.h2d(d_x, x)
    ops.gray_from_nhwc4(ctx, d_x, 2, 33, 50, d_g)
    got = np.empty((2, 33, 50), np.float32)
    ctx.d2h(got, d_g)
    ctx.free(d_x)
    ctx.free(d_g)
    assert np.array_equal(got, R.gray_f32(x))


# ---- the clip: detector + ReID state dicts of the test's own, the reference chain once -------------------------------------------
CLIP_SEED = 5
CLS_BG_BIAS = 6.0      # picked on the CPU from the reference chain alone: a handful of detections per frame pass 0.5, and the chain
#                        contains propagated tracks and suppressed detections (asserted below)
OFFSETS = ((0, 0), (1, 0), (1, 1), (2, 1), (2, 2))     # integer camera motion over one larger canvas: ECC has a real motion to find


def clip_state_dicts():
    sd = synth.synth_state_dict(fr.faster_rcnn_param_shapes(), seed=2)
    # He-normal heads give saturated scores and e^4-sized boxes (tests/test_gpu_detector.py); the background logit's bias does for
    # the RoI head's class layer what yolox.seed_synthetic_head does for YOLOX: few boxes pass the tracker's 0.5
    for k, g in (("detector.rpn_head.rpn_cls.weight", 0.5), ("detector.rpn_head.rpn_reg.weight", 0.1),
                 ("detector.roi_head.bbox_head.fc_reg.weight", 0.2)):
        sd[k] = (sd[k] * g).astype(np.float32)
    sd["detector.roi_head.bbox_head.fc_cls.bias"][1] += np.float32(CLS_BG_BIAS)
    return sd, synth.synth_state_dict(reid_r50.reid_param_shapes(), seed=7)


def clip_frames():
    canvas = synth_frame(np.random.default_rng(CLIP_SEED), 135 + 8, 240 + 8)
    return np.stack([canvas[oy:oy + 135, ox:ox + 240] for ox, oy in OFFSETS])


@pytest.fixture(scope="module")
def clip():
    """frames, state dicts and the CPU reference (detector half per frame), computed once for the module"""
    det_sd, reid_sd = clip_state_dicts()
    frames = clip_frames()
    model = odet.FasterRCNNRef(det_sd)
    return dict(frames=frames, det_sd=det_sd, reid_sd=reid_sd, model=model, per_frame=R.reference_frames(model, frames))


def test_regress_matches_oracle_composition(ctx, clip):
    """5 boxes on frame 1 of a 2-frame pass (a frame offset into the resident FPN maps): one partly outside the image, one small
    enough for the finest level, the others on coarser levels; row i answers box i"""
    det = fr.Detector(ctx, clip["det_sd"], 135, 240, max_frames=2)
    dets = det.run(clip["frames"][:2])
    boxes = np.array([[-20.0, 30.0, 60.0, 110.0], [100.0, 50.0, 106.0, 59.0], [40.0, 10.0, 120.0, 130.0], [5.0, 5.0, 235.0, 130.0],
                      [150.5, 20.25, 200.75, 90.5]], np.float32)
    got_b, got_s = det.regress(1, boxes)
    mid = clip["per_frame"][1][1]
    ref_b, ref_s = R.regress_ref(clip["model"], mid["feats"], boxes, mid["scale_factor"])
    lv = odet.map_roi_levels((boxes * mid["scale_factor"][None, :]).astype(np.float32))
    assert lv.min() == 0 and lv.max() >= 2, lv
    assert np.array_equal(got_b, ref_b) and np.array_equal(got_s, ref_s), (np.abs(got_b - ref_b).max(), np.abs(got_s - ref_s).max())
    assert len(set(np.round(got_s, 6))) == 5                  # five different answers: no row served from another's slot
    # the pass's own outputs are what they were: the same pass again returns the same detections
    again = det.run(clip["frames"][:2])
    assert all(np.array_equal(a, b) for a, b in zip(dets, again))
    assert np.array_equal(dets[1], clip["per_frame"][1][0])
    with pytest.raises(L.PosePipeHipError, match="frame 2"):
        det.regress(2, boxes)
    det.close()


def test_wrapper_and_table_match_the_reference_chain(ctx, clip, tmp_path, monkeypatch):
    from posepipeline_amd import djshim, pipeline as pl, video
    from posepipeline_amd.wrappers import mmtrack as wmt
    reid = orm.ReidNetRef(clip["reid_sd"])
    memo = {}

    class Memo:                      # the second chain asks the same questions wherever its warps round to the same float32
        def forward(self, crops):
            key = crops.tobytes()
            if key not in memo:
                memo[key] = reid.forward(crops)
            return memo[key]
    # the reference chain: its ECC on the float64 gray images of the (float32) network inputs; the deviation: the same chain with its
    # ECC fed the gray images rounded to float32, which is what the device computes (R.gray_f32 = pp_gray_from_nhwc4, bit for bit)
    rows64, trk, warps, iters = R.reference_chain(clip["model"], Memo(), clip["per_frame"], R.gray_f64)
    rows32, _, _, _ = R.reference_chain(clip["model"], Memo(), clip["per_frame"], R.gray_f32)
    trace = trk.trace
    assert sum(len(t["propagated"]) for t in trace) >= 1 and sum(t["suppressed"] for t in trace) >= 1, trace
    assert [[int(r[0]) for r in f] for f in rows32] == [[int(r[0]) for r in f] for f in rows64]
    dev = max(float(np.abs(a[:, 1:] - b[:, 1:]).max()) for a, b in zip(rows64, rows32) if len(a))

    def fake_state_dict(relpath, shapes, seed, synth=None):
        assert relpath in ("mmtracking/checkpoints/faster-rcnn_r50_fpn_4e_mot17-ffa52ae7.pth", "mmtracking/checkpoints/reid_r50_6e_mot17-4bf6b63d.pth")
        return clip["det_sd"] if "faster-rcnn" in relpath else clip["reid_sd"]
    monkeypatch.setattr(wmt.weights, "get_state_dict", fake_state_dict)
    wmt._cache.clear()
    path = str(tmp_path / "v.ppvid")
    video.write_ppvid(path, clip["frames"], fps=30.0)
    tracks = wmt.mmtrack_bounding_boxes(path)                      # the signature's default method
    assert len(tracks) == 5
    print(f"ECC iterations per frame: wrapper {wmt.last_timing['ecc_iters']}, reference {iters[1:]}; "
          f"ids per frame {[[int(r[0]) for r in f] for f in rows64]}; reference float32-vs-float64 deviation {dev:.3e}")
    assert all(abs(a - b) <= 1 for a, b in zip(wmt.last_timing["ecc_iters"], iters[1:]))
    err = 0.0
    for f, (got, want) in enumerate(zip(tracks, rows64)):
        assert [d["track_id"] for d in got] == [int(r[0]) for r in want], f
        for d, r in zip(got, want):
            assert isinstance(d["track_id"], int)
            err = max(err, float(np.abs(d["tlbr"] - r[1:5]).max()), abs(float(d["confidence"]) - float(r[5])))
            assert np.array_equal(d["tlhw"], np.array([d["tlbr"][0], d["tlbr"][1], d["tlbr"][2] - d["tlbr"][0], d["tlbr"][3] - d["tlbr"][1]]))
    print(f"wrapper vs reference chain: boxes and scores off by {err:.3e} (bound {FACTOR:g} x {dev:.3e})")
    assert err <= FACTOR * dev, (err, dev)
    # the table path: tracking_method 1 = MMTrack_tracktor
    djshim.reset()
    vkey = {"video_project": "test", "filename": "tracktor_clip"}
    pl.Video().insert1({**vkey, "video": path, "start_time": datetime.datetime(2024, 1, 1)})
    tkey = {**vkey, "tracking_method": 1}
    pl.TrackingBboxMethod().insert1(tkey)
    pl.TrackingBbox().populate()
    stored = (pl.TrackingBbox & tkey).fetch1("tracks")
    assert (pl.TrackingBbox & tkey).fetch1("num_tracks") == len({d["track_id"] for f in tracks for d in f})
    assert len(stored) == 5
    for a, b in zip(stored, tracks):
        assert [d["track_id"] for d in a] == [d["track_id"] for d in b]
        assert all(np.array_equal(x["tlbr"], y["tlbr"]) and x["confidence"] == y["confidence"] for x, y in zip(a, b))
    wmt._cache.clear()
