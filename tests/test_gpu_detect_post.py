"""The detector's selection kernels (det_post.hip: rpn_select / rpn_compact / gather_kept / final_decode; nms.hip convention 0)
against the oracle BY COMPOSITION, under ties, saturation, empty frames and capped cuts.

tests/test_gpu_detector.py pins the image program and the RoI head bit for bit, so the oracle here is fed the GPU's OWN network
outputs: the RPN maps of net_a and the cls / reg rows of net_b (frame f's RoIs are rows f * 1000 ... of net_b: pp_detector_run runs
it on F * max_rois rows).  Given those, every selection is exact in BOTH numerics -- with the bit-exact kernels and with the default
(split) ones -- so each check is `==`.  The inputs (tests/tie_scenarios.py) change only the 1x1 head tensors; each scenario asserts
here, on the oracle side, that its edge really occurs."""
import numpy as np
import pytest

from oracle import detector as odet
from posepipeline_amd.models import faster_rcnn as fr
from tests import tie_scenarios as ts

pytestmark = pytest.mark.gpu
f32 = np.float32
NUMERICS = ("exact", "split")


@pytest.fixture(scope="module")
def scen():
    return ts.scenarios()


@pytest.fixture(scope="module")
def two_frames():
    rng = np.random.default_rng(2)
    return np.stack([ts.synth_frame(rng, ts.SRC_H, ts.SRC_W), ts.synth_frame(rng, ts.SRC_H, ts.SRC_W)])


@pytest.fixture(scope="module")
def bar_frames():
    return ts.frames_with_bars()


def compose(det, frames):
    """run the detector, then assert that its proposals and detections equal the oracle's selection applied to its own network
    outputs; -> per frame the views the edge assertions read"""
    F = frames.shape[0]
    dets, props = det.run(frames, want_proposals=True)
    rpn = [det.net_a.read(f"rpn{l}", F) for l in range(5)]          # fused head: channels 0 - 2 logits, 3 - 14 deltas
    cls = det.net_b.read("cls", F * det.MAX_ROIS).reshape(F, det.MAX_ROIS, 2)
    reg = det.net_b.read("reg", F * det.MAX_ROIS).reshape(F, det.MAX_ROIS, 4)
    sf = ts.scale_factor(det)
    views = []
    for f in range(F):
        cm, rm = [r[f][..., :3] for r in rpn], [r[f][..., 3:15] for r in rpn]
        p_ref, _ = odet.rpn_proposals(cm, rm)
        assert props[f].shape == p_ref.shape, (f, props[f].shape, p_ref.shape)
        assert np.array_equal(props[f], p_ref), f
        n = props[f].shape[0]
        d_ref = odet.final_detections(props[f], cls[f, :n], reg[f, :n], sf)
        assert dets[f].shape == d_ref.shape, (f, dets[f].shape, d_ref.shape)
        assert np.array_equal(dets[f], d_ref), f
        views.append(dict(cls_maps=cm, reg_maps=rm, props=props[f], cls=cls[f, :n], reg=reg[f, :n], dets=dets[f], sf=sf))
    return dets, props, views


def det_survivors(v):
    """final_detections up to its NMS: the scores of the kept boxes in kept order (before the 100 cut)"""
    scores = odet.softmax_fg(v["cls"])
    boxes = (odet.delta2bbox(v["props"], v["reg"], stds=(0.1, 0.1, 0.2, 0.2)) / v["sf"][None, :]).astype(f32)
    inds = np.nonzero(scores > f32(0.05))[0]
    keep = odet.batched_nms(boxes[inds], scores[inds], np.zeros(len(inds), np.int64), 0.5)
    return scores[inds][keep]


def assert_edge(edge, det, views):
    F = len(views)
    for f, v in enumerate(views):
        if edge == "rpn_cut_in_tie":        # level 0: more anchors equal the 1000th score than the cut takes
            assert ts.cut_in_tie(ts.level_scores(v["cls_maps"][0]), 1000), f
        elif edge == "rpn_all_tied":        # three runs of equal scores per level; level 4 (510 anchors) skips the top-k
            for l in range(4):
                assert ts.cut_in_tie(ts.level_scores(v["cls_maps"][l]), 1000), (f, l)
            s4 = ts.level_scores(v["cls_maps"][4])
            assert s4.shape == (510,) and len(np.unique(s4)) == 3, f
        elif edge == "some_dropped":        # empty boxes dropped from the middle of the candidate list, others kept
            _, boxes = ts.rpn_candidates(v["cls_maps"], v["reg_maps"])
            b = np.concatenate(boxes)
            valid = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
            assert 0 < valid.sum() < len(valid) and (~valid[:-1] & valid[1:]).any(), f
            assert len(v["props"]) > 0
        elif edge == "no_proposals":        # nothing survives the compaction: NMS, RoIAlign, the RoI head and the decode see 0 rows
            assert v["props"].shape == (0, 4) and v["dets"].shape == (0, 5), f
        elif edge == "rois_sample_nothing":  # every RoI lies outside the feature maps: RoIAlign returns zeros, every RoI scores alike
            assert len(v["props"]) > 0
            feats = [det.net_a.read(f"p{i}", F)[f: f + 1] for i in range(2, 6)]
            got, _ = odet.extract_roi_feats(feats, v["props"][:4])
            assert not got.any(), f
            assert (v["cls"] == v["cls"][0]).all(), f
        elif edge == "all_at_threshold":     # every RoI scores exactly 0.05: the strict > keeps none
            assert len(v["props"]) > 0 and (odet.softmax_fg(v["cls"]) == f32(0.05)).all() and len(v["dets"]) == 0, f
        elif edge == "det_cut_in_tie":       # more than 100 survivors of NMS .5, and the 100th and 101st tie
            kept = det_survivors(v)
            assert len(kept) > 100 and kept[99] == kept[100], (f, len(kept))
            assert len(v["dets"]) == 100
        else:
            raise AssertionError(edge)


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("name", ["saturated_rpn", "constant_rpn", "empty_one_type", "empty_all_types", "off_image",
                                  "threshold_eq", "threshold_up", "saturated_roi"])
def test_selection_matches_oracle_by_composition(ctx, scen, two_frames, name, numerics):
    sd, edge = scen[name]
    det = fr.Detector(ctx, sd, ts.SRC_H, ts.SRC_W, max_frames=2, numerics=numerics)
    assert det.net_a.numerics == det.net_b.numerics == numerics
    _, _, views = compose(det, two_frames)
    assert_edge(edge, det, views)


@pytest.mark.parametrize("numerics", NUMERICS)
def test_bar_frames_batch_equals_single_frames(ctx, bar_frames, numerics):
    """black, grey, pillarboxed, letterboxed and synthetic frames in one batch of a max_frames=8 detector: each frame's result
    equals the oracle's selection of its own maps and the result of a single-frame run; the async path equals `run`"""
    sd = ts.tamed_state_dict()
    det = fr.Detector(ctx, sd, ts.SRC_H, ts.SRC_W, max_frames=8, numerics=numerics)
    dets, props, views = compose(det, bar_frames)
    if numerics == "exact":       # the bars give bit-identical RPN scores: ties among the selected anchors
        for f in (0, 1, 2, 3):
            top = np.sort(ts.level_scores(views[f]["cls_maps"][0]))[::-1][:1000]
            assert len(np.unique(top)) < 1000, ts.FRAME_NAMES[f]
    for f in range(len(bar_frames)):
        d1, p1 = det.run(bar_frames[f: f + 1], want_proposals=True)
        assert np.array_equal(d1[0], dets[f]) and np.array_equal(p1[0], props[f]), ts.FRAME_NAMES[f]
    det.enqueue(bar_frames, want_proposals=True)
    d2, p2 = det.collect()
    assert all(np.array_equal(a, b) for a, b in zip(d2, dets)) and all(np.array_equal(a, b) for a, b in zip(p2, props))


def test_bar_frames_match_oracle_end_to_end(ctx, bar_frames):
    """two of the bar frames through the whole oracle (odet.detect), as tests/test_gpu_detector.py does for the synthetic ones"""
    sd = ts.tamed_state_dict()
    det = fr.Detector(ctx, sd, ts.SRC_H, ts.SRC_W, max_frames=2, numerics="exact")
    frames = bar_frames[[0, 2]]                                             # black, pillarbox
    dets, props = det.run(frames, want_proposals=True)
    model = odet.FasterRCNNRef(sd)
    for f in range(2):
        ref, mid = odet.detect(model, frames[f][:, :, ::-1], want_intermediates=True)
        assert np.array_equal(props[f], mid["proposals"]), f
        assert dets[f].shape == ref.shape and np.array_equal(dets[f], ref), f


@pytest.mark.parametrize("numerics", NUMERICS)
def test_run_order_leaves_no_stale_state(ctx, scen, bar_frames, numerics):
    """capped -> other -> capped on one detector equals a fresh detector per run (stale device counts or buffers would show).
    With the saturated RoI head the synthetic frame fills the 100 cut inside a tie; the black frame in between gives other boxes.
    (An EMPTY frame needs other head weights, which is another detector: the empty scenarios above run their frames as a batch.)"""
    sd, _ = scen["saturated_roi"]
    det = fr.Detector(ctx, sd, ts.SRC_H, ts.SRC_W, max_frames=2, numerics=numerics)
    seq = [bar_frames[4:5], bar_frames[0:1], bar_frames[4:5]]
    got = [det.run(x, want_proposals=True) for x in seq]
    for x, (d, p) in zip(seq, got):
        fresh = fr.Detector(ctx, sd, ts.SRC_H, ts.SRC_W, max_frames=2, numerics=numerics)
        dr, pr = fresh.run(x, want_proposals=True)
        fresh.close()
        assert np.array_equal(d[0], dr[0]) and np.array_equal(p[0], pr[0])
    n = [len(d[0]) for d, _ in got]
    assert n[0] == n[2] == 100 and np.array_equal(got[0][0][0], got[2][0][0]), n
    assert not np.array_equal(got[1][1][0], got[0][1][0])
