"""The tied / saturated / empty inputs of the selection tests, checked without a GPU: each scenario changes only the head tensors it
names and its edge holds by construction where that can be stated without a backbone; the vectorised NMS references equal the
plain oracles where those are defined (tests/tie_scenarios.py)."""
import numpy as np
import pytest

from oracle import boxes as obox
from oracle import detector as odet
from oracle import yolo as oyolo
from tests import tie_scenarios as ts

f32 = np.float32


@pytest.fixture(scope="module")
def scen():
    return ts.tamed_state_dict(), ts.scenarios()


def test_scenarios_change_only_the_head_tensors(scen):
    base, sc = scen
    assert len(sc) == 8
    for name, (sd, _) in sc.items():
        assert sd.keys() == base.keys()
        changed = {k for k in sd if sd[k] is not base[k] and not np.array_equal(sd[k], base[k])}
        assert changed and changed <= set(ts.HEAD_KEYS), (name, changed)
        assert all(sd[k].dtype == f32 and sd[k].shape == base[k].shape and np.isfinite(sd[k]).all() for k in changed), name


def test_threshold_biases_land_on_the_threshold():
    tb = ts.threshold_biases()
    thr = f32(0.05)
    eq = odet.softmax_fg(tb["eq"][None])[0]
    up = odet.softmax_fg(tb["up"][None])[0]
    assert eq == thr and not eq > thr                          # final_detections' strict > drops it
    assert up == np.nextafter(thr, f32(1)) and up > thr


def test_constant_rpn_ties_every_anchor_of_a_type(scen):
    base, sc = scen
    sd, _ = sc["constant_rpn"]
    assert not sd[ts.RPN_CLS_W].any()                          # logits = bias, bit for bit, whatever the features
    s = odet.sigmoid_f32(sd[ts.RPN_CLS_B])
    assert len(np.unique(s)) == 3 and np.argmax(s) == 1
    # 640 x 1088 input: one anchor of each type per position, so the level's scores are three runs of equal values; on levels
    # 0 - 3 the top-1000 cut falls inside one of them, level 4 (10 x 17 x 3 = 510) takes the natural-order branch of nms_pre
    sizes = [(640 // st) * (1088 // st) for st in odet.STRIDES]
    for lvl, n in enumerate(sizes):
        assert ts.cut_in_tie(np.repeat(s, n), 1000) == (lvl < 4), lvl
    assert sizes[4] * 3 == 510


def _anchor_boxes(dx, dy=(-3.0, 0.0, 3.0), dwh=(-odet.MAX_RATIO, 0.0, odet.MAX_RATIO)):
    """every anchor of every level of the 640 x 1088 input, decoded with each combination of the given deltas: -> [type][k][4]"""
    out = [[] for _ in range(3)]
    for lvl, st in enumerate(odet.STRIDES):
        a = odet.grid_anchors(640 // st, 1088 // st, st).reshape(-1, 3, 4)
        for t in range(3):
            for x in dx:
                for y in dy:
                    for w in dwh:
                        d = np.tile(np.array([[x, y, w, w]], f32), (a.shape[0], 1))
                        out[t].append(odet.delta2bbox(a[:, t], d))
    return [np.concatenate(o) for o in out]


def test_empty_proposal_deltas_collapse_the_boxes(scen):
    _, sc = scen
    b1 = sc["empty_one_type"][0][ts.RPN_REG_B]
    ball = sc["empty_all_types"][0][ts.RPN_REG_B]
    assert b1[4] == ts.DX_EMPTY and (ball[0::4] == ts.DX_EMPTY).all()
    big = [f32(ts.DX_EMPTY) * f32(1 - 1e-6), f32(ts.DX_EMPTY), f32(ts.DX_EMPTY) * f32(1 + 1e-6)]
    for t, boxes in enumerate(_anchor_boxes(big)):
        assert np.isfinite(boxes).all() and (boxes[:, 2] == boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all(), t
    # the other types of empty_one_type keep a positive width with the tamed deltas: dropped boxes sit mid-list
    for t in (0, 2):
        boxes = _anchor_boxes([b1[4 * t] - 3, b1[4 * t] + 3])[t]
        assert ((boxes[:, 2] - boxes[:, 0]) > 0).all(), t


def test_off_image_proposals_sample_nothing(scen):
    _, sc = scen
    b = sc["off_image"][0][ts.RPN_REG_B]
    assert (b[0::4] == ts.DX_OFF).all()
    for t, boxes in enumerate(_anchor_boxes([ts.DX_OFF - 3, ts.DX_OFF + 3])):
        assert (boxes[:, 0] > 1088 + 64).all(), t              # right of the padded input at every level's sampling grid
        assert ((boxes[:, 2] - boxes[:, 0]) <= 725 * np.exp(odet.MAX_RATIO)).all()     # sizes stay those of the anchors
    feats = [np.random.default_rng(l).standard_normal((1, 640 // st, 1088 // st, 8)).astype(f32)
             for l, st in enumerate(odet.STRIDES[:4])]
    rois = _anchor_boxes([ts.DX_OFF])[1][::20000][:6]
    got, _ = odet.extract_roi_feats(feats, rois)
    assert len(rois) == 6 and not got.any()


@pytest.mark.parametrize("n", [1, 2, 15, 63, 64, 65, 128, 129])
def test_vectorised_nms_references_equal_the_plain_oracles(n):
    for name, boxes, scores in ts.tie_box_sets(n):
        b, s = ts.to_convention(boxes, scores, 2)
        for thr in (0.3, 0.5):
            assert ts.tf_nms_all(b, s, thr) == oyolo.tf_nms(b, s, n, thr).tolist(), (name, thr)
        b, s = ts.to_convention(boxes, scores, 1)
        # numpy's default argsort (the reference's) is stable only for a handful of elements on SIMD builds: where it happens to
        # agree with the stable one on these scores, the plain restatement must give the same picks
        if n <= 15 and np.array_equal(np.argsort(s), np.argsort(s, kind="stable")):
            for thr in (0.3, 0.5, 1.0):
                assert obox.nms_deepsort_stable(b, thr, s) == obox.nms_deepsort(b, thr, s), (name, thr)
        elif n <= 2:
            raise AssertionError("np.argsort is not stable on two elements")


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 4096])
def test_tie_order_decides_the_kept_set(n):
    """the all-equal grid is a real test of the tie rule: reading the ties the other way round keeps a different set"""
    _, grid, scores = ts.tie_box_sets(n)[0]
    rev = grid[::-1]
    for conv, thr in ((0, 0.2), (1, 0.3), (2, 0.2)):
        b, s = ts.to_convention(grid, scores, conv)
        br, _ = ts.to_convention(rev, scores, conv)
        fwd = set(ts.nms_reference(b, s, thr, conv))
        back = {n - 1 - i for i in ts.nms_reference(br, s, thr, conv)}
        assert fwd != back, conv


def test_bar_frames():
    fr_ = ts.frames_with_bars()
    assert fr_.shape == (5, ts.SRC_H, ts.SRC_W, 3) and fr_.dtype == np.uint8
    black, grey, pillar, letter, _ = fr_
    assert not black.any() and (grey == 128).all()
    assert not pillar[:, :30].any() and not pillar[:, -30:].any() and pillar[:, 30:210].any()
    assert not letter[:16].any() and not letter[-17:].any() and letter[16:118].any()
