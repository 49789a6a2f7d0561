"""tests/roi_align_cases.py without a GPU: the reference is the oracle (float32 mode bit for bit), pins the sample geometry on ramp
maps in closed form, and every RoI family is what its builder says -- levels, which bins are nonzero, zero rows, the variety of column
windows.  tests/test_gpu_roi_align.py compares the two RoIAlign kernels with these references."""
import numpy as np
import pytest

from oracle import detector as odet
from posepipeline_amd.models import faster_rcnn as fr
from tests import roi_align_cases as RC

f32, f64 = np.float32, np.float64
NONZERO_FAMILIES = [n for n in RC.FAMILY_NAMES if n not in RC.ZERO_FAMILIES]


def nonzero_bins(ref):
    return int(np.any(ref != 0, axis=-1).sum())


def test_geometry_and_scale_factors():
    assert fr.detector_input_size(RC.SRC_H, RC.SRC_W) == RC.INPUT_SIZE
    assert odet.rescale_size(RC.SRC_W, RC.SRC_H) == (RC.INPUT_SIZE[1], RC.INPUT_SIZE[0])
    sfx, sfy = f32(RC.INPUT_SIZE[1] / RC.SRC_W), f32(RC.INPUT_SIZE[0] / RC.SRC_H)       # pp_detector_create: (float)((double)nw / src_w)
    assert sfx == sfy == 4
    assert RC.MAP_HW == tuple((RC.IMG_H // s, RC.IMG_W // s) for s in RC.STRIDES) and RC.STRIDES == tuple(odet.STRIDES[:4])
    for name in RC.FAMILY_NAMES:
        RC.source_boxes(RC.families()[name])            # asserts the round trip through source pixels
    a, b = RC.feature_maps(0), RC.feature_maps(1)
    assert all(x.shape == (h, w, RC.C) and x.dtype == f32 for x, (h, w) in zip(a, RC.MAP_HW))
    assert not np.array_equal(a[3], b[3])
    # every channel its own scale and offset
    assert np.allclose(a[0].reshape(-1, RC.C).mean(0), 0.01 * np.arange(RC.C), atol=0.15)
    assert np.allclose(a[0].reshape(-1, RC.C).std(0), 1 + np.arange(RC.C) % 7, rtol=0.03)


@pytest.mark.parametrize("name", RC.FAMILY_NAMES)
def test_float32_mode_is_the_oracle_bit_for_bit(name):
    """roi_align_ref(float32) == oracle.detector.roi_align, every RoI with a defined level, both frames"""
    rois = RC.families()[name]
    for frame in range(RC.N_FRAMES):
        ref, maps = RC.reference(frame, name), RC.feature_maps(frame)
        for i in RC.defined(name):
            lv = int(ref["levels"][i])
            got = RC.roi_align_ref(maps[lv], rois[i], 1.0 / RC.STRIDES[lv], f32)
            assert got.dtype == f32 and np.array_equal(got.view(np.uint32), ref["ref32"][i].view(np.uint32)), (name, frame, i)


def test_ramp_bins_equal_the_ramp_at_the_bin_centre():
    """the bin average of a linear function is the function at the bin's centre in real arithmetic; the RoIs' positions are exact in
    float32, so only float64 rounding remains: 1e-9 relative.  Pins the sample geometry independently of any loop order."""
    a, b, d = RC.ramp_coefficients()
    levels = odet.map_roi_levels(RC.RAMP_ROIS)
    assert levels.tolist() == [0, 1, 2, 3, 0]
    for roi, lv in zip(RC.RAMP_ROIS, levels):
        info = {}
        got = RC.roi_align_ref(RC.ramp_maps()[lv], roi, 1.0 / RC.STRIDES[lv], f64, info)
        h, w = RC.MAP_HW[lv]
        assert info["n_valid"] == info["n_samples"] and info["gh"] * info["gw"] >= 4
        assert 0 < info["cols"][0] and info["cols"][1] < w - 1 and 0 < info["rows"][0] and info["rows"][1] < h - 1      # interior
        x1, y1, x2, y2 = (float(v) / RC.STRIDES[lv] - 0.5 for v in roi)
        cx = x1 + (np.arange(7) + 0.5) * (x2 - x1) / 7
        cy = y1 + (np.arange(7) + 0.5) * (y2 - y1) / 7
        want = a[None, None, :] * cx[None, :, None] + b[None, None, :] * cy[:, None, None] + d[None, None, :]
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (roi, np.abs(got - want).max())


def test_levels_family():
    rois = RC.families()["levels"]
    ref = RC.reference(0, "levels")
    lv = ref["levels"].tolist()
    sides = (rois[:7, 2] - rois[:7, 0]).tolist()
    assert sides == [float(f32(s)) for s in RC.LEVEL_SIDES] and np.array_equal(rois[:7, 3] - rois[:7, 1], rois[:7, 2] - rois[:7, 0])
    for s, l_ in zip(sides, lv):
        if s in RC.LEVELS_CLEAN:
            assert l_ == RC.LEVELS_CLEAN[s], (s, l_)
    assert [lv[i] for i in (0, 2, 3, 4, 5, 6)] == [0, 1, 1, 2, 2, 3]
    # the side just below 112: the 1e-6 term alone puts it on level 1
    assert 111.9999 < sides[1] < 112 and lv[1] == 1 and RC.level_without_epsilon(rois)[1] == 0
    assert np.array_equal(np.delete(RC.level_without_epsilon(rois), 1), np.delete(ref["levels"], 1))
    assert lv[7] == 3 and lv[8] == 0                    # the 3000-pixel square clamps to 3, the 0.5-pixel square to 0
    assert ref["info"][7]["gh"] == 14 and 0 < ref["info"][7]["n_valid"] < ref["info"][7]["n_samples"]
    assert ref["info"][8]["gh"] == ref["info"][8]["gw"] == 1
    assert all(nonzero_bins(r) == 49 for r in ref["ref64"][[0, 1, 2, 3, 4, 5, 6, 8]])


def test_window_family():
    rois = RC.families()["window"]
    ref = RC.reference(0, "window")
    assert (ref["levels"] == 0).all()
    widths = []
    for i, k in enumerate(RC.WINDOW_K):
        info = ref["info"][i]
        assert info["gh"] == 1 and info["n_valid"] == info["n_samples"] and info["rows"] == (74, 77)
        widths.append(info["cols"][1] - info["cols"][0] + 1)
        assert k + 1 <= widths[-1] <= k + 2            # k columns of samples and the bilinear neighbours
    assert widths[0] <= 3 and widths[-1] > 4 * 64                   # from two or three columns to beyond four 64-lane rounds
    assert {wd % 4 for wd in widths} == {0, 1, 2, 3}                 # every tail of the four-column loop
    full, vert = ref["info"][len(RC.WINDOW_K)], ref["info"][len(RC.WINDOW_K) + 1]
    assert rois[len(RC.WINDOW_K)].tolist() == [0, 200, 1088, 208] and full["gw"] == 39 and full["gh"] == 1 and full["cols"] == (0, 271)
    assert rois[len(RC.WINDOW_K) + 1].tolist() == [500, 0, 508, 640] and vert["gh"] == 23 and vert["gw"] == 1 and vert["rows"] == (0, 159)
    assert all(nonzero_bins(r) == 49 for r in ref["ref64"])


def test_edges_family():
    rois = RC.families()["edges"]
    for frame in range(RC.N_FRAMES):
        ref = RC.reference(frame, "edges")
        for i, (roi, want) in enumerate(RC.EDGES_STATED):
            assert rois[i].tolist() == list(roi) and ref["levels"][i] == 0
            assert nonzero_bins(ref["ref64"][i]) == nonzero_bins(ref["ref32"][i]) == want, (i, roi)
    ref = RC.reference(0, "edges")
    info = ref["info"]
    assert info[0]["cols"][0] == 0 and info[2]["cols"] == (271, 271) and info[4]["rows"][0] == 0 and info[6]["rows"] == (159, 159)
    # which bins: the first column / row of bins is the empty one at -4.5, the only one left at 1088 / 640
    assert not ref["ref64"][1][:, 0].any() and ref["ref64"][1][:, 1:].any(axis=-1).all()
    assert ref["ref64"][2][:, 0].any(axis=-1).all() and not ref["ref64"][2][:, 1:].any()
    assert not ref["ref64"][5][0].any() and ref["ref64"][5][1:].any(axis=-1).all()
    assert ref["ref64"][6][0].any(axis=-1).all() and not ref["ref64"][6][1:].any()
    n0 = len(RC.EDGES_STATED)
    assert ref["levels"][n0:].tolist() == RC.EDGES_STRADDLE_LEVELS
    for j in range(len(RC.EDGES_STRADDLE)):
        i, (h, w) = info[n0 + j], RC.MAP_HW[RC.EDGES_STRADDLE_LEVELS[j]]
        assert 0 < i["n_valid"] < i["n_samples"]
        side = j % 4                                      # left, right, top, bottom
        assert (i["cols"][0] == 0, i["cols"][1] == w - 1, i["rows"][0] == 0, i["rows"][1] == h - 1) == tuple(s == side for s in range(4)), j


def test_outside_huge_and_degenerate_families():
    for frame in range(RC.N_FRAMES):
        for name in RC.ZERO_FAMILIES:
            ref = RC.reference(frame, name)
            assert not ref["ref32"].any() and not ref["ref64"].any()
    out = RC.reference(0, "outside")
    assert all(i["n_valid"] == 0 and i["n_samples"] > 0 for i in out["info"])
    # above and below: x is inside the map (not the separable kernel's `empty` branch, which looks at x alone); left and right: x outside
    rois, lv = RC.families()["outside"], out["levels"]
    for i in (2, 3):
        assert 0 <= rois[i][0] / RC.STRIDES[lv[i]] and rois[i][2] / RC.STRIDES[lv[i]] <= RC.MAP_HW[lv[i]][1]
    deg = RC.reference(0, "degenerate")
    assert deg["levels"].tolist() == [0, 0, 0, 0, -1, -1] and RC.defined("degenerate") == [0, 1, 2, 3]
    assert [(i["gw"] < 1, i["gh"] < 1) for i in deg["info"][:4]] == [(True, False), (False, True), (True, True), (True, True)]
    d = RC.families()["degenerate"]
    assert (d[4, 2] < d[4, 0] and d[4, 3] > d[4, 1]) and (d[5, 2] > d[5, 0] and d[5, 3] < d[5, 1])
    huge = RC.reference(0, "huge")
    assert huge["levels"].tolist() == [3, 3]
    assert [i["gh"] * i["gw"] for i in huge["info"]] == [11 * 19, 4 * 41]
    assert all(i["cols"] == (0, 33) and i["rows"] == (0, 19) and 0 < i["n_valid"] < i["n_samples"] for i in huge["info"])


def test_generic_and_pair_families():
    rois = RC.families()["generic"]
    ref = RC.reference(0, "generic")
    assert len(rois) == 24 and (rois != np.round(rois)).all(axis=1).all()          # fractional corners
    assert np.bincount(ref["levels"], minlength=4).min() >= 4
    crossing = [0 < i["n_valid"] < i["n_samples"] for i in ref["info"]]
    assert sum(crossing) >= 8 and sum(not c for c in crossing) >= 8
    assert all(nonzero_bins(r) > 0 for r in ref["ref64"])
    pair = RC.reference(0, "pair")
    assert np.array_equal(RC.families()["pair"], rois[:2]) and np.array_equal(pair["ref64"], ref["ref64"][:2])


@pytest.mark.parametrize("name", NONZERO_FAMILIES)
def test_float32_deviation_is_positive(name):
    """what the separable kernel's error is measured against: max |ref32 - ref64| over the family, per frame"""
    for frame in range(RC.N_FRAMES):
        ref = RC.reference(frame, name)
        assert np.abs(ref["ref32"].astype(f64) - ref["ref64"]).max() > 0, (name, frame)
