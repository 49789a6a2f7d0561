"""The bottom-up stage on the CPU: the host grouping against tests/bottomup_ref.py on synthetic candidate lists, `oks_nms`,
`get_group_preds` and the size rule, the vendored config's settings, the HigherHRNet parameter inventory and program, and the
four tables on the shim.  The GPU side is tests/test_gpu_bottomup.py."""
import ctypes
import datetime
import json
import os

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd import bottomup as bu
from posepipeline_amd import djshim, pipeline as pl
from posepipeline_amd.models import higherhrnet as hh
from posepipeline_amd.models import hrnet, synth
from tests import bottomup_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arch_config_higherhrnet.json")
K, M = 17, 30


@pytest.fixture(autouse=True)
def clean():
    djshim.reset()
    yield
    djshim.reset()


# ---- 1. grouping ------------------------------------------------------------------------------------------------------------
def make_cand(entries):
    """entries: {joint: [(val, x, y, tag0, tag1), ...]} (already in descending val) -> cand [K][M][8] as the device returns it"""
    cand = np.zeros((K, M, 8), np.float32)
    cand[:, :, 1:3] = -1
    cand[:, :, 7] = -1
    for j, rows in entries.items():
        for m, (val, x, y, t0, t1) in enumerate(rows):
            cand[j, m] = (val, x, y, t0, t1, (x + y) % 2, (x + 2 * y) % 3 == 0, y * 48 + x)
    return cand


def persons_scenario(rng, tags, n_joints=K, drop=()):
    """one candidate per (person, joint) around the person's tag; drop: (person, joint) pairs without a candidate"""
    entries = {}
    for j in range(n_joints):
        rows = []
        for p, t in enumerate(tags):
            if (p, j) in drop:
                continue
            rows.append((float(rng.uniform(0.3, 0.95)), int(rng.integers(0, 48)), int(rng.integers(0, 32)),
                         t + float(rng.uniform(-0.05, 0.05)), t + float(rng.uniform(-0.05, 0.05))))
        entries[j] = sorted(rows, reverse=True)
    return entries


def scenarios():
    rng = np.random.default_rng(5)
    out = {}
    out["three_persons"] = persons_scenario(rng, (0.0, 3.0, 6.0))
    out["missing_joints"] = persons_scenario(rng, (0.0, 3.0, 6.0), drop={(0, 0), (1, 5), (2, 11), (2, 12), (0, 16)})
    # candidates at or below the detection threshold are not grouped.  mmpose compares in float64 (its rows are float64): the
    # float32 nearest to 0.1 lies ABOVE the float64 0.1 and is grouped, the float32 just below it is not
    e = persons_scenario(rng, (0.0, 3.0))
    e[3] = e[3] + [(0.1, 5, 5, 9.0, 9.0), (float(np.nextafter(np.float32(0.1), np.float32(0))), 7, 7, 15.0, 15.0), (0.05, 6, 6, 12.0, 12.0)]
    out["threshold"] = e
    # equal keys: two noses with the SAME tag dimension 0 share one dictionary key, the later one overwrites the earlier
    e = persons_scenario(rng, (0.0, 4.0))
    e[0] = [(0.9, 10, 10, 0.5, 0.1), (0.8, 30, 20, 0.5, 0.3), (0.7, 40, 5, 4.0, 4.0)]
    out["equal_key_merge"] = e
    # ... and in the `else` branch: an unmatched candidate whose tag dimension 0 equals an existing key lands in that group
    e = persons_scenario(rng, (0.0, 4.0), n_joints=3)
    k0 = np.float32(e[0][0][3])
    e[2] = e[2] + [(0.5, 7, 7, float(k0), 9.5)]
    out["equal_key_else_branch"] = e
    # distance to the group's mean tag just under / just over tag_threshold 1: joins / opens a new group
    base = {0: [(0.9, 10, 10, 0.0, 0.0)]}
    out["just_under_1"] = {**base, 1: [(0.8, 12, 10, 0.999, 0.0)]}
    out["just_over_1"] = {**base, 1: [(0.8, 12, 10, 1.001, 0.0)]}
    # more candidates than groups: the cost matrix is padded with 1e10 columns, the surplus opens groups
    e = persons_scenario(rng, (0.0, 3.0))
    e[1] = e[1] + [(0.29, 1, 1, 8.0, 8.0), (0.28, 2, 2, 11.0, 11.0), (0.27, 3, 3, 0.4, 0.3)]
    out["more_candidates_than_groups"] = e
    # the joint order: the hips (11, 12) come BEFORE the elbows (7, 8).  Seven joints at tag 0, hips at 0.9 pull the mean to 0.2,
    # so the elbow at 1.15 joins (0.95 < 1); in index order it would meet a mean of 0 and open a second group
    e = {j: [(0.9, 10 + j, 10, 0.0, 0.0)] for j in range(7)}
    e[11] = [(0.9, 20, 20, 0.9, 0.0)]
    e[12] = [(0.9, 22, 20, 0.9, 0.0)]
    e[7] = [(0.9, 15, 15, 1.15, 0.0)]
    out["joint_order"] = e
    # use_detection_val: two candidates at the same rounded distance compete for one group, the larger value wins it
    out["detection_val"] = {0: [(0.9, 10, 10, 0.0, 0.0)], 1: [(0.6, 11, 10, 0.3, 0.0), (0.5, 12, 10, 0.1, 0.0)]}
    # more than 30 groups: only the first 30 are matched against
    e = {0: [(0.9 - 0.01 * i, i, i, 3.0 * i, 0.0) for i in range(30)], 1: [(0.8, 1, 1, 0.0, 0.1)],
         2: [(0.9 - 0.01 * i, i, 2, 3.0 * i + 0.1, 100.0) for i in range(30)] + []}
    e[3] = [(0.7, 5, 5, 0.0, 100.0), (0.6, 6, 6, 0.05, 0.05)]
    out["thirty_groups"] = e
    out["empty"] = {}
    return out


SCENARIOS = scenarios()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_grouping_equals_the_reference(name):
    cand = make_cand(SCENARIOS[name])
    got = bu.match_by_tag(cand)
    want = ref.match_by_tag(cand[:, :, 0], cand[:, :, 1].astype(np.int64), cand[:, :, 2].astype(np.int64), cand[:, :, 3:5])
    assert got.dtype == np.float32 and got.shape == (len(want), K, 8)
    assert np.array_equal(got[:, :, [1, 2, 0, 3, 4]], want)
    # the extra columns travel with their candidate
    for p in got:
        for j in range(K):
            if p[j, 0] > 0:
                src = cand[j][(cand[j, :, 7] == p[j, 7])][0]
                assert np.array_equal(src, p[j])
            else:
                assert not p[j].any()
    n = {"three_persons": 3, "missing_joints": 3, "threshold": 3, "equal_key_merge": 2, "just_under_1": 1, "just_over_1": 2,
         "joint_order": 1, "detection_val": 2, "empty": 0, "equal_key_else_branch": 2}.get(name)
    if n is not None:
        assert len(got) == n, len(got)
    if name == "equal_key_merge":          # the second nose (x = 30) replaced the first in the shared group
        assert got[0, 0, 1] == 30 and got[0, 0, 4] == np.float32(0.3)
    if name == "joint_order":
        assert (got[0, [7, 11, 12], 0] > 0).all()
    if name == "threshold":
        assert got[2, 3, 0] == np.float32(0.1) and got[2, 3, 3] == 9.0 and not (got[:, :, 3] > 10).any()
    if name == "detection_val":            # cost round(d) * 100 - val: both round to 0, the 0.6 candidate takes the group
        assert got[0, 1, 0] == np.float32(0.6) and got[1, 1, 0] == np.float32(0.5)
    if name == "more_candidates_than_groups":
        assert len(got) >= 4
    if name == "thirty_groups":
        assert len(got) > 30


def test_adjust_from_the_bits():
    cand = make_cand(SCENARIOS["missing_joints"])
    persons = bu.match_by_tag(cand)
    xy = bu.adjust(persons)
    on = persons[:, :, 0] > 0
    assert on.any() and (~on).any()
    assert np.array_equal(xy[~on], np.zeros_like(xy[~on]))
    dx = xy[:, :, 0] - persons[:, :, 1]
    dy = xy[:, :, 1] - persons[:, :, 2]
    assert np.array_equal(dx[on], np.where(persons[:, :, 6][on] > 0, 0.75, 0.25).astype(np.float32))
    assert np.array_equal(dy[on], np.where(persons[:, :, 5][on] > 0, 0.75, 0.25).astype(np.float32))


# ---- 2. size rule, back-mapping, oks_nms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,want", [((1080, 1920), (960, 512)), ((1920, 1080), (512, 960)), ((100, 60), (512, 896))])
def test_size_rule(hw, want):
    h, w = hw
    wr, hr, c, s = bu.input_size(h, w, 512)
    rwr, rhr, rc, rs = ref.input_size(h, w, 512)
    assert (wr, hr) == (rwr, rhr) == want
    assert np.array_equal(c, rc) and np.array_equal(s, rs) and c.dtype == s.dtype == np.float64
    assert np.array_equal(c, [round(w / 2), round(h / 2)])
    # the transform is isotropic: both axes of the padded input cover scale * 200 source pixels
    assert abs(s[0] * 200 / wr - s[1] * 200 / hr) < 1e-12
    assert (s[0] * 200 == w) if w < h else (s[1] * 200 == h)
    wr2, hr2, _, _ = bu.input_size(h, w, 128)
    assert wr2 % 64 == 0 and hr2 % 64 == 0 and min(wr2, hr2) == 128


@pytest.mark.parametrize("hw", [(1080, 1920), (1920, 1080), (100, 60)])
def test_group_preds_and_oks_nms(hw):
    h, w = hw
    wr, hr, c, s = bu.input_size(h, w, 512)
    rng = np.random.default_rng(h)
    base = np.concatenate([rng.uniform(0, [wr, hr], (6, K, 2)), rng.uniform(0, 1, (6, K, 1))], axis=2).astype(np.float32)
    # persons 2 and 4 are near copies of persons 0 and 1 (a fraction of a pixel off): oks > 0.9, the lower score is dropped;
    # person 5 is person 3 moved by a tenth of the image: kept
    base[2, :, :2] = base[0, :, :2] + 0.3
    base[4, :, :2] = base[1, :, :2] - 0.2
    base[5, :, :2] = base[3, :, :2] + 0.1 * min(wr, hr)
    scores = np.array([0.5, 0.9, 0.7, 0.3, 0.6, 0.8], np.float32)
    got = bu.get_group_preds(base, c, s, wr, hr)
    want = ref.get_group_preds(base, c, s, wr, hr)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(got[..., 2], base[..., 2])
    # the corners of the padded input map back to a box centred on `center` that covers the frame
    corners = bu.get_group_preds(np.array([[[0, 0, 1], [wr, hr, 1]]], np.float32), c, s, wr, hr)[0]
    assert np.allclose((corners[0, :2] + corners[1, :2]) / 2, c) and (corners[1, :2] - corners[0, :2] >= [w - 1e-3, h - 1e-3]).all()
    keep = bu.oks_nms(got, scores)
    assert list(keep) == ref.oks_nms(list(want), scores) == [1, 5, 2, 3]
    assert len(bu.oks_nms(np.zeros((0, K, 3), np.float32), np.zeros(0))) == 0


# ---- 3. the vendored config -----------------------------------------------------------------------------------------------------
def test_spec_equals_the_vendored_config():
    g = json.load(open(GOLDEN))
    spec = hh.higher_hrnet48_coco_512x512()
    mine = json.loads(json.dumps(hh.vendored_config(spec)))
    for section in ("data_cfg", "backbone", "keypoint_head", "test_cfg", "normalize"):
        assert mine[section] == g[section], section
    assert g["source"].endswith("bottom_up/higherhrnet/coco/higher_hrnet48_coco_512x512.py") and g["model_type"] == "BottomUp"
    assert g["test_pipeline_is_val_pipeline"] and g["val_pipeline_types"] == ["LoadImageFromFile", "BottomUpGetImgSize", "BottomUpResizeAlign", "Collect"]
    # the constants the code reads are the config's
    t = g["test_cfg"]
    assert (spec.image_size, spec.width, spec.num_joints) == (g["data_cfg"]["image_size"], g["keypoint_head"]["in_channels"], t["num_joints"])
    assert bu.TEST_CFG["max_num_people"] == t["max_num_people"] == ref.MAX_PEOPLE == 30
    assert bu.TEST_CFG["detection_threshold"] == t["detection_threshold"] == ref.DET_THR
    assert bu.TEST_CFG["tag_threshold"] == t["tag_threshold"] == ref.TAG_THR
    assert (t["nms_kernel"], t["nms_padding"]) == (5, 2) and t["flip_test"] and t["adjust"] and t["refine"] and t["project2image"]
    assert "align_corners" not in t and bu.ALIGN_CORNERS is True          # test_cfg.get('align_corners', True)
    assert tuple(g["normalize"]["mean"]) == bu.MEAN and tuple(g["normalize"]["std"]) == bu.STD
    assert list(bu.JOINT_ORDER) == ref.JOINT_ORDER and list(hrnet.flip_perm(17)) == ref.FLIP_INDEX
    assert np.array_equal(bu.COCO_SIGMAS, ref.SIGMAS)
    assert os.path.basename(bu.CHECKPOINT) == "higher_hrnet48_coco_512x512-60fedcbc_20200712.pth"


# ---- 4. parameter inventory and program -------------------------------------------------------------------------------------------
def test_param_shapes():
    spec = hh.higher_hrnet48_coco_512x512()
    sh = hh.higherhrnet_param_shapes(spec)
    H = "keypoint_head."
    assert sh[H + "final_layers.0.weight"] == (34, 48, 1, 1) and sh[H + "final_layers.0.bias"] == (34,)
    assert sh[H + "deconv_layers.0.0.0.weight"] == (82, 48, 4, 4)
    assert all(sh[H + "deconv_layers.0.0.1." + s] == (48,) for s in ("weight", "bias", "running_mean", "running_var"))
    for i in range(4):
        assert sh[f"{H}deconv_layers.0.1.{i}.conv1.weight"] == sh[f"{H}deconv_layers.0.1.{i}.conv2.weight"] == (48, 48, 3, 3)
        assert sh[f"{H}deconv_layers.0.1.{i}.bn2.running_var"] == (48,)
    assert f"{H}deconv_layers.0.1.4.conv1.weight" not in sh
    assert sh[H + "final_layers.1.weight"] == (17, 48, 1, 1) and sh[H + "final_layers.1.bias"] == (17,)
    # the backbone is the pose HRNet's (multiscale_output=False: the last module has only fuse output 0)
    pose = hrnet.hrnet_backbone_shapes(hrnet.HRNetSpec(48, 17, 512, 512))
    assert {k: v for k, v in sh.items() if k.startswith("backbone.")} == pose
    assert not any(k.startswith("backbone.stage4.2.fuse_layers.1.") for k in sh)
    assert sum(1 for k in sh if k.startswith(H)) == 2 + 5 + 4 * 10 + 2


def test_program():
    spec = hh.HigherHRNetSpec(image_size=128, width=16)
    sd = synth.synth_state_dict(hh.higherhrnet_param_shapes(spec), seed=2)
    prog = hh.build_higherhrnet_program(spec, sd, 64, 128)
    assert prog.bufs[prog.named["input"]] == (64, 128, 4)
    assert prog.bufs[prog.named["output0"]] == (16, 32, 34) and prog.bufs[prog.named["output1"]] == (32, 64, 17)
    types = [op.type for op in prog.ops]
    assert L.PP_OP_DECONV_BF16 not in types and types.count(L.PP_OP_DEPTH_TO_SPACE) == 1
    d2s = prog.ops[types.index(L.PP_OP_DEPTH_TO_SPACE)]
    assert prog.bufs[d2s.in_] == (16, 32, 64) and prog.bufs[d2s.out] == (32, 64, 16)
    quad = [op for op in prog.ops if op.type == L.PP_OP_CONV and op.out == d2s.in_ and op.kh == 2]
    assert len(quad) == 4 and sorted(op.out_c_off for op in quad) == [0, 16, 32, 48] and all((op.kh, op.kw, op.cin) == (2, 2, 52) for op in quad)
    cat = quad[0].in_
    assert prog.bufs[cat] == (16, 32, 16 + 36) and all(op.in_ == cat for op in quad)
    writers = [op for op in prog.ops if op.out == cat and prog.op_names[list(prog.ops).index(op)].startswith("keypoint_head.cat.")]
    assert [(op.type, op.out_c_off, op.cout) for op in writers] == [(L.PP_OP_MAXPOOL, 0, 16), (L.PP_OP_CONV, 16, 36)]
    assert (writers[0].kh, writers[0].stride) == (1, 1)
    outs = [op for op in prog.ops if op.out_nchw]
    assert [(op.out, op.cout) for op in outs] == [(prog.named["output0"], 34), (prog.named["output1"], 17)]
    assert ctypes.sizeof(L.pp_op) == 120                      # no new pp_op field
    with pytest.raises(KeyError):
        hh.build_higherhrnet_program(spec, {k: v for k, v in sd.items() if k != "keypoint_head.final_layers.1.bias"}, 64, 128)
    bad = dict(sd)
    bad["keypoint_head.deconv_layers.0.0.0.weight"] = np.zeros((16, 50, 4, 4), np.float32)
    with pytest.raises(ValueError):
        hh.build_higherhrnet_program(spec, bad, 64, 128)


# ---- 5. the tables -------------------------------------------------------------------------------------------------------------------
def test_module_paths_and_table_exports():
    import pose_pipeline
    import pose_pipeline.wrappers.mmpose as mp
    import posepipeline_amd.wrappers.mmpose as mp2
    assert mp is mp2 and callable(mp.mmpose_bottom_up)
    for n in ("BottomUpMethodLookup", "BottomUpMethod", "BottomUpPeople", "BottomUpPerson"):
        assert n in pose_pipeline.__all__ and getattr(pose_pipeline, n) is getattr(pl, n)
    assert [r["bottom_up_method_name"] for r in pl.BottomUpMethodLookup().fetch(as_dict=True)] == [
        "OpenPose", "OpenPose_BODY25B", "OpenPose_HR", "OpenPose_LR", "MMPose", "Bridging_OpenPose"]
    assert pl.BottomUpMethodLookup.primary_key == ["bottom_up_method_name"]
    assert pl.BottomUpMethod.primary_key == pl.BottomUpPeople.primary_key == ["video_project", "filename", "bottom_up_method_name"]
    assert pl.BottomUpPeople.heading[-2:] == ["keypoints", "timestamp"]
    assert pl.BottomUpPerson.primary_key == pl.PersonBbox.primary_key + ["bottom_up_method_name"]
    assert pl.BottomUpPerson.heading[-1] == "keypoints"


def test_tables_with_the_wrapper_monkeypatched(monkeypatch):
    from posepipeline_amd.wrappers import mmpose as mp
    rng = np.random.default_rng(0)

    def person(x0, y0):
        kp = np.concatenate([rng.uniform([x0, y0], [x0 + 50, y0 + 100], (17, 2)), rng.uniform(0.3, 1, (17, 1))], axis=1).astype(np.float32)
        kp[0, :2], kp[1, :2] = (x0, y0), (x0 + 50, y0 + 100)
        return kp
    frames = [np.stack([person(10, 10), person(200, 50)]), np.zeros((0, 17, 3), np.float32), np.stack([person(205, 55)])]
    calls = []
    monkeypatch.setattr(mp, "mmpose_bottom_up", lambda key: calls.append(dict(key)) or frames)
    vkey = {"video_project": "p", "filename": "f"}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 5, 1)})
    mkey = {**vkey, "bottom_up_method_name": "MMPose"}
    pl.BottomUpMethod().insert1(mkey)
    pl.BottomUpPeople().populate(mkey)
    assert calls == [mkey]
    kps = (pl.BottomUpPeople & mkey).fetch1("keypoints")
    assert len(kps) == 3 and all(np.array_equal(a, b) for a, b in zip(kps, frames)) and kps[1].shape == (0, 17, 3)
    pkey = {**vkey, "tracking_method": 0, "video_subject_id": 0}
    bbox = np.array([[200.0, 50.0, 50.0, 100.0], [200.0, 50.0, 50.0, 100.0], [200.0, 50.0, 50.0, 100.0]])
    pl.PersonBbox().insert1({**pkey, "bbox": bbox, "present": np.ones(3, bool)})
    pl.BottomUpPerson().populate(pkey)
    got = (pl.BottomUpPerson & {**pkey, **mkey}).fetch1("keypoints")
    # rectangular: the frame without a person is a (17, 3) row of zeros (num_keypoints=17), not the default (25, 3)
    assert isinstance(got, np.ndarray) and got.shape == (3, 17, 3) and got.dtype != object
    assert np.array_equal(got[0], frames[0][1]) and not got[1].any() and np.array_equal(got[2], frames[2][0])


@pytest.mark.parametrize("method", ["OpenPose", "OpenPose_BODY25B", "Bridging_OpenPose"])
def test_other_bottom_up_methods_raise(method):
    vkey = {"video_project": "p", "filename": "f"}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 5, 1)})
    mkey = {**vkey, "bottom_up_method_name": method}
    pl.BottomUpMethod().insert1(mkey)
    with pytest.raises(Exception, match="Method not implemented"):
        pl.BottomUpPeople().populate(mkey)
    assert len(pl.BottomUpPeople()) == 0


# ---- 6. the reference's own float32 error is what the GPU bounds scale with ---------------------------------------------------------
@pytest.mark.parametrize("align", [True, False])
def test_reference_resize_vs_torch_float64(align):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 8, 12))
    for size in ((32, 48), (40, 56), (8, 12), (9, 30)):
        want = F.interpolate(torch.from_numpy(x), size=size, mode="bilinear", align_corners=align).numpy()
        got = ref.resize(x, size[0], size[1], align, np.float64)
        assert np.abs(got - want).max() <= 1e-14
        got32 = ref.resize(x.astype(np.float32), size[0], size[1], align, np.float32)
        want32 = F.interpolate(torch.from_numpy(x.astype(np.float32)), size=size, mode="bilinear", align_corners=align).numpy()
        # two float32 evaluations agree up to the rounding of the source coordinate (<= 2 ulp of the largest coordinate per axis,
        # times a slope of at most 2 max|x| per pixel) and of the four products and three sums of a sample
        amax = np.abs(x).max()
        assert got32.dtype == np.float32 and np.abs(got32 - want32).max() <= 2 * amax * 4 * 2.0 ** -23 * max(size) + 8 * 2.0 ** -24 * amax
