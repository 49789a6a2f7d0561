"""The SMPL stage on the CPU: tables, recipe, box helpers, the body-model data and the references of tests/vibe_ref.py.
(The device code is held by tests/test_gpu_vibe.py.)"""
import datetime
import inspect
import json
import os
import sys
import types

import numpy as np
import pytest

from posepipeline_amd import djshim, pipeline as pl
from posepipeline_amd.models import smpl as S
from posepipeline_amd.models import vibe as VM
from posepipeline_amd.utils import bounding_box as BB
from tests import vibe_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def clean():
    djshim.reset()
    yield
    djshim.reset()


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
def test_tables_exist_and_are_exported():
    import pose_pipeline
    import pose_pipeline.pipeline as ref_pl
    for name in ("SMPLMethodLookup", "SMPLMethod", "SMPLPerson"):
        assert getattr(pose_pipeline, name) is getattr(pl, name) and getattr(ref_pl, name) is getattr(pl, name)
        assert name in pose_pipeline.__all__
    ns = {}
    exec("from pose_pipeline import *", ns)
    assert {"SMPLMethodLookup", "SMPLMethod", "SMPLPerson"} <= set(ns)
    assert pl.SMPLMethod.primary_key == pl.PersonBbox.primary_key + ["smpl_method"]
    assert pl.SMPLPerson.primary_key == pl.SMPLMethod.primary_key
    assert pl.SMPLPerson.heading[-6:] == ["model_type", "cams", "poses", "betas", "joints3d", "joints2d"]      # no `verts` column


def test_lookup_rows_are_the_reference_rows():
    rows = sorted(pl.SMPLMethodLookup().fetch(as_dict=True), key=lambda r: r["smpl_method"])
    assert [(r["smpl_method"], r["smpl_method_name"]) for r in rows] == [
        (0, "VIBE"), (1, "MEVA"), (2, "ProHMR"), (3, "Expose"), (4, "PARE"), (5, "PIXIE"), (6, "ProHMR_MMPose"), (7, "HybrIK")]


def test_joint_names_equal_the_golden_list():
    with open(os.path.join(HERE, "golden", "joint_names_49.json")) as f:
        want = json.load(f)
    assert len(want) == 49
    assert pl.SMPLPerson.joint_names() == want and pl.SMPLPerson.joint_names(model="SMPL") == want
    assert len(S.JOINT_MAP_54) == 49 and max(S.JOINT_MAP_54) == 53 and min(S.JOINT_MAP_54) == 0
    # the same joint under its OpenPose and its ground-truth name
    name = {n: i for i, n in enumerate(want)}
    for a, b in (("OP Nose", "Nose"), ("OP RKnee", "Right Knee"), ("OP LWrist", "Left Wrist"), ("OP REar", "Right Ear")):
        assert S.JOINT_MAP_54[name[a]] == S.JOINT_MAP_54[name[b]]
    assert len(set(S.VERTEX_IDS_SMPLH)) == 21 and max(S.VERTEX_IDS_SMPLH) < S.N_VERTS


def _video_with_tracks(tmp_path, monkeypatch, vkey, tracks):
    from posepipeline_amd import video
    import posepipeline_amd.wrappers as W
    path = str(tmp_path / (vkey["filename"] + ".ppvid"))
    video.write_ppvid(path, np.zeros((len(tracks), 32, 48, 3), np.uint8), 30.0)
    pl.Video.insert1({**vkey, "video": path, "start_time": datetime.datetime(2024, 5, 1)})
    fake = types.ModuleType("posepipeline_amd.wrappers.mmtrack")
    fake.mmtrack_bounding_boxes = lambda file_path, method="tracktor": tracks
    monkeypatch.setitem(sys.modules, "posepipeline_amd.wrappers.mmtrack", fake)
    monkeypatch.setattr(W, "mmtrack", fake, raising=False)


def _row(track_id, x=1.0):
    return {"track_id": track_id, "tlbr": np.array([x, 2, x + 10, 22]), "tlhw": np.array([x, 2, 10, 20]), "confidence": 0.9}


def _stub_vibe(calls, n=9):
    def process_vibe(key):
        calls.append(dict(key))
        key.update(cams=np.zeros((n, 4)), verts=np.zeros((n, 6890, 3), np.float32), poses=np.zeros((n, 72), np.float32),
                   betas=np.zeros((n, 10), np.float32), joints3d=np.zeros((n, 49, 3), np.float32), joints2d=np.zeros((n, 49, 2), np.float32))
        return key
    return process_vibe


def test_make_dispatch_with_stub_wrapper(monkeypatch, tmp_path):
    from posepipeline_amd.utils import standard_pipelines as sp
    from posepipeline_amd.wrappers import vibe as wv
    calls = []
    monkeypatch.setattr(wv, "process_vibe", _stub_vibe(calls))
    vkey = {"video_project": "p", "filename": "m"}
    _video_with_tracks(tmp_path, monkeypatch, vkey, [[_row(3)]] * 9)
    person = sp.tracking_pipeline(vkey, tracking_method_name="MMTrack_deepsort")[0]
    key0 = {**person, "smpl_method": 0}
    pl.SMPLMethod.insert1(key0)
    pl.SMPLPerson.populate(key0)
    assert len(calls) == 1 and calls[0]["smpl_method"] == 0
    row = (pl.SMPLPerson & key0).fetch1()                      # a stub that returns `verts` still inserts: the column does not exist
    assert row["model_type"] == "SMPL" and "verts" not in row and row["joints3d"].shape == (9, 49, 3)
    for method in range(1, 8):
        key = {**person, "smpl_method": method}
        pl.SMPLMethod.insert1(key)
        name = (pl.SMPLMethodLookup & key).fetch1("smpl_method_name")
        with pytest.raises(Exception, match=f"Method {name} not implemented"):
            pl.SMPLPerson.populate(key)
        (pl.SMPLMethod & key).delete()
    assert len(calls) == 1 and len(pl.SMPLPerson()) == 1


def test_smpl_pipeline_recipe_with_stub_wrappers(monkeypatch, tmp_path):
    from posepipeline_amd.utils import standard_pipelines as sp
    from pose_pipeline.utils.standard_pipelines import smpl_pipeline
    from posepipeline_amd.wrappers import vibe as wv
    assert smpl_pipeline is sp.smpl_pipeline
    sig = inspect.signature(sp.smpl_pipeline).parameters
    assert [(n, p.default) for n, p in sig.items()][1:] == [("tracking_method_name", "DeepSortYOLOv4"), ("smpl_method_name", "PIXIE"),
                                                            ("reserve_jobs", False)]
    calls = []
    monkeypatch.setattr(wv, "process_vibe", _stub_vibe(calls))
    vkey = {"video_project": "p", "filename": "s"}
    _video_with_tracks(tmp_path, monkeypatch, vkey, [[_row(3)]] * 9)
    with pytest.raises(Exception, match="Method PIXIE not implemented"):
        sp.smpl_pipeline(vkey, tracking_method_name="MMTrack_deepsort")               # the default, as the reference's
    (pl.SMPLMethod & {**vkey, "smpl_method": 5}).delete()                              # the row that call registered
    keys = sp.smpl_pipeline(vkey, tracking_method_name="MMTrack_deepsort", smpl_method_name="VIBE")
    assert isinstance(keys, list) and len(keys) == 1 and keys[0]["smpl_method"] == 0 and keys[0]["video_subject_id"] == 0
    assert len(pl.SMPLPerson & keys[0]) == 1 and len(calls) == 1
    again = sp.smpl_pipeline(vkey, tracking_method_name="MMTrack_deepsort", smpl_method_name="VIBE")
    assert again == keys and len(calls) == 1                                           # a second call computes nothing
    with pytest.raises(Exception, match="fetch1"):
        sp.smpl_pipeline(vkey, tracking_method_name="MMTrack_deepsort", smpl_method_name="NoSuchMethod")
    # two identities: no automatic annotation, the recipe waits
    vkey2 = {"video_project": "p", "filename": "t"}
    _video_with_tracks(tmp_path, monkeypatch, vkey2, [[_row(3), _row(4, 30.0)]] * 9)
    assert sp.smpl_pipeline(vkey2, tracking_method_name="MMTrack_deepsort", smpl_method_name="VIBE") is False
    assert len(pl.SMPLMethod & vkey2) == 0 and len(calls) == 1


# ---- box helpers: hand-computed float64 values ---------------------------------------------------------------------------------------------
def test_fix_bb_aspect_ratio():
    # wide: 40 x 20 at (10, 20), centre (30, 30) -> the height grows to 40
    assert np.array_equal(BB.fix_bb_aspect_ratio(np.array([10.0, 20, 40, 20]), dilate=1.0, ratio=1.0), [10, 10, 40, 40])
    # tall: 20 x 40 at (10, 20), centre (20, 40) -> the width grows to 40
    assert np.array_equal(BB.fix_bb_aspect_ratio(np.array([10.0, 20, 20, 40]), dilate=1.0, ratio=1.0), [0, 20, 40, 40])
    # square: unchanged
    assert np.array_equal(BB.fix_bb_aspect_ratio(np.array([4.0, 6, 10, 10]), dilate=1.0, ratio=1.0), [4, 6, 10, 10])
    # the default dilation 1.2 about the centre: 40 -> 48
    assert np.allclose(BB.fix_bb_aspect_ratio(np.array([10.0, 20, 40, 20])), [6, 6, 48, 48], rtol=0, atol=1e-12)
    # another ratio (288 / 384): 10 x 40 at the origin, centre (5, 20) -> 30 x 40
    assert np.array_equal(BB.fix_bb_aspect_ratio(np.array([0.0, 0, 10, 40]), dilate=1.0, ratio=0.75), [-10, 0, 30, 40])
    assert [p.default for p in inspect.signature(BB.fix_bb_aspect_ratio).parameters.values()][1:] == [1.2, 1.0]


def test_convert_crop_helpers():
    from pose_pipeline.utils.bounding_box import convert_crop_cam_to_orig_img
    assert convert_crop_cam_to_orig_img is BB.convert_crop_cam_to_orig_img
    bbox = np.array([[100.0, 50, 200, 200]])
    # cx = 200, cy = 150, side 200 in a 640 x 480 image: sx = .8 / 3.2, sy = .8 / 2.4, tx = -.375 / sx + .1, ty = -.375 / sy - .2
    cam = BB.convert_crop_cam_to_orig_img(np.array([[0.8, 0.1, -0.2]]), bbox, 640, 480)
    assert cam.shape == (1, 4) and cam.dtype == np.float64
    assert np.allclose(cam, [[0.25, 1.0 / 3.0, -1.4, -1.325]], rtol=0, atol=1e-14)
    kp = np.array([[[-1.0, -1], [0, 0], [1, 1], [0.5, -0.5]]])
    got = BB.convert_crop_coords_to_orig_img(bbox, kp.copy(), 224)
    assert np.allclose(got, [[[100, 50], [200, 150], [300, 250], [250, 100]]], rtol=0, atol=1e-12)
    # the kept quirk: the side is the box WIDTH (column 2), also for a box that is not square
    got = BB.convert_crop_coords_to_orig_img(np.array([[100.0, 50, 200, 100]]), kp.copy(), 224)
    assert np.allclose(got[0, 0], [100, 0], rtol=0, atol=1e-12) and np.allclose(got[0, 2], [300, 200], rtol=0, atol=1e-12)
    # float32 joints stay float32, as in the reference's in-place arithmetic
    assert BB.convert_crop_coords_to_orig_img(bbox, kp.astype(np.float32), 224).dtype == np.float32


def test_crop_matrices_use_the_squared_box():
    from posepipeline_amd.wrappers import vibe as wv
    from oracle import preprocess as opre
    boxes = np.array([[10.0, 20, 40, 20], [3.25, 7.5, 20, 41]])
    sq, mats = wv.crop_matrices(boxes)
    assert np.array_equal(sq[0], [10, 10, 40, 40]) and sq.dtype == np.float64 and mats.shape == (2, 2, 3)
    # the three corners land on (0, 0), (224, 224), (0, 224)
    for b, m in zip(sq, mats):
        corners = np.array([[b[0], b[1], 1], [b[0] + b[2], b[1] + b[3], 1], [b[0], b[1] + b[3], 1]])
        assert np.allclose(corners @ m.T, [[0, 0], [224, 224], [0, 224]], atol=1e-4)
        src = np.float32([[b[0], b[1]], [b[0] + b[2], b[1] + b[3]], [b[0], b[1] + b[3]]])
        assert np.array_equal(m, opre.get_affine_transform_cv(src, np.float32([[0, 0], [224, 224], [0, 224]])))


# ---- body model and references -----------------------------------------------------------------------------------------------------------
def _random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def test_rot6d_gives_rotations():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 144))
    r = R.rot6d_np(x)
    assert r.shape == (50 * 24, 3, 3)
    assert np.abs(r @ np.transpose(r, (0, 2, 1)) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(r) - 1).max() < 1e-12
    # the identity in 6-D form, and the torch twin
    assert np.array_equal(R.rot6d_np(np.tile([1.0, 0, 0, 1, 0, 0], 24)), np.tile(np.eye(3), (24, 1, 1)))
    import torch
    assert np.abs(R._t_rot6d(torch.from_numpy(x)).numpy() - r).max() < 1e-12


def test_axis_angle_reference_reconstructs_every_branch():
    rng = np.random.default_rng(1)
    rot = _random_rotations(rng, 400)
    # rotations by nearly pi about each axis and the identity reach the other quaternion branches and sin^2 = 0
    for axis in range(3):
        v = np.zeros(3)
        v[axis] = np.pi - 1e-3
        rot = np.concatenate([rot, R.rodrigues_np(v[None])])
    rot = np.concatenate([rot, np.eye(3)[None]])
    aa = R.rotmat_to_aa_np(rot)
    assert np.abs(R.rodrigues_np(aa) - rot).max() < 1e-9
    assert np.linalg.norm(aa, axis=1).max() <= np.pi + 1e-12 and not aa[-1].any()
    import torch
    assert np.abs(R._t_aa(torch.from_numpy(rot)).numpy() - aa).max() < 1e-12


def test_synth_body_model_invariants():
    for n_verts in (37, 6890):
        body = S.synth_body_model(5, n_verts)
        assert {k: v.shape for k, v in body.items()} == {k: shp(n_verts) for k, shp in S.ARRAYS.items()}
        assert all(v.dtype == np.float32 for v in body.values())
        for k, nnz in (("J_regressor", 32), ("J_regressor_extra", 32), ("weights", 4)):
            a = body[k]
            assert (a >= 0).all() and np.abs(a.astype(np.float64).sum(axis=1) - 1).max() < 1e-6, k
            assert ((a > 0).sum(axis=1) == min(nnz, a.shape[1])).all(), k
        assert np.abs(body["v_template"]).max() <= 0.5 and 5e-3 < body["shapedirs"].std() < 2e-2 and 5e-4 < body["posedirs"].std() < 2e-3
        assert S.check_body_model(body)["posedirs"].shape == (207, 3 * n_verts)
    assert np.array_equal(S.synth_body_model(5, 37)["weights"], S.synth_body_model(5, 37)["weights"])
    with pytest.raises(ValueError, match="posedirs"):
        S.check_body_model({**S.synth_body_model(5, 37), "posedirs": np.zeros((207, 3))})
    assert S.vertex_ids(6890).tolist() == list(S.VERTEX_IDS_SMPLH) and S.vertex_ids(37).max() < 37


def test_smpl_reference_at_rest():
    body = S.synth_body_model(2, 37)
    ids, jm = S.vertex_ids(37), S.JOINT_MAP_54
    eye = np.tile(np.eye(3), (2, 24, 1, 1))
    # float32 skinning weights sum to 1 only to float32 rounding: renormalised in float64, the rest pose returns the template exactly
    b64 = R.as_dtype(body, np.float64)
    b64["weights"] = b64["weights"] / b64["weights"].sum(axis=1, keepdims=True)
    verts, j49, chain = R.smpl_np(b64, np.zeros((2, 10)), eye, ids, jm)
    assert np.abs(verts - b64["v_template"]).max() < 1e-14
    # with the float32 weights as they are, the deviation is the weights' rounding: 4 weights x 2^-25 x |v| <= 0.5
    assert np.abs(R.smpl_np(body, np.zeros((2, 10)), eye, ids, jm)[0] - b64["v_template"]).max() < 4 * 2.0 ** -25 * 0.5
    assert np.abs(chain - b64["J_regressor"] @ b64["v_template"]).max() < 1e-14
    assert np.abs(j49[:, 8] - chain[:, 0]).max() == 0                                   # OP MidHip is chain joint 0
    # the torch twin agrees with the numpy code on a posed body
    rng = np.random.default_rng(3)
    rot, betas, cam = _random_rotations(rng, 48).reshape(2, 24, 3, 3), rng.standard_normal((2, 10)), np.array([[0.9, 0.1, -0.1], [1.1, 0, 0.2]])
    import torch
    t = R.torch_smpl(body, betas, rot, cam, ids, jm, torch.float64)
    verts, j49, _ = R.smpl_np(body, betas, rot, ids, jm)
    assert np.abs(t["verts"] - verts).max() < 1e-12 and np.abs(t["joints3d"] - j49).max() < 1e-12
    assert np.abs(t["kp2d"] - R.project_np(j49, cam)).max() < 1e-12
    assert np.abs(t["pose_aa"] - R.rotmat_to_aa_np(rot).reshape(2, 72)).max() < 1e-12


def test_head_references_agree_and_program_shapes():
    import torch
    sd = VM.synth_params(VM.vibe_param_shapes(), seed=4)
    assert sum(int(np.prod(s)) for s in VM.vibe_param_shapes().values()) == 9437184 + 6291456 + 4 * 3072 + 2099200 + 2258944 + 1049600 + 160925 + 157
    body = S.synth_body_model(2, 37)
    feats = np.random.default_rng(6).standard_normal((5, 2048)).astype(np.float32)
    a = R.head_np(feats, sd, body, S.vertex_ids(37), S.JOINT_MAP_54, seq=3)              # two sequences: 3 + 2
    b = R.torch_head(feats, sd, body, S.vertex_ids(37), S.JOINT_MAP_54, torch.float64, seq=3)
    for k in ("cam", "betas", "joints3d", "kp2d", "verts", "pose_aa"):
        assert np.abs(a[k] - b[k]).max() < 1e-9, k
    # sequences do not see each other's state: the second sequence alone gives its rows (to float64 rounding: the matrix products
    # over 2 and over 5 rows may add in another order)
    alone = R.head_np(feats[3:], sd, body, S.vertex_ids(37), S.JOINT_MAP_54, seq=3)
    assert np.abs(alone["joints3d"] - a["joints3d"][3:]).max() < 1e-12
    carried = R.head_np(feats, sd, body, S.vertex_ids(37), S.JOINT_MAP_54, seq=5)         # one sequence of 5: the state carries over
    assert np.abs(carried["joints3d"][3:] - a["joints3d"][3:]).max() > 1e-6
    prog = VM.build_head_program(sd)
    assert {n: prog.bufs[i] for n, i in prog.named.items()} == {"h": (1, 1, 1024), "features": (1, 1, 2048), "init_pose": (1, 1, 144),
                                                               "init_shape": (1, 1, 12), "init_cam": (1, 1, 4), "pose6d": (1, 1, 144),
                                                               "shape": (1, 1, 12), "cam": (1, 1, 4)}
    w = VM.fc1_permuted(sd["regressor.fc1.weight"])
    assert w.shape == (1024, 2208) and not w[:, 2202:2204].any() and not w[:, 2207].any()
    assert np.array_equal(w[:, 2204:2207], sd["regressor.fc1.weight"][:, 2202:]) and np.array_equal(w[:, 2192:2202], sd["regressor.fc1.weight"][:, 2192:2202])
    with pytest.raises(KeyError, match="encoder.linear.bias"):
        VM.build_head_program({k: v for k, v in sd.items() if k != "encoder.linear.bias"})


def test_checkpoint_key_candidates(tmp_path):
    import torch
    from posepipeline_amd import weights
    for key in ("model", "gen_state_dict"):
        path = str(tmp_path / f"{key}.pth.tar")
        torch.save({key: {"a.weight": torch.ones(2, 3)}, "epoch": 3}, path)
        sd = weights.load_state_dict(path)
        assert list(sd) == ["a.weight"] and sd["a.weight"].shape == (2, 3)
