"""GAST-Net lifting without a device: the parameter inventory and the graphs, the two references against each other, chunked against
per-window evaluation, the host side of the wrapper (score conversion, revise_kpts, valid-frame compaction, coco_h36m against the
PoseFormer golden file, flip symmetry, camera_to_world) and the dispatch of LiftingPerson.make."""
import datetime
import os

import numpy as np
import pytest
import torch

from posepipeline_amd.models import gastnet as M
from posepipeline_amd.wrappers import gastnet as W
from tests import gastnet_ref as R

SMALL = M.GastNetSpec(channels=16, filter_widths=(3, 3, 3), chunk=8)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseformer_pre.npz")


@pytest.fixture(scope="module")
def sd():
    return M.synth_params(M.gastnet_param_shapes(SMALL), seed=3)


def _forward64(sd, spec):
    sd64 = R.as_dtype(sd, np.float64)
    return lambda b: R.forward_np(b.transpose(0, 2, 1, 3).astype(np.float64), sd64, spec.filter_widths, spec.heads).transpose(0, 2, 1, 3)


def test_param_shapes():
    for spec, rf, widest in ((M.GastNetSpec(), 27, 1024), (M.GastNetSpec(filter_widths=(3, 3, 3, 3), channels=64), 81, 1024)):
        shapes = M.gastnet_param_shapes(spec)
        assert spec.receptive_field == rf and spec.pad == (rf - 1) // 2
        model = R.SpatioTemporalModel(spec.filter_widths, spec.channels, spec.heads)
        want = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")}
        assert {k: tuple(v) for k, v in shapes.items()} == want
        assert shapes["shrink.weight"] == (3, widest, 1, 1)
        assert shapes["expand_conv.weight"] == (spec.channels, 2, 3, 1) and shapes["init_bn.weight"] == (2,)
    s = M.gastnet_param_shapes(M.GastNetSpec())
    assert s["layers_graph_conv.2.cat_conv.weight"] == (1024, 1536, 1, 1)
    assert s["layers_graph_conv.0.local_graph_layer.gcn_sym.W"] == (2, 128, 128)
    assert s["layers_graph_conv.0.local_graph_layer.gcn_sym.e"] == (128, 29)
    assert s["layers_graph_conv.1.global_graph_layer.theta.3.weight"] == (64, 256, 1, 1)
    assert s["layers_conv.3.weight"] == (512, 512, 1, 1) and s["layers_conv.2.weight"] == (512, 512, 3, 1)


def test_masks():
    m, r = M.graph_masks(), R.masks()
    assert int(m["sym"].sum()) == 29 and np.array_equal(m["sym"], m["sym"].T)
    assert np.array_equal(m["sym"], r["sym"]) and np.array_equal(m["con"], r["con"])
    adj = M.skeleton_adjacency()
    assert np.allclose(adj.sum(1), 1) and int((adj > 0).sum()) == 17 + 2 * 16
    for j in range(17):
        want = (adj @ adj)[j] > 0 if j in M.H36M_DISTAL else adj[j] > 0
        assert np.array_equal(m["con"][j], want), j
    assert m["con"].diagonal().all()


def test_build_errors(sd):
    bad = dict(sd)
    del bad["init_bn.weight"]
    with pytest.raises(KeyError, match="init_bn.weight"):
        M.checked_state_dict(SMALL, bad)
    bad = dict(sd)
    bad["shrink.weight"] = np.zeros((3, 64, 1, 1), np.float32)
    with pytest.raises(ValueError, match="shrink.weight"):
        M.checked_state_dict(SMALL, bad)
    bad = dict(sd)
    k = "layers_graph_conv.1.local_graph_layer.gcn_con.e"
    nnz = int(M.graph_masks()["con"].sum())
    bad[k] = np.zeros((32, nnz + 4), np.float32)
    with pytest.raises(ValueError, match=f"{nnz + 4} edges.*con mask.*{nnz}"):
        M.checked_state_dict(SMALL, bad)
    with pytest.raises(ValueError, match="multiple of 16"):
        M.build_gastnet_program(M.GastNetSpec(channels=24), sd)


def test_graph_matrices_fold():
    """the folded matrix times (h0 on the diagonal, h1 off it) + bias == BatchNorm(SemCHGraphConv), in float64 up to the one rounding"""
    rng = np.random.default_rng(0)
    d, mask = 8, M.graph_masks()["con"]
    e, bias = rng.standard_normal((d, int(mask.sum()))), rng.standard_normal(d)
    bn = (rng.uniform(0.5, 2, d), rng.standard_normal(d), rng.standard_normal(d), rng.uniform(0.5, 2, d))
    w = rng.standard_normal((2, d, d))
    x = rng.standard_normal((1, 2, 17, d))
    a, b = M.graph_matrices(e, mask, bias, bn)
    assert a.shape == (17, 17, d) and a.dtype == np.float32 and not a[~mask].any() and (a[mask] != 0).all()
    h0, h1 = x @ w[0], x @ w[1]
    eye = np.eye(17)[:, :, None]
    got = np.einsum("jic,btic->btjc", a * eye, h0) + np.einsum("jic,btic->btjc", a * (1 - eye), h1) + b
    sdl = {"bn.weight": bn[0], "bn.bias": bn[1], "bn.running_mean": bn[2], "bn.running_var": bn[3]}
    want = R._bn(R.sem_ch_graph_conv(x, w, e, bias, mask), sdl, "bn")
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


def test_references_agree(sd):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (2, 30, 17, 2))
    sd64 = R.as_dtype(sd, np.float64)
    a = R.forward_np(x, sd64, SMALL.filter_widths)
    b = R.torch_forward(x, sd64, SMALL.filter_widths, SMALL.channels, torch.float64)
    assert a.shape == b.shape == (2, 4, 17, 3) and a.dtype == b.dtype == np.float64
    assert 0.01 < np.abs(a).max() < 100, np.abs(a).max()          # the synthetic weights give outputs of order one
    assert np.abs(a - b).max() <= 1e-10, np.abs(a - b).max()


def test_chunked_equals_per_window(sd):
    """the lifter's chunk loop (edge padding, halos, one full chunk and a ragged one of 3) == one receptive field per output frame"""
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (11, 17, 2)).astype(np.float32)
    sd64 = R.as_dtype(sd, np.float64)
    calls = []

    def forward(b):
        calls.append(b.shape)
        return _forward64(sd, SMALL)(b)
    got = W.lift_chunks(forward, x, SMALL, flip_augment=False)
    assert calls == [(1, 17, 8 + 26, 2)] * 2 and got.shape == (11, 17, 3) and got.dtype == np.float32
    xp = np.pad(x, ((13, 13), (0, 0), (0, 0)), mode="edge").astype(np.float64)
    want = R.forward_windows_np(xp, sd64, SMALL.filter_widths)
    assert want.shape == (11, 17, 3)
    chunked64 = np.concatenate([R.forward_np(xp[None, s:s + min(8, 11 - s) + 26], sd64, SMALL.filter_widths)[0] for s in (0, 8)])
    assert np.abs(chunked64 - want).max() <= 1e-12
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()      # (lift_chunks rounds its result to float32)


def test_flip_augmentation_is_symmetric(sd):
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, (11, 17, 2)).astype(np.float32)
    fwd = _forward64(sd, SMALL)
    a = W.lift_chunks(fwd, x, SMALL, flip_augment=True)
    b = W.lift_chunks(fwd, W.mirror_input(x), SMALL, flip_augment=True)
    assert np.array_equal(b, W.mirror_output(a))
    plain = W.lift_chunks(fwd, x, SMALL, flip_augment=False)
    assert not np.array_equal(a, plain)
    assert np.array_equal(W.mirror_input(W.mirror_input(x)), x)
    m = W.mirror_input(x)
    assert np.array_equal(m[:, 4], x[:, 1] * (-1, 1)) and np.array_equal(m[:, 14], x[:, 11] * (-1, 1)) and np.array_equal(m[:, 0], x[:, 0] * (-1, 1))


def _frame(scores):
    kp = np.arange(34, dtype=np.float32).reshape(1, 17, 2) + 1
    return kp, np.asarray(scores, np.float32)[None]


@pytest.mark.parametrize("low,dst,src", [((2, 3, 5, 6), [2, 3, 5, 6], [1, 1, 4, 4]), ((2, 3, 6), [2, 3, 6], [1, 1, 5]),
                                         ((3, 5, 6), [3, 5, 6], [2, 4, 4]), ((3, 6), [3, 6], [2, 5]), ((3,), [3], [2]), ((6,), [6], [5]),
                                         ((2,), [], []), ((2, 5), [], []), ((), [], [])])
def test_revise_kpts(low, dst, src):
    s = np.full(17, 0.9, np.float32)
    s[list(low)] = 0.2
    s[9] = 0.1                                   # a low score elsewhere changes nothing
    kp, sc = _frame(s)
    two = np.concatenate([kp, kp]), np.concatenate([sc, sc])
    out = W.revise_kpts(two[0], two[1], [1])
    assert np.array_equal(out[0], kp[0])         # frame 0 is not a valid frame: untouched
    want = kp[0].copy()
    want[dst] = kp[0][src]
    assert np.array_equal(out[1], want) and out is not two[0]
    s[list(low)] = 0.3                           # the threshold is strict
    assert np.array_equal(W.revise_kpts(kp, s[None], [0]), kp)


def test_score_conversion_and_valid_frames():
    rng = np.random.default_rng(6)
    kp = rng.uniform(10, 400, (5, 17, 2)).astype(np.float32)
    sc = rng.uniform(0, 1, (5, 17)).astype(np.float32)
    kp[2] = 0                                    # no detection in the middle of the clip
    out, s, valid = W.h36m_coco_format(kp, sc)
    assert out.dtype == np.float32 and s.dtype == np.float32 and valid.tolist() == [0, 1, 3, 4]
    assert not out[2].any() and np.array_equal(out, W.coco_h36m(kp))
    for h, c in {9: 0, 1: 12, 2: 14, 3: 16, 4: 11, 5: 13, 6: 15, 11: 5, 12: 7, 13: 9, 14: 6, 15: 8, 16: 10}.items():
        assert np.array_equal(s[:, h], sc[:, c]), h
    assert np.allclose(s[:, 0], sc[:, [11, 12]].mean(1), rtol=1e-6) and np.allclose(s[:, 8], sc[:, [5, 6]].mean(1), rtol=1e-6)
    assert np.allclose(s[:, 7], (s[:, 0] + s[:, 8]) / 2, rtol=1e-6) and np.allclose(s[:, 10], sc[:, 1:5].mean(1), rtol=1e-6)
    # a clip without any detection: nothing is valid, everything stays zero
    out0, s0, valid0 = W.h36m_coco_format(np.zeros((3, 17, 2), np.float32), np.ones((3, 17), np.float32))
    assert not out0.any() and not s0.any() and valid0.size == 0
    with pytest.raises(ValueError):
        W.h36m_coco_format(np.zeros((3, 16, 2)), np.zeros((3, 16)))


def test_coco_h36m_against_the_golden_file():
    """the coordinates are poseformer.coco_h36m's, whose rounding points tests/golden/poseformer_pre.npz pins: the first window of the
    golden network input is the normalised conversion of the first 81 frames"""
    g = np.load(GOLDEN)
    for clip in ("a", "b"):
        kp, (height, width) = g[f"kp_{clip}"], g[f"hw_{clip}"]
        out, _, valid = W.h36m_coco_format(kp[..., :2], kp[..., 2])
        assert valid.tolist() == list(range(len(kp)))
        norm = (out / np.array([height, width])[None, None, :]).astype(np.float32)
        assert np.array_equal(norm[:81], g[f"windows_{clip}"][0])


def test_normalize_and_camera_to_world():
    rng = np.random.default_rng(8)
    x = rng.uniform(0, 640, (4, 17, 2)).astype(np.float32)
    n = W.normalize_screen_coordinates(x, w=640, h=480)
    assert n.dtype == np.float64 and np.allclose(n[..., 0], x[..., 0] / 320 - 1) and np.allclose(n[..., 1], x[..., 1] / 320 - 0.75)
    v = rng.standard_normal((4, 17, 3)).astype(np.float32)
    q = W.CAMERA_QUATERNION.astype(np.float64)
    assert abs(np.linalg.norm(q) - 1) < 1e-6
    w_, x_, y_, z_ = q
    rot = np.array([[1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - z_ * w_), 2 * (x_ * z_ + y_ * w_)],
                    [2 * (x_ * y_ + z_ * w_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ - x_ * w_)],
                    [2 * (x_ * z_ - y_ * w_), 2 * (y_ * z_ + x_ * w_), 1 - 2 * (x_ * x_ + y_ * y_)]])
    got = W.camera_to_world(v)
    assert got.dtype == np.float32 and got.shape == v.shape
    assert np.abs(got - v.astype(np.float64) @ rot.T).max() <= 2e-6 * np.abs(v).max()


class _Recorder:
    def __init__(self):
        self.inputs = []

    def lift(self, x):
        self.inputs.append(np.array(x))
        return np.broadcast_to(np.arange(len(x), dtype=np.float32)[:, None, None] + 1, (len(x), 17, 3)).copy()


def _tables(kp, height=480, width=640, name="g"):
    from posepipeline_amd import pipeline as pl
    vkey = {"video_project": "gast", "filename": name}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 10, 18)})
    pl.VideoInfo().insert1({**vkey, "timestamps": [], "delta_time": [], "fps": 30.0, "height": height, "width": width, "num_frames": len(kp)})
    key = {**vkey, "tracking_method": 5, "video_subject_id": 0, "top_down_method": 0}
    pl.TopDownPerson().insert1({**key, "keypoints": kp})
    return key


def test_wrapper_assembly(monkeypatch):
    """valid-frame compaction with an all-zero frame in the middle: the model sees the 4 valid frames, revised and normalised; its rows
    land at the valid indices, rotated; the others are zeros"""
    from posepipeline_amd import djshim
    djshim.reset()
    rng = np.random.default_rng(10)
    kp = np.empty((5, 17, 3), np.float32)
    kp[..., :2] = rng.uniform(10, 400, (5, 17, 2))
    kp[..., 2] = 0.9
    kp[2] = 0
    kp[3, 16, 2] = 0.1                           # COCO right ankle = H36M joint 3: frame 3 is revised, 3 <- 2
    key = _tables(kp)
    model = _Recorder()
    monkeypatch.setattr(W, "_model", lambda device=0: model)
    before = dict(key)
    try:
        res = W.process_gastnet(key)
    finally:
        djshim.reset()
    assert key == before and set(res) == {"keypoints_3d", "keypoints_valid"}
    assert res["keypoints_valid"] == [True, True, False, True, True] and all(type(v) is bool for v in res["keypoints_valid"])
    k3 = res["keypoints_3d"]
    assert k3.shape == (5, 17, 3) and k3.dtype == np.float64 and not k3[2].any()
    for row, f in enumerate((0, 1, 3, 4)):
        assert np.array_equal(k3[f], W.camera_to_world(np.full((17, 3), row + 1, np.float32)).astype(np.float64))
    (x,) = model.inputs
    assert x.dtype == np.float32 and x.shape == (4, 17, 2)
    h36m = W.coco_h36m(kp[..., :2])
    want = h36m[[0, 1, 3, 4]].copy()
    want[2, 3] = want[2, 2]
    assert np.array_equal(x, W.normalize_screen_coordinates(want, w=640, h=480).astype(np.float32))


def test_wrapper_argument_errors(monkeypatch):
    from posepipeline_amd import djshim
    monkeypatch.setattr(W, "_model", lambda device=0: _Recorder())
    for kp, what in ((np.zeros((4, 17, 3), np.float32), "no valid frame"), (np.ones((4, 16, 3), np.float32), "expected")):
        djshim.reset()
        key = _tables(kp)
        try:
            with pytest.raises(ValueError, match=what):
                W.process_gastnet(key)
        finally:
            djshim.reset()
    with pytest.raises(ValueError, match="17"):
        W._check_input(np.zeros((4, 16, 2), np.float32))


def test_module_path():
    import pose_pipeline.wrappers.gastnet_lifting as shim
    from pose_pipeline.wrappers.gastnet_lifting import process_gastnet
    assert shim is W and process_gastnet is W.process_gastnet


def test_lifting_person_dispatch(monkeypatch, tmp_path, sd):
    """without the checkpoint file the row is `not implemented`, naming the path; with one, make() calls process_gastnet"""
    from posepipeline_amd import djshim, pipeline as pl
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    djshim.reset()
    kp = np.ones((4, 17, 3), np.float32)
    key = {**_tables(kp), "lifting_method": 0}
    calls = []

    def fake(k):
        calls.append(dict(k))
        return {"keypoints_3d": np.zeros((4, 17, 3)), "keypoints_valid": [True] * 4}
    monkeypatch.setattr(W, "process_gastnet", fake)
    try:
        pl.LiftingMethod().insert1(key)
        with pytest.raises(Exception, match="Method not implemented.*27_frame_model.bin"):
            pl.LiftingPerson().make(dict(key))
        assert not calls and len(pl.LiftingPerson & key) == 0
        os.makedirs(tmp_path / "gastnet")
        torch.save({"model_pos": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, str(tmp_path / "gastnet" / "27_frame_model.bin"))
        assert W.checkpoint_path() == str(tmp_path / "gastnet" / "27_frame_model.bin")
        pl.LiftingPerson().make(dict(key))
        assert calls == [key] and len(pl.LiftingPerson & key) == 1
        # the file is read with the `module.` prefix dropped
        got = W.load_state_dict(SMALL)
        assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    finally:
        djshim.reset()
