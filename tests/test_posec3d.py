"""The SkeletonAction stage on the CPU: sampler, key-point transforms, parameter names, programs, tables and shims.
(The device code is held by tests/test_gpu_posec3d.py.)"""
import os

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd import djshim, pipeline as pl
from posepipeline_amd.models import posec3d as PM
from posepipeline_amd.wrappers import mmaction as W
from tests import posec3d_ref as R

TINY = PM.PoseC3DSpec(base_channels=8, stage_blocks=(1, 2, 1), clip_len=4, height=16, width=16)


@pytest.fixture(autouse=True)
def clean():
    djshim.reset()
    yield
    djshim.reset()


# ---- sampler ---------------------------------------------------------------------------------------------------------------------------
def test_frame_indices_of_the_wrapper_call():
    """total_frames 10 < clip_len 48: the simple strategy; only the first ten frames of a window are read"""
    assert W.TOTAL_FRAMES == 10 and W.CLIP_LEN == 48 and W.NUM_CLIPS == 10
    inds = W.uniform_sample_frames(10, 48, 10)
    want = np.concatenate([(i + np.arange(48)) % 10 for i in range(10)])
    assert inds.dtype == np.int64 and np.array_equal(inds, want) and inds.max() == 9
    assert np.array_equal(inds, R.sample_frames_loop(10, 48, 10))


@pytest.mark.parametrize("total,clip_len,num_clips", [(4, 6, 2), (3, 6, 5), (10, 6, 2), (60, 48, 10), (100, 48, 10), (96, 48, 3)])
def test_frame_indices_other_branches(total, clip_len, num_clips):
    """fewer frames than clips; the seeded skip branch (clip_len <= n < 2 clip_len); the seeded bucket branch"""
    inds = W.uniform_sample_frames(total, clip_len, num_clips)
    assert inds.shape == (num_clips * clip_len,) and inds.min() >= 0 and inds.max() < total
    assert np.array_equal(inds, R.sample_frames_loop(total, clip_len, num_clips))
    per_clip = inds.reshape(num_clips, clip_len)
    if total >= clip_len:
        assert (np.diff(per_clip, axis=1) > 0).all()                  # strictly increasing inside a clip
        assert np.array_equal(inds, W.uniform_sample_frames(total, clip_len, num_clips))      # seeded: the same on every call


def test_window_starts_are_the_reference_range():
    assert W.window_starts(52) == [0, 1, 2] and W.window_starts(50) == [0] and W.window_starts(49) == [] and W.window_starts(3) == []
    assert W.window_starts(60, stride=4) == [0, 4, 8]


# ---- transforms ----------------------------------------------------------------------------------------------------------------------
def _track(rng, n=48, h=480, w=640, box=(200, 120, 160, 300)):
    x0, y0, bw, bh = box
    kp = np.zeros((n, 17, 3))
    base = np.stack([rng.uniform(x0, x0 + bw, 17), rng.uniform(y0, y0 + bh, 17)], axis=1)
    for t in range(n):
        kp[t, :, :2] = base + rng.normal(0, 3, (17, 2)) + t * np.array([1.5, -0.5])
        kp[t, :, 2] = rng.uniform(0.2, 1.0, 17)
    return kp


def _tracks():
    rng = np.random.default_rng(5)
    plain = _track(rng)
    absent = _track(rng)
    absent[3] = 0.0                                                   # a frame without the person: all-zero row
    absent[7, 4] = 0.0
    border = _track(rng, box=(-20, -10, 200, 300))                    # touches (and leaves) the image at the left and top
    border[:, 0, :2] = (0.25, 479.5)
    small = _track(rng, box=(300, 200, 6, 40))                        # x extent under PoseCompact's threshold: the box is not applied
    small[:, :, 0] = 300 + rng.uniform(0, 6, (48, 17))
    wide = _track(rng, h=1080, w=1920, box=(100, 500, 900, 120))      # wider than tall: hw_ratio squares the box
    f32 = _track(rng).astype(np.float32)
    return {"plain": (plain, (480, 640)), "absent": (absent, (480, 640)), "border": (border, (480, 640)),
            "small": (small, (480, 640)), "wide": (wide, (1080, 1920)), "float32": (f32, (480, 640))}


@pytest.mark.parametrize("name", ["plain", "absent", "border", "small", "wide", "float32"])
def test_window_keypoints_equal_the_loop_twin(name):
    kp, shape = _tracks()[name]
    inds = W.uniform_sample_frames(W.TOTAL_FRAMES, 48, 10)
    frames = np.unique(inds)
    got = W.window_keypoints(kp, shape, frames)
    assert got.dtype == np.float64 and got.shape == (10, 17, 3)
    xy, score = R.pipeline_loop(kp, shape, inds)                      # the twin works on all 480 decoded frames
    slot = np.searchsorted(frames, inds)
    assert np.array_equal(got[slot][..., :2], xy)
    assert np.array_equal(got[slot][..., 2], score.astype(np.float64))
    if name == "small":                                               # no box: the frame itself is resized, 640 x 480 -> 85 x 64
        assert np.allclose(got[0, :, 0], kp[0, :, 0] * (85 / 640) - 10, atol=1e-3)
    if name == "absent":                                              # CenterCrop shifts absent points too; their score stays zero
        assert (got[3, :, 2] == 0).all() and (got[3, :, :2] == got[3, 0, :2]).all()
    if name in ("plain", "wide"):                                     # the padded square box lands inside the 64 x 64 crop
        assert got[..., :2].min() > 0 and got[..., :2].max() < 64


def test_mirror_perm_swaps_left_and_right():
    perm = W.mirror_perm()
    assert perm.tolist() == [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15] and np.array_equal(perm[perm], np.arange(17))


def test_average_clips_and_top5():
    rng = np.random.default_rng(2)
    logits = rng.normal(0, 2, (20, 81)).astype(np.float32)
    p = W.average_clips(logits)
    assert p.dtype == np.float32 and p.shape == (81,) and abs(float(p.sum()) - 1) < 1e-6
    assert np.abs(p - R.average_clips_ref(logits)).max() < 1e-7
    labels = {i: f"class_{i}" for i in range(1, 81)}
    t5 = W.top5(p, labels)
    order = np.argsort(-p)[:5]
    assert [s for _, s in t5] == [p[i] for i in order] and [n for n, _ in t5] == [labels.get(int(i), str(int(i))) for i in order]
    q = p.copy()
    q[0] = 2.0
    assert W.top5(q, labels)[0] == ("0", q[0])                        # index 0 has no AVA label (declared difference: no KeyError)


# ---- parameters and programs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [PM.PoseC3DSpec(), TINY, PM.PoseC3DSpec(num_classes=60, inflate=(0, 0, 1))])
def test_param_shapes_equal_the_torch_twin(spec):
    ours, twin = PM.posec3d_param_shapes(spec), R.param_shapes(spec)
    assert list(ours) == list(twin)
    assert ours == twin
    if spec == PM.PoseC3DSpec():
        assert ours["backbone.conv1.conv.weight"] == (32, 17, 1, 7, 7) and ours["backbone.layer2.0.conv1.conv.weight"] == (64, 128, 3, 1, 1)
        assert ours["backbone.layer1.0.conv1.conv.weight"] == (32, 32, 1, 1, 1) and ours["backbone.layer3.0.downsample.conv.weight"] == (512, 256, 1, 1, 1)
        assert ours["cls_head.fc_cls.weight"] == (81, 512) and "backbone.layer2.0.downsample.bn.running_var" in ours


@pytest.mark.parametrize("spec", [PM.PoseC3DSpec(), TINY])
def test_programs_use_only_existing_op_types(spec):
    progs, steps = PM.build_programs(spec, PM.synth_params(PM.posec3d_param_shapes(spec), 1))
    allowed = {L.PP_OP_CONV, L.PP_OP_MAXPOOL, L.PP_OP_AVGPOOL, L.PP_OP_COPY}
    for name, prog in progs.items():
        assert {op.type for op in prog.ops} <= allowed, name
    # the clip program: one 3x1x1 convolution per inflated block, then the temporal average and fc_cls
    clip = progs["clip"]
    temporal = [op for op in clip.ops if op.type == L.PP_OP_CONV and (op.kh, op.kw) == (3, 1)]
    n_inflated = sum(b for b, i in zip(spec.stage_blocks, spec.inflate) if i)
    assert len(temporal) == n_inflated and all((op.pad_h, op.pad_w, op.stride) == (1, 0, 1) for op in temporal)
    assert len(clip.ops) == n_inflated + 2
    assert all((op.kh, op.kw) != (3, 1) for p in ("front", "frame") for op in progs[p].ops)
    # every op of the two later programs is run exactly once, in order; a view change goes both ways for every inflated block
    for name in ("frame", "clip"):
        ranges = [(s[2], s[3]) for s in steps if s[0] == "run" and s[1] == name]
        assert ranges[0][0] == 0 and ranges[-1][1] == len(progs[name].ops) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    copies = [s for s in steps if s[0] == "copy"]
    assert len(copies) == 2 * n_inflated + 1
    for _, (dn, db), (sn, sb), floats in copies:                      # the same bytes per clip on both sides
        dh, dw, dc = progs[dn].bufs[progs[dn].named[db]]
        sh, sw, sc = progs[sn].bufs[progs[sn].named[sb]]
        per = {"frame": spec.clip_len, "clip": 1}
        assert dh * dw * dc * per[dn] == sh * sw * sc * per[sn] == floats and dc == sc
    assert progs["front"].bufs[progs["front"].named["input"]] == (spec.height, spec.width, 20)
    assert progs["clip"].bufs[progs["clip"].named["logits"]] == (1, 1, 84)


def test_temporal_strides_subsample_frames():
    """(1, 1, 2): layer3.0's conv2 and projection see every second frame; the clip view and the head follow with T / 2"""
    spec = PM.replace(TINY, temporal_strides=(1, 1, 2))
    assert PM.posec3d_param_shapes(spec) == PM.posec3d_param_shapes(TINY) == R.param_shapes(spec)      # weight shapes do not reveal it
    progs, steps = PM.build_programs(spec, PM.synth_params(PM.posec3d_param_shapes(spec), 1))
    subs = [s for s in steps if s[0] == "subsample"]
    assert [(s[1][1], s[2][1], s[3], s[4]) for s in subs] == [("ys2", "t2a", 4, 2), ("xs2", "x1_1", 4, 2)]
    per = [s[4] for s in steps if s[0] == "run" and s[1] == "frame"]
    assert per == [4, 4, 2, 2]                                        # layer2.0, layer2.1, layer3.0, the head's spatial average
    assert progs["clip"].bufs[progs["clip"].named["cpool"]] == (2, 1, 128)
    assert {op.type for p in progs.values() for op in p.ops} <= {L.PP_OP_CONV, L.PP_OP_MAXPOOL, L.PP_OP_AVGPOOL}
    with pytest.raises(AssertionError):                               # a stride in a front stage would change which frames exist
        PM.build_programs(PM.replace(TINY, temporal_strides=(2, 1, 1)), PM.synth_params(PM.posec3d_param_shapes(TINY), 1))
    assert PM.PoseC3DSpec().temporal_strides == (1, 1, 1)


def test_flops_and_pass_size_come_from_the_spec():
    spec = PM.PoseC3DSpec()
    progs, _ = PM.build_programs(spec, PM.synth_params(PM.posec3d_param_shapes(spec), 1))
    macs = ((progs["front"].flops + progs["frame"].flops) * 48 + progs["clip"].flops) / 2
    assert 15e9 < macs < 30e9                                         # "about 22 GMAC per clip"
    per_clip = PM.activation_bytes_per_clip(spec, progs)
    n = PM.clips_per_pass(spec, 20, progs)
    assert 1 <= n <= 20 and n * per_clip <= PM.PASS_BUDGET_BYTES and (n == 20 or (n + 1) * per_clip > PM.PASS_BUDGET_BYTES)
    assert n == 4 and 256 << 20 < n * per_clip < 1 << 30            # hundreds of MB
    assert PM.clips_per_pass(spec, 20, progs, budget_bytes=1) == 1
    small = PM.activation_bytes_per_clip(TINY)
    assert small < per_clip / 100


# ---- the wrapper and the tables --------------------------------------------------------------------------------------------------------
class _StubModel:
    clip_len = 48

    def __init__(self):
        self.calls = []

    def scores(self, keypoints, img_shape, stride=1):
        self.calls.append((np.asarray(keypoints).shape, tuple(img_shape), stride))
        n = len(W.window_starts(np.asarray(keypoints).shape[0], 48, stride))
        rng = np.random.default_rng(n)
        p = rng.uniform(0, 1, (n, 81)).astype(np.float32)
        return p / p.sum(axis=1, keepdims=True) if n else p


def _person(n_frames):
    key = {a: 1 for a in pl.TopDownPerson.primary_key}
    key.update(video_project="p", filename=f"v{n_frames}")
    vkey = {a: key[a] for a in pl.VideoInfo.primary_key}
    pl.VideoInfo.insert1({**vkey, "timestamps": [], "delta_time": [], "num_frames": n_frames, "fps": 30.0, "height": 480, "width": 640})
    pl.TopDownPerson.insert1({**key, "keypoints": np.zeros((n_frames, 17, 3), np.float32)})
    return key


def _stub(monkeypatch):
    stub = _StubModel()
    labels = {i: f"class_{i}" for i in range(1, 81)}
    monkeypatch.setattr(W, "_model", lambda device=0: (stub, labels))
    return stub, labels


@pytest.mark.parametrize("n_frames,n_windows", [(52, 3), (50, 1)])
def test_wrapper_keys_and_shapes(monkeypatch, n_frames, n_windows):
    stub, labels = _stub(monkeypatch)
    key = _person(n_frames)
    out = W.mmaction_skeleton_action_person(dict(key), stride=1)
    assert set(out) - set(key) == {"top5", "action_scores", "label_map", "action_window_len", "stride"}
    assert stub.calls == [((n_frames, 17, 3), (480, 640), 1)]
    assert out["action_scores"].shape == (n_windows, 81) and out["action_scores"].dtype == np.float32
    assert len(out["top5"]) == n_windows and all(len(t) == 5 for t in out["top5"])
    for t, row in zip(out["top5"], out["action_scores"]):
        assert [s for _, s in t] == sorted(row, reverse=True)[:5]
    assert out["label_map"] == labels and out["action_window_len"] == 48 and out["stride"] == 1


@pytest.mark.parametrize("n_frames", [49, 48, 10, 1])
def test_zero_windows_return_what_the_reference_code_returns(monkeypatch, n_frames):
    """the reference's loop body never runs: top5 = [], action_scores = np.array([]) -- shape (0,), float64"""
    _stub(monkeypatch)
    out = W.mmaction_skeleton_action_person(_person(n_frames))
    assert out["top5"] == [] and out["action_scores"].shape == (0,) and out["action_scores"].dtype == np.float64
    assert out["action_window_len"] == 48 and out["stride"] == 1


def test_device_argument():
    assert W._device_index("cuda") == 0 and W._device_index("cuda:3") == 3 and W._device_index(2) == 2
    with pytest.raises(ValueError, match="only GPUs"):
        W._device_index("cpu")


def test_skeleton_action_make_stores_the_columns(monkeypatch):
    calls = []

    def fake(key, device="cuda", stride=1):
        calls.append((dict(key), stride))
        key.update(top5=[[("class_3", 0.5)] * 5] * 3, action_scores=np.full((3, 81), 1 / 81, np.float32), label_map={1: "class_1"},
                   action_window_len=48, stride=stride)
        return key
    monkeypatch.setattr(W, "mmaction_skeleton_action_person", fake)
    key = _person(52)
    assert pl.SkeletonAction.primary_key == pl.TopDownPerson.primary_key + ["method"]
    assert pl.SkeletonAction.heading[-6:] == ["top5", "action_scores", "label_map", "action_window_len", "stride", "computed_timestamp"]
    pl.SkeletonAction.populate(key)
    assert len(calls) == 1 and calls[0][1] == 1 and calls[0][0] == key
    row = (pl.SkeletonAction & key).fetch1()
    assert row["method"] == "mmaction_skeleton" and row["action_window_len"] == 48 and row["stride"] == 1
    assert row["action_scores"].shape == (3, 81) and len(row["top5"]) == 3 and row["label_map"] == {1: "class_1"}
    pl.SkeletonAction.populate(key)                                    # a second call computes nothing
    assert len(calls) == 1 and len(pl.SkeletonAction()) == 1


def test_shims_and_exports():
    import pose_pipeline
    import pose_pipeline.pipeline as ref_pl
    import pose_pipeline.wrappers.mmaction as shim
    import posepipeline_amd.wrappers.mmaction as ours
    assert shim is ours and hasattr(shim, "mmaction_skeleton_action_person")
    assert "SkeletonAction" in pose_pipeline.__all__
    assert pose_pipeline.SkeletonAction is pl.SkeletonAction and ref_pl.SkeletonAction is pl.SkeletonAction
    ns = {}
    exec("from pose_pipeline import *", ns)
    assert "SkeletonAction" in ns


def test_missing_files_raise_with_their_paths(monkeypatch, tmp_path):
    """nothing is fetched: without the files (and without the synthetic switch) the paths are named"""
    import socket
    monkeypatch.setattr(socket, "socket", lambda *a, **k: (_ for _ in ()).throw(AssertionError("network access")))
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    monkeypatch.delenv("POSEPIPE_SYNTHETIC_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError, match="mmaction2/tools/data/ava/label_map.txt"):
        W.get_label_map()
    with pytest.raises(FileNotFoundError, match="mmaction2/checkpoints/posec3d_ava.pth") as e:
        W.load_state_dict(PM.PoseC3DSpec())
    assert str(tmp_path) in str(e.value)
    # a label map at the expected place is read in the reference's `id: name` form; num_classes follows the largest id
    path = tmp_path / "mmaction2" / "tools" / "data" / "ava"
    path.mkdir(parents=True)
    (path / "label_map.txt").write_text("1: bend/bow (at the waist)\n3: crouch/kneel\n80: watch (a person)\n")
    assert W.get_label_map() == {1: "bend/bow (at the waist)", 3: "crouch/kneel", 80: "watch (a person)"}
    monkeypatch.setattr(W, "_cache", {})
    with pytest.raises(FileNotFoundError, match="posec3d_ava.pth"):   # the label map is there, the checkpoint is not
        W._model(0)
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    (path / "label_map.txt").unlink()
    assert W.get_label_map() == {i: f"class_{i}" for i in range(1, 81)}
    sd = W.load_state_dict(TINY)
    assert {k: v.shape for k, v in sd.items()} == PM.posec3d_param_shapes(TINY)
