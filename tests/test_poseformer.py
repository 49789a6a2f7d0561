"""PoseFormer lifting without a device: the wrapper's pre- and post-processing against golden vectors recorded from the reference's own
`process_liftformer` (tests/golden/make_goldens_poseformer.py), the two references against each other, the parameter inventory, the
checkpoint prefix, the spatial-stage reuse, the module path, the argument errors and the padded program's blob."""
import datetime
import os

import numpy as np
import pytest
import torch

from posepipeline_amd import _lib as L
from posepipeline_amd.models import poseformer as M
from posepipeline_amd.wrappers import poseformer as W
from tests import poseformer_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseformer_pre.npz")
SPEC = M.PoseFormerSpec()


@pytest.fixture(scope="module")
def sd():
    return M.synth_params(M.poseformer_param_shapes(SPEC), seed=11)


class _IndexModel:
    """what the golden script put in the network's place: window i -> i in every element"""

    def __init__(self):
        self.inputs = []

    def lift(self, x):
        self.inputs.append(np.array(x))
        n = x.shape[0] - 80
        return np.broadcast_to(np.arange(n, dtype=np.float32)[:, None, None], (n, 17, 3)).copy()


@pytest.mark.parametrize("clip", ["a", "b"])
def test_golden_windows(clip):
    g = np.load(GOLDEN)
    kp, (height, width) = g[f"kp_{clip}"], g[f"hw_{clip}"]
    assert (width > height) == (clip == "a") and kp.dtype == np.float32 and kp.shape == (84, 17, 3)
    h36m = W.coco_h36m(kp[..., :2])
    assert h36m.dtype == np.float32
    x = W.normalize(h36m, height, width)
    assert x.dtype == np.float64
    wins = W.windows(x).astype(np.float32)                # torch.Tensor(...) of the reference rounds to float32
    assert wins.shape == (4, 81, 17, 2)
    assert np.array_equal(wins, g[f"windows_{clip}"])
    # the quirk: x over the height, y over the width
    h64 = h36m.astype(np.float64)
    assert np.array_equal(x[..., 0], h64[..., 0] / float(height)) and np.array_equal(x[..., 1], h64[..., 1] / float(width))


@pytest.mark.parametrize("clip", ["a", "b"])
def test_golden_assembly(clip, monkeypatch):
    from posepipeline_amd import djshim, pipeline as pl
    g = np.load(GOLDEN)
    kp, (height, width) = g[f"kp_{clip}"], g[f"hw_{clip}"]
    djshim.reset()
    vkey = {"video_project": "golden", "filename": clip}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 10, 18)})
    pl.VideoInfo().insert1({**vkey, "timestamps": [], "delta_time": [], "fps": 30.0, "height": int(height), "width": int(width),
                            "num_frames": len(kp)})
    key = {**vkey, "tracking_method": 5, "video_subject_id": 0, "top_down_method": 0}
    pl.TopDownPerson().insert1({**key, "keypoints": kp})
    model = _IndexModel()
    monkeypatch.setattr(W, "_model", lambda device=0: model)
    before = dict(key)
    res = W.process_liftformer(key)
    assert res is key and set(res) - set(before) == {"keypoints_3d"} and all(res[k] == v for k, v in before.items())
    assert res["keypoints_3d"].dtype == np.float64 and np.array_equal(res["keypoints_3d"], g[f"k3d_{clip}"])
    # what reached the model is the reference's network input, window by window
    (x,) = model.inputs
    assert x.dtype == np.float32 and np.array_equal(W.windows(x), g[f"windows_{clip}"])
    djshim.reset()


def test_references_agree(sd):
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 1, (83, 17, 2))
    sd64 = R.as_dtype(sd, np.float64)
    a = R.forward_windows(x, sd64)
    b = R.torch_forward_windows(x, sd64, torch.float64)
    assert a.shape == b.shape == (3, 17, 3) and a.dtype == b.dtype == np.float64
    assert 0.1 < np.abs(a).max() < 20, np.abs(a).max()          # the synthetic weights give outputs of order one
    assert np.abs(a - b).max() <= 1e-12, np.abs(a - b).max()


def test_param_shapes():
    shapes = M.poseformer_param_shapes(SPEC)
    assert len(shapes) == 110
    assert sum(int(np.prod(s)) for s in shapes.values()) == 9_602_885
    assert set(shapes) == set(R.PoseTransformerT().state_dict())
    assert {k: tuple(v.shape) for k, v in R.PoseTransformerT().state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    assert shapes["weighted_mean.weight"] == (1, 81, 1) and shapes["blocks.3.attn.qkv.weight"] == (1632, 544)


def test_module_prefix(sd, tmp_path, monkeypatch):
    pref = {"module." + k: v for k, v in sd.items()}
    got = M.checked_state_dict(SPEC, pref)
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    a, b = M.build_poseformer_program(SPEC, sd), M.build_poseformer_program(SPEC, pref)
    assert np.array_equal(a.blob, b.blob) and a.named == b.named and a.param_offsets == b.param_offsets
    assert set(a.named) == {"input", "output"}          # buffer ids only: the parameter blocks' offsets are a table of their own
    # a tensor of another shape fails at load (weighted_mean.weight's shape is one of the unpinned points)
    with pytest.raises(ValueError, match="weighted_mean.weight"):
        M.build_poseformer_program(SPEC, {**sd, "weighted_mean.weight": sd["weighted_mean.weight"][:, :80]})
    # through the checkpoint file: checkpoint["model_pos"] of an nn.DataParallel model
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    monkeypatch.delenv("POSEPIPE_SYNTHETIC_WEIGHTS", raising=False)
    os.makedirs(tmp_path / "poseformer")
    torch.save({"model_pos": {k: torch.from_numpy(v) for k, v in pref.items()}}, str(tmp_path / "poseformer" / "detected81f.bin"))
    loaded = W.load_state_dict()
    assert set(loaded) == set(sd) and all(np.array_equal(loaded[k], sd[k]) for k in sd)
    # a missing key is a KeyError (the reference loads with strict=False)
    short = dict(pref)
    del short["module.head.1.bias"]
    torch.save({"model_pos": {k: torch.from_numpy(v) for k, v in short.items()}}, str(tmp_path / "poseformer" / "detected81f.bin"))
    with pytest.raises(KeyError, match="head.1.bias"):
        W.load_state_dict()
    with pytest.raises(KeyError, match="head.1.bias"):
        M.build_poseformer_program(SPEC, {k: v for k, v in sd.items() if k != "head.1.bias"})


def test_spatial_stage_once_per_frame_is_exact(sd):
    """the spatial transformer sees each frame on its own: evaluating it once per frame of the clip gives, in float64, exactly what
    evaluating it inside every window gives"""
    rng = np.random.default_rng(2)
    x = rng.uniform(0, 1, (86, 17, 2))
    sd64 = R.as_dtype(sd, np.float64)
    per_window, per_clip = R.forward_windows(x, sd64), R.forward_clip(x, sd64, batch=4)
    assert per_window.shape == (6, 17, 3) and np.array_equal(per_window, per_clip)


def test_module_path():
    import pose_pipeline.wrappers.poseformer as shim
    assert shim is W and shim.process_liftformer is W.process_liftformer
    from pose_pipeline.wrappers.poseformer import process_liftformer
    assert process_liftformer is W.process_liftformer


def test_errors_before_any_device(monkeypatch):
    from posepipeline_amd import djshim, pipeline as pl

    def no_device(*a, **k):
        raise AssertionError("a device object was created")
    lifter_cls = W.PoseFormerLifter
    monkeypatch.setattr(L, "Context", no_device)
    monkeypatch.setattr(W, "PoseFormerLifter", no_device)
    W._cache.clear()
    djshim.reset()
    for name, kp in (("short", np.ones((80, 17, 3), np.float32)), ("wholebody", np.ones((90, 133, 3), np.float32))):
        vkey = {"video_project": "err", "filename": name}
        pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 10, 18)})
        pl.VideoInfo().insert1({**vkey, "timestamps": [], "delta_time": [], "fps": 30.0, "height": 480, "width": 640, "num_frames": len(kp)})
        key = {**vkey, "tracking_method": 5, "video_subject_id": 0, "top_down_method": 0}
        pl.TopDownPerson().insert1({**key, "keypoints": kp})
        with pytest.raises(ValueError, match="81 frames" if name == "short" else "17"):
            W.process_liftformer(key)
        assert "keypoints_3d" not in key
    djshim.reset()
    with pytest.raises(ValueError, match="81 frames"):
        W.windows(np.zeros((80, 17, 2)))
    with pytest.raises(ValueError, match="17"):
        W.coco_h36m(np.zeros((90, 133, 2)))
    # the lifter's own argument check sits in front of the device call as well
    lifter = lifter_cls.__new__(lifter_cls)
    with pytest.raises(ValueError, match="81 frames"):
        lifter.lift(np.zeros((80, 17, 2), np.float32))
    with pytest.raises(ValueError, match="17"):
        lifter.lift(np.zeros((90, 133, 2), np.float32))


def _conv_blocks(prog):
    """(op, name, W [cout_pad16][K], bias [cout_pad16]) of every convolution, unpacked from the blob's MFMA operand order"""
    for op, name in zip(prog.ops, prog.op_names):
        if op.type != L.PP_OP_CONV:
            continue
        k = op.kh * op.kw * op.cin
        kp, cp = (k + 31) // 32 * 32, (op.cout + 15) // 16 * 16
        w = prog.blob[op.w_off:op.w_off + kp * cp].reshape(kp // 32, cp, 4, 8)          # [chunk][cout][g][s], k = chunk * 32 + 4 s + g
        w = np.transpose(w, (1, 0, 3, 2)).reshape(cp, kp)
        yield op, name, w, prog.blob[op.b_off:op.b_off + cp]


def test_program_and_padding(sd):
    plain = M.build_poseformer_program(SPEC, sd, 0)
    padded = M.build_poseformer_program(SPEC, sd, 128)
    for prog, c, hid in ((plain, 544, 1088), (padded, 640, 1152)):
        assert prog.bufs[prog.named["input"]] == (1, 81, c) and prog.bufs[prog.named["output"]] == (1, 81, c)
        types = [op.type for op in prog.ops]
        assert types == [L.PP_OP_LAYERNORM, L.PP_OP_CONV, L.PP_OP_ATTENTION, L.PP_OP_CONV, L.PP_OP_LAYERNORM, L.PP_OP_CONV,
                         L.PP_OP_GELU_ADD, L.PP_OP_CONV] * 4 + [L.PP_OP_LAYERNORM]
        att = [op for op in prog.ops if op.type == L.PP_OP_ATTENTION]
        assert all((op.cin, op.cout, op.stride) == (544, c, 8) for op in att) and L.PP_OP_ATTENTION == 15
        assert [op.cout for op in prog.ops if op.type == L.PP_OP_CONV] == [3 * c, c, hid, c] * 4
        # the blocks the lift reads ride in the blob
        s0, p0, h0 = prog.param_offsets["spatial_params"], prog.param_offsets["temporal_pos"], prog.param_offsets["head_params"]
        assert s0 % 4 == 0 and p0 % 4 == 0 and h0 % 4 == 0 and h0 + 28972 <= prog.blob.size
        assert np.array_equal(prog.blob[s0:s0 + 34880], M.spatial_param_block(SPEC, sd))
        assert np.array_equal(prog.blob[p0:p0 + 81 * 544], sd["Temporal_pos_embed"].reshape(-1))
        assert np.array_equal(prog.blob[h0 + 88 + 1088:h0 + 88 + 1088 + 51 * 544], sd["head.1.weight"].reshape(-1))
    # the padded program: the real weights in place, exact zeros in every padding row and column
    for (op, name, w, b), (op0, _, w0, b0) in zip(_conv_blocks(padded), _conv_blocks(plain)):
        cin0, cout0 = op0.cin, op0.cout
        if name.endswith("attn.qkv"):          # q | k | v each in its own third of the padded channels
            w3, b3 = w[:op.cout].reshape(3, 640, -1), b[:op.cout].reshape(3, 640)
            assert np.array_equal(w3[:, :544, :544].reshape(1632, 544), w0[:1632, :544]) and np.array_equal(b3[:, :544].reshape(-1), b0[:1632])
            assert not w3[:, 544:].any() and not w3[:, :, 544:].any() and not b3[:, 544:].any() and not w[op.cout:].any()
        else:
            assert np.array_equal(w[:cout0, :cin0], w0[:cout0, :cin0]) and np.array_equal(b[:cout0], b0[:cout0])
            assert not w[cout0:].any() and not w[:, cin0:].any() and not b[cout0:].any()
    for op in padded.ops:
        if op.type == L.PP_OP_LAYERNORM:       # gamma and beta are zero beyond the 544 real channels; eps follows beta
            assert op.cin == 544 and op.cout == 640
            assert not padded.blob[op.w_off + 544:op.w_off + 640].any() and not padded.blob[op.b_off + 544:op.b_off + 640].any()
            want = 1e-6
            assert padded.blob[op.b_off + 640] == np.float32(want)
