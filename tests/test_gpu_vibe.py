"""The SMPL stage (VIBE) on the GPU: the per-sample warp, the GRU, the body model, the head, the backbone program and the wrapper on
the table shim, against tests/vibe_ref.py.

Tolerance (the project's rule, tests/test_gpu_poseformer.py:4-7): in each test `dev32` is the largest deviation, on that test's own
inputs, of the torch float32 CPU evaluation from the float64 reference; the GPU result must lie within FACTOR = 4 x dev32 of the
float64 reference.  Integer and selection results (crop bytes, shapes, row counts) are bit-equal.  Every ratio is printed;
DESIGN_LOG.md 5m is where a GPU visit records them.
"""
import datetime

import numpy as np
import pytest
import torch

from oracle import preprocess as opre
from posepipeline_amd import _lib as L
from posepipeline_amd import ops
from posepipeline_amd.models import smpl as S
from posepipeline_amd.models import synth
from posepipeline_amd.models import vibe as VM
from posepipeline_amd.program import Net
from posepipeline_amd.utils import bounding_box as BB
from posepipeline_amd.wrappers import vibe as W
from tests import vibe_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def _check(got, ref32, ref64, what):
    dev = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    assert dev > 0, what
    print(f"{what}: GPU vs float64 {err:.3e}, float32-on-CPU vs float64 (dev32) {dev:.3e}, ratio {err / dev:.2f} (bound {FACTOR:g}), "
          f"max |ref| {np.abs(ref64).max():.3g}")
    assert err <= FACTOR * dev, (what, err, dev, err / dev)


# ---- 1. the per-sample warp ------------------------------------------------------------------------------------------------------------
def test_warp_affine_normalize_each(ctx):
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    # (frame, box TLWH): inside the frame; partly outside (left and top); odd sub-pixel corners
    cases = [(0, (10.0, 8.0, 30.0, 30.0)), (1, (-12.0, -7.0, 40.0, 40.0)), (1, (13.37, 5.81, 29.53, 29.53))]
    dst = np.float32([[0, 0], [224, 224], [0, 224]])
    mats = []
    for _, (x, y, w, h) in cases:
        mats.append(opre.get_affine_transform_cv(np.float32([[x, y], [x + w, y + h], [x, y + h]]), dst))
    idx = [f for f, _ in cases]
    lut = ops.normalize_lut(VM.MEAN, VM.STD)
    cm = (2, 1, 0)
    got = ops.warp_affine_normalize_each(ctx, frames, idx, np.stack(mats), (224, 224), lut, cm, want_crop_u8=True)
    assert got["out"].shape == (3, 224, 224, 4) and got["crop_u8"].shape == (3, 224, 224, 3)
    for i, (f, _) in enumerate(cases):
        want = opre.warp_affine_u8(frames[f], mats[i], (224, 224))
        assert np.array_equal(got["crop_u8"][i], want), i
        for c in range(3):
            assert np.array_equal(got["out"][i, :, :, c], lut[c][want[:, :, cm[c]]]), (i, c)
        assert not got["out"][i, :, :, 3].any()
    assert (got["crop_u8"][1][:30, :30] == 0).all() and got["crop_u8"][1].any()          # the border is 0, the rest is image
    assert np.array_equal(lut, opre.normalize_lut(np.asarray(VM.MEAN, np.float32), np.asarray(VM.STD, np.float32)))
    # a frame index out of range is refused
    bad = ctx.lib.pp_warp_affine_normalize_each(ctx.handle, L.ptr(frames), 2, 48, 64, L.ptr(np.array([2], np.int32)), L.ptr(np.stack(mats[:1])), 1,
                                                224, 224, L.ptr(lut), L.ptr(np.asarray(cm, np.int32)), L.ptr(got["out"]), None, L.PP_MEM_HOST)
    assert bad == -1 and "out of range" in L.last_error()


# ---- 2. the GRU -------------------------------------------------------------------------------------------------------------------------
def _gru_case(b, t, inp, hid, layers, seed=0):
    rng = np.random.default_rng(seed + hid)
    k = 1.0 / np.sqrt(hid)
    params = []
    for l in range(layers):
        i = inp if l == 0 else hid
        params.append(tuple(rng.uniform(-k, k, s).astype(np.float32) for s in ((3 * hid, i), (3 * hid, hid), (3 * hid,), (3 * hid,))))
    x = rng.standard_normal((b, t, inp)).astype(np.float32)
    return x, params


@pytest.mark.parametrize("b,t,inp,hid,layers", [(1, 1, 4, 4, 1), (3, 5, 8, 20, 2), (2, 32, 2048, 1024, 2)],
                         ids=["1x1_4to4", "3x5_8to20_2layers", "2x32_2048to1024_2layers"])
def test_gru_forward(ctx, b, t, inp, hid, layers):
    x, params = _gru_case(b, t, inp, hid, layers)
    ref64 = R.gru_np(x, params)
    ref32 = R.torch_gru(x, params, torch.float32)
    assert np.abs(R.torch_gru(x.astype(np.float64), R_params64(params), torch.float64) - ref64).max() < 1e-12
    g = ops.Gru(ctx, params)
    try:
        got = g.forward(x)
        assert got.shape == (b, t, hid) and got.dtype == np.float32
        _check(got, ref32, ref64, f"GRU B={b} T={t} in={inp} H={hid} layers={layers}")
        assert np.array_equal(g.forward(x), got), "two runs differ"
    finally:
        g.close()


def R_params64(params):
    return [tuple(np.asarray(a, np.float64) for a in lay) for lay in params]


def test_gru_batch_independence(ctx):
    """5 sequences (more than one pass of 4 inside the step kernel): each row is bit-equal to the same sequence run alone"""
    x, params = _gru_case(5, 6, 12, 24, 2, seed=3)
    g = ops.Gru(ctx, params)
    try:
        full = g.forward(x)
        three = g.forward(x[:3])
        assert np.array_equal(three, full[:3])
        for row in (0, 3, 4):
            assert np.array_equal(g.forward(x[row:row + 1])[0], full[row]), row
        # a ragged sequence padded with zero input: the rows in front of the padding are those of the short sequence
        padded = x[:1].copy()
        padded[0, 4:] = 0
        assert np.array_equal(g.forward(padded)[0, :4], g.forward(x[:1, :4])[0])
    finally:
        g.close()


def test_gru_argument_errors(ctx):
    x, params = _gru_case(1, 2, 4, 8, 1)
    g = ops.Gru(ctx, params)
    y = np.full((1, 2, 8), 7.0, np.float32)
    call = lambda **kw: ctx.lib.pp_gru_forward(ctx.handle, kw.get("x", L.ptr(x)), kw.get("b", 1), kw.get("t", 2), kw.get("inp", 4),   # noqa: E731
                                               kw.get("hid", 8), kw.get("layers", 1), kw.get("params", L.ptr(g.params)), kw.get("y", L.ptr(y)),
                                               kw.get("mem", L.PP_MEM_HOST))
    try:
        for bad in (dict(hid=6), dict(hid=0), dict(layers=0), dict(t=0), dict(b=0), dict(inp=0), dict(x=None), dict(params=None), dict(y=None),
                    dict(mem=5)):
            assert call(**bad) == -1, (bad, L.last_error())
            assert (y == 7.0).all(), bad                      # nothing ran
        assert call(hid=6) == -1 and "multiple of 4" in L.last_error()
        assert call() == 0 and not (y == 7.0).any()
        assert ctx.lib.pp_gru_param_floats(2048, 1024, 2) == 3 * 1024 * (2048 + 1024 + 2) + 3 * 1024 * (1024 + 1024 + 2)
    finally:
        g.close()


# ---- 3. the body model --------------------------------------------------------------------------------------------------------------------
def _random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def _smpl_case(n_verts, f, seed):
    rng = np.random.default_rng(seed)
    body = S.synth_body_model(seed, n_verts)
    rot = _random_rotations(rng, f * 24).reshape(f, 24, 3, 3)
    rot[1] = np.eye(3)                                          # one frame at rest: the sin^2 = 0 branch of the axis-angle
    rot[2, 5] = R.rodrigues_np(np.array([[0.0, np.pi - 0.01, 0.0]]))[0]      # and one joint turned by nearly pi: another quaternion branch
    rot = rot.astype(np.float32)
    betas = rng.standard_normal((f, 10)).astype(np.float32)
    cam = np.stack([rng.uniform(0.6, 1.2, f), rng.uniform(-0.2, 0.2, f), rng.uniform(-0.2, 0.2, f)], axis=1).astype(np.float32)
    return body, rot, betas, cam


def _check_smpl(got, body, rot, betas, cam, n_verts, what):
    ids, jm = S.vertex_ids(n_verts), S.JOINT_MAP_54
    verts64, j64, _ = R.smpl_np(body, betas, rot, ids, jm)
    kp64 = R.project_np(j64, cam)
    t32 = R.torch_smpl(body, betas, rot, cam, ids, jm, torch.float32)
    if got["verts"] is not None:
        _check(got["verts"], t32["verts"], verts64, what + " verts")
    _check(got["joints3d"], t32["joints3d"], j64, what + " joints3d")
    _check(got["kp2d"], t32["kp2d"], kp64, what + " kp2d")
    # pose_aa through reconstruction: Rodrigues of it is the rotation matrix; the angle lies in [0, pi]
    rot64 = rot.astype(np.float64).reshape(-1, 3, 3)
    _check(R.rodrigues_np(got["pose_aa"].reshape(-1, 3)), R.rodrigues_np(t32["pose_aa"].reshape(-1, 3)), rot64, what + " Rodrigues(pose_aa)")
    angle = np.linalg.norm(got["pose_aa"].reshape(-1, 3).astype(np.float64), axis=1)
    assert angle.max() <= np.pi * (1 + 2.0 ** -23) and angle.max() > 3.0
    assert not got["pose_aa"][1].any()                          # the frame at rest: k = 2, zero vector
    assert np.isfinite(got["pose_aa"]).all()


@pytest.mark.parametrize("n_verts,f", [(37, 5), (6890, 3)], ids=["37_vertices", "6890_vertices"])
def test_smpl_forward(ctx, n_verts, f):
    body, rot, betas, cam = _smpl_case(n_verts, f, seed=11)
    m = ops.SmplModel(ctx, body, S.vertex_ids(n_verts), S.JOINT_MAP_54)
    try:
        got = m.forward(betas, rot, cam)
        assert got["verts"].shape == (f, n_verts, 3) and got["joints3d"].shape == (f, 49, 3) and got["kp2d"].shape == (f, 49, 2)
        _check_smpl(got, body, rot, betas, cam, n_verts, f"SMPL V={n_verts} F={f}")
        # without the mesh: the same joints bit for bit; two runs: the same bits
        lean = m.forward(betas, rot, cam, want_verts=False)
        assert lean["verts"] is None
        again = m.forward(betas, rot, cam)
        for k in ("joints3d", "kp2d", "pose_aa"):
            assert np.array_equal(lean[k], got[k]) and np.array_equal(again[k], got[k]), k
        assert np.array_equal(again["verts"], got["verts"])
        # a frame's result does not depend on the frames it rides with
        one = m.forward(betas[2:3], rot[2:3], cam[2:3])
        assert np.array_equal(one["joints3d"][0], got["joints3d"][2]) and np.array_equal(one["verts"][0], got["verts"][2])
    finally:
        m.close()


def test_smpl_model_argument_errors(ctx):
    body = S.synth_body_model(1, 37)
    with pytest.raises(L.PosePipeHipError, match="vertex_ids"):
        ops.SmplModel(ctx, body, np.full(21, 37, np.int32), S.JOINT_MAP_54)
    with pytest.raises(L.PosePipeHipError, match="joint_map"):
        ops.SmplModel(ctx, body, S.vertex_ids(37), np.full(49, 54, np.int32))


# ---- 4. the head: encoder + regressor + body model ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vibe_sd():
    return VM.synth_params(VM.vibe_param_shapes(), seed=21)


@pytest.fixture(scope="module")
def head_case(vibe_sd):
    """39 feature rows = one full sequence of 32 and a ragged one of 7, and their references, computed once"""
    rng = np.random.default_rng(8)
    feats = np.abs(rng.standard_normal((39, 2048))).astype(np.float32)
    body = S.synth_body_model(4, 37)
    ids, jm = S.vertex_ids(37), S.JOINT_MAP_54
    ref64 = R.head_np(feats, vibe_sd, body, ids, jm)
    ref32 = R.torch_head(feats, vibe_sd, body, ids, jm, torch.float32)
    return feats, body, ref64, ref32


def _check_fields(got, ref32, ref64, what, fields=("cam", "betas", "verts", "joints3d", "kp2d")):
    for k in fields:
        _check(got[k], ref32[k], ref64[k], f"{what} {k}")
    _check(R.rodrigues_np(got["pose_aa"].reshape(-1, 3)), R.rodrigues_np(ref32["pose_aa"].reshape(-1, 3)), ref64["rotmat"].reshape(-1, 3, 3),
           f"{what} Rodrigues(pose_aa)")


@pytest.mark.parametrize("numerics", [None, "split"], ids=["suite_numerics", "split"])
def test_head(ctx, vibe_sd, head_case, numerics):
    feats, body, ref64, ref32 = head_case
    model = W.VibeModel(ctx=ctx, numerics=numerics, vibe_sd=vibe_sd, body=body, backbone=False)
    n = feats.shape[0]
    padded = np.zeros((64, 2048), np.float32)
    padded[:n] = feats
    dev = ctx.malloc(padded.nbytes)
    try:
        if numerics == "split":
            assert model.head.numerics == "split" and (model.head.conv_kinds() == 2).any()
        ctx.h2d(dev, padded)
        got = model.run_head(dev, n)
        assert got["joints3d"].shape == (n, 49, 3) and got["verts"].shape == (n, 37, 3) and got["pose_aa"].shape == (n, 72)
        _check_fields(got, ref32, ref64, f"head ({model.head.numerics})")
        again = model.run_head(dev, n, timed=True)
        assert all(np.array_equal(again[k], got[k]) for k in got) and (model.stage_ms > 0).all()
        # the ragged sequence alone: its frames see no state of the sequence in front of it
        ctx.h2d(dev, np.concatenate([feats[32:], np.zeros((25, 2048), np.float32)]))
        alone = model.run_head(dev, 7)
        assert all(np.array_equal(alone[k], got[k][32:]) for k in got)
    finally:
        ctx.free(dev)
        model.close()


# ---- 5. the backbone program -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spin_sd():
    return synth.synth_state_dict(VM.spin_param_shapes(), seed=31)


def test_backbone_program(ctx, spin_sd):
    rng = np.random.default_rng(2)
    crops = rng.integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    lut = opre.normalize_lut(np.asarray(VM.MEAN, np.float32), np.asarray(VM.STD, np.float32))
    x = np.stack([lut[c][crops[..., c]] for c in range(3)], axis=1).astype(np.float32)          # NCHW
    ref64 = R.torch_backbone(x.astype(np.float64), spin_sd, torch.float64)
    ref32 = R.torch_backbone(x, spin_sd, torch.float32)
    xin = np.zeros((2, 224, 224, 4), np.float32)
    xin[..., :3] = np.transpose(x, (0, 2, 3, 1))
    net = Net(ctx, VM.build_backbone_program(spin_sd), max_batch=2)
    try:
        got = net.forward(xin, "input", "features").reshape(2, 2048)
        _check(got, ref32, ref64, "backbone features")
    finally:
        net.close()


# ---- 6. the wrapper on the table shim ------------------------------------------------------------------------------------------------------
def test_process_vibe_through_the_tables(monkeypatch, tmp_path):
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path / "no_checkpoints"))
    from posepipeline_amd import djshim, pipeline as pl, video
    djshim.reset()
    W._cache.clear()
    rng = np.random.default_rng(13)
    n, height, width = 40, 48, 64
    frames = rng.integers(0, 256, (n, height, width, 3), dtype=np.uint8)
    path = str(tmp_path / "clip.ppvid")
    video.write_ppvid(path, frames, 30.0)
    bbox = np.stack([rng.uniform(2, 25, n), rng.uniform(-4, 10, n), rng.uniform(15, 34, n), rng.uniform(20, 40, n)], axis=1)
    present = np.ones(n, bool)
    present[[3, 20]] = False
    vkey = {"video_project": "test", "filename": "vibe"}
    pl.Video().insert1({**vkey, "video": path, "start_time": datetime.datetime(2024, 10, 18)})
    pl.VideoInfo().insert1({**vkey, "timestamps": [], "delta_time": [], "fps": 30.0, "height": height, "width": width, "num_frames": n})
    pkey = {**vkey, "tracking_method": 5, "video_subject_id": 0}
    pl.PersonBbox().insert1({**pkey, "bbox": bbox, "present": present})
    key = {**pkey, "smpl_method": 0}
    try:
        res = W.process_vibe(dict(key))
        shapes = {k: res[k].shape for k in ("cams", "verts", "poses", "betas", "joints3d", "joints2d")}
        assert shapes == {"cams": (38, 4), "verts": (38, 6890, 3), "poses": (38, 72), "betas": (38, 10), "joints3d": (38, 49, 3), "joints2d": (38, 49, 2)}
        # the float64 chain: the oracle's crop, the torch backbone, the numpy head in two sequences (32 + 6), the box helpers
        ids, boxes, _, x = R.crop_reference(frames, bbox, present, opre)
        assert ids.tolist() == [i for i in range(n) if i not in (3, 20)] and len(ids) == 38
        spin, vibe = W.load_state_dicts()
        body = S.load_body_model()
        vids, jm = S.vertex_ids(6890), S.JOINT_MAP_54
        f64 = R.torch_backbone(x.astype(np.float64), spin, torch.float64)
        f32 = R.torch_backbone(x, spin, torch.float32)
        ref64 = R.head_np(f64, vibe, body, vids, jm)
        ref32 = R.torch_head(f32, vibe, body, vids, jm, torch.float32)
        for r in (ref64, ref32):
            r["cams"] = BB.convert_crop_cam_to_orig_img(r["cam"], boxes, width, height)
            r["joints2d"] = BB.convert_crop_coords_to_orig_img(boxes, r["kp2d"], 224)
        got = dict(res, pose_aa=res["poses"])
        _check_fields(got, ref32, ref64, "process_vibe", fields=("cams", "betas", "verts", "joints3d", "joints2d"))
        # two sequences: frame 32 of the present frames starts from a zero state -- one sequence of 38 gives other values there
        one_seq = R.head_np(f64, vibe, body, vids, jm, seq=38)
        assert np.abs(one_seq["joints3d"][32:] - ref64["joints3d"][32:]).max() > 100 * np.abs(got["joints3d"][32:] - ref64["joints3d"][32:]).max()
        # through the tables: one row, no mesh
        pl.SMPLMethod().insert1(key)
        pl.SMPLPerson().populate(key)
        row = (pl.SMPLPerson & key).fetch1()
        assert len(pl.SMPLPerson()) == 1 and "verts" not in row and row["model_type"] == "SMPL"
        for k in ("cams", "poses", "betas", "joints3d", "joints2d"):
            assert np.array_equal(row[k], res[k]), k
        # no present frame: an error that names the key
        pl.PersonBbox().insert1({**pkey, "video_subject_id": 1, "bbox": bbox, "present": np.zeros(n, bool)})
        with pytest.raises(ValueError, match="present in no frame"):
            W.process_vibe({**key, "video_subject_id": 1})
    finally:
        for m in W._cache.values():
            m.close()
        W._cache.clear()
        djshim.reset()
