"""pp_gastnet_lift_many: the GAST-Net chunk loop, flip merge and camera rotation of every track in one device-side call, and the
streamed cascade that lifts with it (Cascade(lifter="GastNet")).

A work item is one (track, chunk) pair: the window and its mirror image in two neighbouring batch samples, packed on the device with
the halo clamped to its own track; the pair is averaged, rotated and scattered by a second kernel whose float32 operations are those
of the host formulas one by one.  So every track's result must be `camera_to_world(GastNetLifter.lift(track))` -- the host chunk loop
on the same net -- BIT FOR BIT, in both numerics, whatever shares the batch with it and wherever a batch group ends."""
import datetime
import os

import numpy as np
import pytest
import torch

from posepipeline_amd import _lib as L
from posepipeline_amd.models import gastnet as M
from posepipeline_amd.wrappers import gastnet as W
from tests.test_gpu_gastnet import FACTOR, SMALL, _ref_lift, _rot64

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEGS = (1, 7, 8, 9, 29)              # one frame; a chunk less one, a whole chunk, a chunk and one; three chunks and a ragged one
SENTINEL = F32(-777.25)


@pytest.fixture(scope="module")
def sd_small():
    return M.synth_params(M.gastnet_param_shapes(SMALL), seed=3)


def _segments(lengths=SEGS, seed=21):
    """tracks at visibly different offsets: a row that read the neighbouring segment instead of its own clamped edge shows"""
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-0.2, 0.2, (n, 17, 2)) + 0.15 * (i - 2)).astype(F32) for i, n in enumerate(lengths)]


def _call(lf, segs, flip, quat, sentinel=SENTINEL, pad=None, bufs=("input", "output"), seg=None):
    """the C entry with host arrays -> (rc, the packed output, pre-filled with the sentinel and two guard rows behind it)"""
    seg = np.array([len(s) for s in segs], np.int32) if seg is None else seg
    rows = int(sum(len(s) for s in segs))
    packed = np.ascontiguousarray(np.concatenate(segs)) if segs else np.zeros((1, 17, 2), F32)
    out = np.full((rows + 2, 17, 3), sentinel, F32)
    named = lf.net.prog.named
    rc = lf.ctx.lib.pp_gastnet_lift_many(lf.net.handle, named[bufs[0]], named[bufs[1]], L.ptr(packed), L.ptr(seg), len(seg),
                                         lf.spec.pad if pad is None else pad, int(flip), L.ptr(quat), L.ptr(out), L.PP_MEM_HOST)
    return rc, out


def _split(out, segs):
    ends = np.cumsum([len(s) for s in segs])
    return [out[e - len(s):e] for e, s in zip(ends, segs)]


# ---- 1. every segment equals the host chunk loop on the same net -------------------------------------------------------------------
@pytest.mark.parametrize("max_batch", [2, 6])
@pytest.mark.parametrize("numerics", ["exact", "split"])
def test_segments_equal_the_host_chain(ctx, sd_small, numerics, max_batch):
    """max_batch 2: one work item per batch group; 6: three, the nine items of the five segments in groups that end mid-segment"""
    segs = _segments()
    lf = W.GastNetLifter(numerics=numerics, ctx=ctx, state_dict=sd_small, spec=SMALL, max_batch=max_batch)
    nf = W.GastNetLifter(numerics=numerics, ctx=ctx, state_dict=sd_small, spec=SMALL, max_batch=max_batch, flip_augment=False)
    try:
        assert lf.net.numerics == numerics and lf.net.max_batch == max_batch
        host = [lf.lift(s) for s in segs]
        host_nf = [nf.lift(s) for s in segs]
        assert all(np.isfinite(h).all() and np.abs(h).max() > 1e-4 for h in host)
        assert not np.array_equal(host[4], host_nf[4])                                  # the mirror image does contribute
        # flip + rotation: the wrapper, and the raw call into a sentinel-filled array (rows packed tightly, nothing behind them)
        got = lf.lift_many(segs)
        assert [g.shape for g in got] == [(n, 17, 3) for n in SEGS] and all(g.dtype == F32 for g in got)
        rc, raw = _call(lf, segs, 1, W.CAMERA_QUATERNION)
        assert rc == 0, L.last_error()
        assert (raw[-2:] == SENTINEL).all() and not (raw[:-2] == SENTINEL).any()
        for i, (g, r, h) in enumerate(zip(got, _split(raw[:-2], segs), host)):
            want = W.camera_to_world(h)
            assert np.array_equal(g, want), (numerics, max_batch, i, np.abs(g - want).max())
            assert np.array_equal(r, want), (numerics, max_batch, i)
        # no rotation
        for i, (g, h) in enumerate(zip(lf.lift_many(segs, rotate=False), host)):
            assert np.array_equal(g, h), (numerics, max_batch, i, np.abs(g - h).max())
        # no flip: one sample per work item
        for i, (g, h) in enumerate(zip(nf.lift_many(segs), host_nf)):
            assert np.array_equal(g, W.camera_to_world(h)), (numerics, max_batch, i)
        for i, (g, h) in enumerate(zip(nf.lift_many(segs, rotate=False), host_nf)):
            assert np.array_equal(g, h), (numerics, max_batch, i)
        # two runs: the same bytes
        rc2, raw2 = _call(lf, segs, 1, W.CAMERA_QUATERNION)
        assert rc2 == 0 and raw2.tobytes() == raw.tobytes()
        # a segment's result does not depend on its neighbours in the call
        alone = lf.lift_many([segs[3]])[0]
        assert np.array_equal(alone, got[3])
    finally:
        lf.close()
        nf.close()


# ---- 2. device-resident arrays -----------------------------------------------------------------------------------------------------
def test_device_memory_gives_the_same_bytes(ctx, sd_small):
    segs = _segments(seed=22)
    lf = W.GastNetLifter(numerics="split", ctx=ctx, state_dict=sd_small, spec=SMALL, max_batch=6)
    packed = np.ascontiguousarray(np.concatenate(segs))
    seg = np.array([len(s) for s in segs], np.int32)
    host = np.concatenate(lf.lift_many(segs))
    d_in, d_out = ctx.malloc(packed.nbytes), ctx.malloc(host.nbytes)
    try:
        ctx.h2d(d_in, packed)
        ctx.h2d(d_out, np.full_like(host, np.nan))
        named = lf.net.prog.named
        L.check(ctx.lib.pp_gastnet_lift_many(lf.net.handle, named["input"], named["output"], L.ptr(d_in), L.ptr(seg), len(seg), SMALL.pad,
                                             1, L.ptr(W.CAMERA_QUATERNION), L.ptr(d_out), L.PP_MEM_DEVICE), "pp_gastnet_lift_many")
        ctx.synchronize()
        got = np.zeros_like(host)
        ctx.d2h(got, d_out)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
        lf.close()
    assert np.isfinite(got).all() and got.tobytes() == host.tobytes()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause(ctx, sd_small):
    lf = W.GastNetLifter(numerics="exact", ctx=ctx, state_dict=sd_small, spec=SMALL, max_batch=2)
    one = W.GastNetLifter(numerics="exact", ctx=ctx, state_dict=sd_small, spec=SMALL, max_batch=1, flip_augment=False)
    segs = _segments((4, 3))
    q = W.CAMERA_QUATERNION
    try:
        rc, out = _call(lf, segs, 1, q, seg=np.array([4, 0, 3], np.int32))
        assert rc == -1 and "pp_gastnet_lift_many: segment 1 has 0 frames" in L.last_error() and (out == SENTINEL).all()
        rc, out = _call(one, segs, 1, q)
        assert rc == -1 and "flip needs two samples" in L.last_error() and "max_batch 1" in L.last_error() and (out == SENTINEL).all()
        rc, _ = _call(one, segs, 0, q)                                                   # without flip one sample is enough
        assert rc == 0, L.last_error()
        rc, out = _call(lf, segs, 1, q, pad=SMALL.pad + 1)
        assert rc == -1 and "pp_gastnet_lift_many: program shape" in L.last_error() and (out == SENTINEL).all()
        rc, out = _call(lf, segs, 1, q, bufs=("output", "input"))
        assert rc == -1 and "pp_gastnet_lift_many: program shape" in L.last_error() and (out == SENTINEL).all()
        rc, out = _call(lf, segs, 1, q, seg=np.zeros(0, np.int32))                       # n_seg = 0: nothing to do, nothing written
        assert rc == 0 and (out == SENTINEL).all()
        rc, _ = _call(lf, segs, 1, q)
        assert rc == 0, L.last_error()
        with pytest.raises(ValueError, match="max_batch"):
            W.GastNetLifter(numerics="exact", ctx=ctx, state_dict=sd_small, spec=SMALL, max_batch=1)
        with pytest.raises(ValueError, match="no valid frame"):
            lf.lift_many([segs[0], np.zeros((0, 17, 2), F32)])
        assert lf.lift_many([]) == []
    finally:
        lf.close()
        one.close()


def test_a_4_byte_aligned_device_source_is_refused(ctx, sd_small):
    """gast_pack_kernel reads the source as float2: a device source 4 bytes into its allocation is refused, nothing is written"""
    segs = _segments((4, 3))
    lf = W.GastNetLifter(numerics="exact", ctx=ctx, state_dict=sd_small, spec=SMALL, max_batch=2)
    packed = np.ascontiguousarray(np.concatenate(segs))
    seg = np.array([len(s) for s in segs], np.int32)
    filled = np.full((len(packed), 17, 3), SENTINEL, F32)
    d_in, d_out = ctx.malloc(packed.nbytes + 8), ctx.malloc(filled.nbytes)
    try:
        assert d_in % 8 == 0
        ctx.h2d(d_in + 4, packed)
        ctx.h2d(d_out, filled)
        named = lf.net.prog.named
        rc = ctx.lib.pp_gastnet_lift_many(lf.net.handle, named["input"], named["output"], L.ptr(d_in + 4), L.ptr(seg), len(seg), SMALL.pad,
                                          1, L.ptr(W.CAMERA_QUATERNION), L.ptr(d_out), L.PP_MEM_DEVICE)
        err = L.last_error()
        ctx.synchronize()
        got = np.zeros_like(filled)
        ctx.d2h(got, d_out)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
        lf.close()
    assert rc == -1 and "pp_gastnet_lift_many" in err and "8-byte aligned" in err, (rc, err)
    assert (got == SENTINEL).all()


# ---- 4. the table path -------------------------------------------------------------------------------------------------------------
def test_process_gastnet_equals_the_host_chain(tmp_path, monkeypatch):
    """process_gastnet goes through lift_many([x]); what it stores is what it stored before: zeros + camera_to_world(lift(x))"""
    sd_full = M.synth_params(M.gastnet_param_shapes(M.GastNetSpec()), seed=7)
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    monkeypatch.delenv("POSEPIPE_SYNTHETIC_WEIGHTS", raising=False)
    os.makedirs(tmp_path / "gastnet")
    torch.save({"model_pos": {"module." + k: torch.from_numpy(v) for k, v in sd_full.items()}}, str(tmp_path / "gastnet" / "27_frame_model.bin"))
    from posepipeline_amd import djshim, pipeline as pl
    djshim.reset()
    W._cache.clear()
    rng = np.random.default_rng(19)
    height, width, n = 480, 640, 9
    kp = np.empty((n, 17, 3), F32)
    kp[..., :2] = ((320, 240) + rng.uniform(-0.3, 0.3, (n, 17, 2)) * (width, height)).astype(F32)
    kp[..., 2] = 0.9
    kp[3] = 0                                        # no detection
    kp[6, 15, 2] = 0.1                               # COCO left ankle = H36M joint 6 below the threshold: revise_kpts, 6 <- 5
    vkey = {"video_project": "test", "filename": "gast_many"}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 10, 18)})
    pl.VideoInfo().insert1({**vkey, "timestamps": [], "delta_time": [], "fps": 30.0, "height": height, "width": width, "num_frames": n})
    key = {**vkey, "tracking_method": 5, "video_subject_id": 0, "top_down_method": 0, "lifting_method": 0}
    pl.TopDownPerson().insert1({k: v for k, v in key.items() if k != "lifting_method"} | {"keypoints": kp})
    pl.LiftingMethod().insert1(key)
    try:
        pl.LiftingPerson().make(dict(key))
        k3, valid = (pl.LiftingPerson & key).fetch1("keypoints_3d", "keypoints_valid")
        k3, valid = np.asarray(k3), list(valid)
        kpts, scores, v = W.h36m_coco_format(kp[..., :2], kp[..., 2])
        kpts = W.revise_kpts(kpts, scores, v)
        x = W.normalize_screen_coordinates(kpts[v], w=width, h=height).astype(F32)
        want = np.zeros((n, 17, 3))
        want[v] = W.camera_to_world(W._model().lift(x))
        assert valid == [i != 3 for i in range(n)] and v.tolist() == [i for i in range(n) if i != 3]
        assert k3.dtype == F64 and k3.shape == want.shape and np.abs(want[v]).min(axis=(1, 2)).max() > 0
        assert np.array_equal(k3, want), np.abs(k3 - want).max()
    finally:
        for lf in W._cache.values():
            lf.close()
        W._cache.clear()
        djshim.reset()


# ---- 5. the streamed cascade -------------------------------------------------------------------------------------------------------
H, Wd, N, CHUNK = 135, 240, 40, 8


def _clip():
    """two separated persons; the second one has no box in frames 14 .. 19.  The SORT configuration ends an id at its first missed
    frame, so its stream ends there (two forward-filled frames later) and a new id, born at frame 20 and back-filled to 18, takes the
    free place: a track that ends early, one born late, one over the whole clip.  (Invalid frames INSIDE a track need a tracker that
    keeps ids across misses; tests/test_gastnet_stream.py covers them.)"""
    rng = np.random.default_rng(31)
    boxes = [(15, 20, 70, 120), (140, 15, 200, 118)]
    base = rng.integers(0, 60, (H, Wd, 3)).astype(np.uint8)
    frames, gt = [], []
    for t in range(N):
        img, rows = base.copy(), []
        for p, (x1, y1, x2, y2) in enumerate(boxes):
            if p == 1 and 14 <= t < 20:
                continue
            dx = (t % 8) // 2 * (1 if p == 0 else -1)
            img[y1:y2, x1 + dx:x2 + dx] = rng.integers(120, 255, (y2 - y1, x2 - x1, 3))
            rows.append([x1 + dx, y1, x2 + dx, y2, 0.9 - 0.05 * p])
        frames.append(img)
        gt.append(np.array(rows, F32).reshape(-1, 5))
    return np.stack(frames), gt


@pytest.fixture(scope="module")
def cascade_inputs(sd_small):
    from posepipeline_amd.models import faster_rcnn as fr, hrnet, synth
    from posepipeline_amd.models import videopose3d as vp3d
    spec = hrnet.HRNetSpec(32, 17, 256, 192)
    frames, gt = _clip()
    return dict(det_sd=synth.synth_state_dict(fr.faster_rcnn_param_shapes(), seed=2), pose_spec=spec,
                pose_sd=synth.synth_state_dict(hrnet.hrnet_param_shapes(spec), seed=1), gast_sd=sd_small,
                vp3d_sd=synth.synth_state_dict(vp3d.videopose3d_param_shapes(vp3d.VideoPose3DSpec()), seed=3), frames=frames, gt=gt)


def _run(cas, ci):
    from posepipeline_amd.cascade import collect
    outs = [cas.step(ci["frames"][i:i + CHUNK], replay=ci["gt"][i:i + CHUNK]) for i in range(0, N, CHUNK)] + [cas.flush()]
    ids = [[r[0] for r in fr_] for o in outs for fr_ in o["tracks"]]
    return outs, ids, {w: collect(outs, w) for w in outs[0] if not w.endswith("_frames") and w != "tracks"}


@pytest.mark.parametrize("numerics", ["exact", "split"])
def test_cascade_lifts_with_gastnet(ctx, cascade_inputs, numerics):
    from posepipeline_amd.cascade import Cascade
    ci = cascade_inputs
    cas = Cascade(ctx, ci["det_sd"], ci["pose_sd"], ci["gast_sd"], H, Wd, chunk=CHUNK, max_persons=2, pose_spec=ci["pose_spec"],
                  numerics=numerics, lifter="GastNet", lift_spec=SMALL)
    try:
        assert cas.lift_net is cas.gast.net and cas.lift_net.numerics == numerics
        assert cas.lift_net.max_batch == 2 * 2 * 5 and cas.persons.lifter == "GastNet" and cas.persons.pad == 13
        vp_like = cas.detector.flops_per_frame + 2 * 2 * cas.pose_net.prog.flops
        assert cas.flops_per_frame == vp_like + 2 * 2 * cas.lift_net.prog.flops / SMALL.chunk          # both samples of a chunk
        calls = []
        many = cas.persons.lift_many_fn
        cas.persons.lift_many_fn = lambda xs: calls.append(len(xs)) or many(xs)
        outs, ids, got = _run(cas, ci)
        assert len(calls) <= len(outs) and max(calls) == 2                               # one call per step, both persons in it
        k2, k3, kv = got["keypoints"], got["keypoints_3d"], got["keypoints_valid"]
        assert len(k3) == 3 and sorted(k2) == sorted(k3) == sorted(kv)
        spans = sorted((k3[tid][0], len(k3[tid][1])) for tid in k3)
        print(f"cascade GastNet {numerics}: (first frame, frames) per track {spans}")
        # the whole clip; the id that ends at the hole (14 boxes + 2 forward-filled frames); the id born behind it (back-filled)
        assert spans[0] == (0, 16) and spans[1] == (0, N) and 16 < spans[2][0] <= 20 and sum(spans[2]) == N, spans
        worst = 0.0
        for tid in sorted(k3):
            first, rows = k2[tid]
            assert k3[tid][0] == kv[tid][0] == first and len(k3[tid][1]) == len(rows)
            kpts, scores, v = W.h36m_coco_format(rows[:, :17, :2], rows[:, :17, 2])
            kpts = W.revise_kpts(kpts, scores, v)
            x = W.normalize_screen_coordinates(kpts[v], w=Wd, h=H).astype(F32)
            is_valid = np.zeros(len(rows), bool)
            is_valid[v] = True
            assert np.array_equal(kv[tid][1], is_valid) and is_valid.all()
            stream3 = k3[tid][1]
            assert stream3.dtype == F32 and np.isfinite(stream3).all()
            if numerics == "exact":
                # each output is one fixed-order chain over its own window, whatever chunk and batch sample it fell into
                want = W.camera_to_world(cas.gast.lift(x))
                assert np.array_equal(stream3[v], want), (tid, np.abs(stream3[v] - want).max())
            else:
                # the per-sample activation scale depends on which frames share a sample: the FACTOR rule of tests/test_gpu_gastnet.py
                ref64 = _rot64(_ref_lift(x, ci["gast_sd"], SMALL, True, F64))
                ref32 = W.camera_to_world(_ref_lift(x, ci["gast_sd"], SMALL, True, F32))
                dev = float(np.abs(ref32.astype(F64) - ref64).max())
                err = float(np.abs(stream3[v].astype(F64) - ref64).max())
                print(f"cascade GastNet split, track {tid}: GPU vs float64 {err:.3e}, float32-on-CPU vs float64 {dev:.3e}, "
                      f"ratio {err / dev:.2f} (bound {FACTOR:g})")
                worst = max(worst, err / dev)
                assert dev > 0 and err <= FACTOR * dev, (tid, err, dev)
        if numerics == "split":
            print(f"cascade GastNet split: worst ratio {worst:.2f}")
    finally:
        cas.release()
    assert cas.gast is None and cas.lift_net is None


def test_cascade_default_lifter_is_unchanged(ctx, cascade_inputs):
    """lifter="VideoPose3D" is the cascade built without the keyword, byte for byte"""
    from posepipeline_amd.cascade import Cascade
    ci = cascade_inputs
    res = []
    for kw in ({}, {"lifter": "VideoPose3D"}):
        cas = Cascade(ctx, ci["det_sd"], ci["pose_sd"], ci["vp3d_sd"], H, Wd, chunk=CHUNK, max_persons=2, pose_spec=ci["pose_spec"],
                      numerics="split", **kw)
        try:
            assert cas.gast is None and cas.persons.lifter == "VideoPose3D" and cas.lift_spec.pad == 121
            res.append(_run(cas, ci))
        finally:
            cas.release()
    (outs_a, ids_a, got_a), (outs_b, ids_b, got_b) = res
    assert ids_a == ids_b and sorted(got_a) == sorted(got_b) == ["keypoints", "keypoints_3d"]
    for o in outs_a + outs_b:
        assert "keypoints_valid" not in o
    for what in got_a:
        assert sorted(got_a[what]) == sorted(got_b[what]) and len(got_a[what]) == 3
        for tid in got_a[what]:
            a, b = got_a[what][tid], got_b[what][tid]
            assert a[0] == b[0] and a[1].dtype == b[1].dtype and a[1].tobytes() == b[1].tobytes(), (what, tid)
    with pytest.raises(ValueError, match="lifter"):
        Cascade(ctx, ci["det_sd"], ci["pose_sd"], ci["vp3d_sd"], H, Wd, chunk=CHUNK, max_persons=2, pose_spec=ci["pose_spec"], lifter="PoseFormer")
