"""pp_videopose3d_lift_many: every followed person's 2D track lifted in one device-side call.

A work item is one (track, chunk) pair in one batch sample, gathered on the device with the halo clamped to its own track, so each
track's result must be what the single-track call -- and the strided per-window oracle -- gives for that track alone, bit for bit,
whatever shares the batch with it.  Checked against the oracle (exact numerics), against the single call (both numerics), with
device-resident arrays, and through the cascade (batched_lift=True against False)."""
import functools

import numpy as np
import pytest

from oracle import nets as onets
from posepipeline_amd import _lib
from posepipeline_amd.models import synth
from posepipeline_amd.models import videopose3d as vp3d
from posepipeline_amd.program import Net
from posepipeline_amd.wrappers.videopose3d import lift, lift_many

pytestmark = pytest.mark.gpu

CHANNELS = 128
SEG_LISTS = {"mixed": [1, 0, 5, 31, 32, 33, 200], "long": [700]}


def _segments(lengths, seed=5):
    """random-walk tracks; neighbours sit at visibly different offsets (+-0.3 .. +-0.9, alternating sign), so a row that read the
    neighbouring segment instead of its own clamped edge changes the input by far more than anything that could cancel"""
    rng = np.random.default_rng(seed)
    segs = []
    for i, n in enumerate(lengths):
        off = np.float32((0.3 + 0.1 * (i % 7)) * (-1) ** i)
        walk = np.cumsum(rng.normal(0, 0.01, (n, 17, 2)), axis=0).astype(np.float32)
        segs.append(walk + rng.uniform(-0.05, 0.05, (1, 17, 2)).astype(np.float32) + off)
    return segs


def _state_dict(channels=CHANNELS):
    return synth.synth_state_dict(vp3d.videopose3d_param_shapes(vp3d.VideoPose3DSpec(channels=channels)), seed=3)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """per segment: the strided per-window reference on that segment alone (independent of chunk length and batch)"""
    model = onets.VideoPose3DRef(_state_dict())
    pad = vp3d.VideoPose3DSpec(channels=CHANNELS).pad
    return [model.forward(onets.videopose3d_windows(s, pad)) if len(s) else np.zeros((0, 17, 3), np.float32)
            for s in _segments(SEG_LISTS[name])]


@pytest.mark.parametrize("max_batch", [1, 2, 4])
@pytest.mark.parametrize("chunk", [32, 243])
@pytest.mark.parametrize("name", list(SEG_LISTS))
def test_lift_many_equals_the_oracle_per_segment(ctx, name, chunk, max_batch):
    spec = vp3d.VideoPose3DSpec(channels=CHANNELS, chunk=chunk)
    net = Net(ctx, vp3d.build_videopose3d_program(spec, _state_dict()), max_batch=max_batch)
    assert net.numerics == "exact"
    segs = _segments(SEG_LISTS[name])
    got = lift_many(net, spec, segs)
    ref = _oracle(name)
    assert len(got) == len(segs)
    for i, (g, r, s) in enumerate(zip(got, ref, segs)):
        assert g.shape == (len(s), 17, 3) and g.dtype == np.float32, i
        if len(s):
            assert np.isfinite(r).all() and np.abs(r).max() > 1e-4
            assert np.array_equal(g, r), (i, len(s), np.abs(g - r).max())
    net.close()


@pytest.mark.parametrize("numerics", ["exact", "split"])
def test_lift_many_equals_the_single_call(ctx, numerics):
    with _lib.default_numerics(numerics):
        nets = [(vp3d.VideoPose3DSpec(channels=CHANNELS, chunk=chunk), mb) for chunk, mb in ((32, 4), (243, 2), (32, 1))]
        nets = [(spec, Net(ctx, vp3d.build_videopose3d_program(spec, _state_dict()), max_batch=mb)) for spec, mb in nets]
    for spec, net in nets:
        assert net.numerics == numerics
        for name in SEG_LISTS:
            segs = _segments(SEG_LISTS[name], seed=11)
            got = lift_many(net, spec, segs)
            assert [len(g) for g in got] == [len(s) for s in segs]
            for i, s in enumerate(segs):
                if len(s) == 0:
                    continue
                one = lift(net, spec, s)
                assert np.array_equal(got[i], one), (numerics, spec.chunk, net.max_batch, name, i, np.abs(got[i] - one).max())
        net.close()


def test_lift_many_full_width_long_track(ctx):
    """the 1024-channel program the cascade runs, one 700-frame track: two chunks of 512 in one batch, against the single call"""
    spec = vp3d.VideoPose3DSpec()
    sd = synth.synth_state_dict(vp3d.videopose3d_param_shapes(spec), seed=3)
    net = Net(ctx, vp3d.build_videopose3d_program(spec, sd), max_batch=2)
    seg = _segments([700], seed=2)
    got = lift_many(net, spec, seg)[0]
    assert np.abs(got).max() > 1e-4 and np.array_equal(got, lift(net, spec, seg[0]))
    net.close()


def test_lift_many_empty_inputs(ctx):
    spec = vp3d.VideoPose3DSpec(channels=CHANNELS, chunk=32)
    net = Net(ctx, vp3d.build_videopose3d_program(spec, _state_dict()), max_batch=2)
    assert lift_many(net, spec, []) == []
    out = lift_many(net, spec, [np.zeros((0, 17, 2), np.float32)] * 3)
    assert [o.shape for o in out] == [(0, 17, 3)] * 3
    net.close()


def test_lift_many_on_device_memory(ctx):
    spec = vp3d.VideoPose3DSpec(channels=CHANNELS, chunk=32)
    net = Net(ctx, vp3d.build_videopose3d_program(spec, _state_dict()), max_batch=4)
    segs = _segments(SEG_LISTS["mixed"], seed=7)
    host = np.concatenate(lift_many(net, spec, segs)).reshape(-1, 51)
    packed = np.ascontiguousarray(np.concatenate(segs).reshape(-1, 34))
    seg = np.array([len(s) for s in segs], np.int32)
    d_in, d_out = ctx.malloc(packed.nbytes), ctx.malloc(host.nbytes)
    try:
        ctx.h2d(d_in, packed)
        ctx.h2d(d_out, np.full_like(host, np.nan))
        _lib.check(ctx.lib.pp_videopose3d_lift_many(net.handle, net.prog.named["input"], net.prog.named["output"], _lib.ptr(d_in),
                                                    _lib.ptr(seg), len(seg), 34, 51, spec.pad, _lib.ptr(d_out), _lib.PP_MEM_DEVICE),
                   "pp_videopose3d_lift_many")
        ctx.synchronize()
        got = np.zeros_like(host)
        ctx.d2h(got, d_out)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    assert np.array_equal(got, host)
    net.close()


def test_lift_many_scalar_gather_on_a_4_byte_aligned_source(ctx):
    """lift_gather_kernel<float> runs only when a pointer is not 8-byte aligned (2 J features are always even): a device source 4
    bytes into its allocation must give the bytes of the aligned call (float2 gather)"""
    spec = vp3d.VideoPose3DSpec(channels=CHANNELS, chunk=32)
    net = Net(ctx, vp3d.build_videopose3d_program(spec, _state_dict()), max_batch=2)
    segs = _segments([1, 5, 33], seed=9)
    packed = np.ascontiguousarray(np.concatenate(segs).reshape(-1, 34))
    seg = np.array([len(s) for s in segs], np.int32)
    d_in, d_out = ctx.malloc(packed.nbytes + 8), ctx.malloc(len(packed) * 51 * 4)
    assert d_in % 8 == 0
    got = []
    try:
        for off in (0, 4):
            ctx.h2d(d_in + off, packed)
            ctx.h2d(d_out, np.full((len(packed), 51), np.nan, np.float32))
            _lib.check(ctx.lib.pp_videopose3d_lift_many(net.handle, net.prog.named["input"], net.prog.named["output"], _lib.ptr(d_in + off),
                                                        _lib.ptr(seg), len(seg), 34, 51, spec.pad, _lib.ptr(d_out), _lib.PP_MEM_DEVICE),
                       "pp_videopose3d_lift_many")
            ctx.synchronize()
            got.append(np.zeros((len(packed), 51), np.float32))
            ctx.d2h(got[-1], d_out)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 1e-4
    assert np.array_equal(got[1], got[0])
    net.close()


def test_lift_many_rejects_a_bad_mem_and_a_wrong_program(ctx):
    spec = vp3d.VideoPose3DSpec(channels=CHANNELS, chunk=32)
    net = Net(ctx, vp3d.build_videopose3d_program(spec, _state_dict()), max_batch=1)
    x, out, seg = np.zeros((4, 34), np.float32), np.zeros((4, 51), np.float32), np.array([4], np.int32)
    call = lambda pad, mem, s=seg: ctx.lib.pp_videopose3d_lift_many(net.handle, net.prog.named["input"], net.prog.named["output"], _lib.ptr(x),
                                                                    _lib.ptr(s), 1, 34, 51, pad, _lib.ptr(out), mem)
    assert call(spec.pad, 7) != 0 and "pp_videopose3d_lift_many: mem" in _lib.last_error()
    assert call(spec.pad + 1, _lib.PP_MEM_HOST) != 0 and "pp_videopose3d_lift_many: program shape" in _lib.last_error()
    assert call(spec.pad, _lib.PP_MEM_HOST, np.array([-4], np.int32)) != 0 and "pp_videopose3d_lift_many: bad dims" in _lib.last_error()
    assert call(spec.pad, _lib.PP_MEM_HOST) == 0
    net.close()


# ---- the cascade: batched_lift=True (default) against batched_lift=False ------------------------------------------------------------
H, W, N, CHUNK = 135, 240, 136, 8


def _clip():
    rng = np.random.default_rng(23)
    boxes = [(12, 20, 62, 120), (95, 12, 145, 118), (175, 25, 228, 125)]           # three separated persons
    base = rng.integers(0, 60, (H, W, 3)).astype(np.uint8)
    frames, gt = [], []
    for t in range(N):
        img, rows = base.copy(), []
        for p, (x1, y1, x2, y2) in enumerate(boxes):
            dx = (t % 16) // 4 * (1 if p != 1 else -1)
            if p == 2 and 40 <= t < 44:
                continue                       # person 2 missed for four frames: its id ends mid-clip, a new one starts
            if p == 1 and t >= 100:
                continue                       # person 1 leaves: its stream is finalised (and lifted) before the end of the clip
            img[y1:y2, x1 + dx:x2 + dx] = rng.integers(120, 255, (y2 - y1, x2 - x1, 3))
            rows.append([x1 + dx, y1, x2 + dx, y2, 0.9 - 0.05 * p])
        frames.append(img)
        gt.append(np.array(rows, np.float32).reshape(-1, 5))
    return np.stack(frames), gt


def _run_cascade(ctx, numerics, batched, sds, frames, gt):
    from posepipeline_amd.cascade import Cascade, collect
    det_sd, spec, pose_sd, lift_sd = sds
    kw = {} if batched else {"batched_lift": False}                                   # True is the default
    with _lib.default_numerics(numerics):
        cas = Cascade(ctx, det_sd, pose_sd, lift_sd, H, W, chunk=CHUNK, max_persons=3, pose_spec=spec, **kw)
    assert cas.lift_net.numerics == numerics and cas.batched_lift == batched
    assert (cas.persons.lift_many_fn is not None) == batched
    calls = {"many": [], "single": 0}
    many_fn, single_fn = cas.persons.lift_many_fn, cas.persons.lift_fn

    def count_many(kns):
        calls["many"].append(len(kns))
        return many_fn(kns)

    def count_single(kn):
        calls["single"] += 1
        return single_fn(kn)

    if batched:
        cas.persons.lift_many_fn = count_many
    cas.persons.lift_fn = count_single
    outs = [cas.step(frames[i:i + CHUNK], replay=gt[i:i + CHUNK]) for i in range(0, N, CHUNK)] + [cas.flush()]
    ids = [[r[0] for r in fr] for o in outs for fr in o["tracks"]]
    res = (ids, collect(outs, "keypoints"), collect(outs, "keypoints_3d"))
    cas.release()
    return res, calls, len(outs)


@pytest.mark.parametrize("numerics", ["exact", "split"])
def test_cascade_batched_lift_equals_per_person_lift(ctx, numerics):
    from tests.test_gpu_sharded import _state_dicts
    sds = _state_dicts(0)
    frames, gt = _clip()
    (ids_b, k2_b, k3_b), calls_b, n_adv = _run_cascade(ctx, numerics, True, sds, frames, gt)
    (ids_s, k2_s, k3_s), calls_s, _ = _run_cascade(ctx, numerics, False, sds, frames, gt)
    # the batched cascade never reaches the single-track entry, and lifts at most once per step
    assert calls_b["single"] == 0 and 0 < len(calls_b["many"]) <= n_adv
    assert max(calls_b["many"]) >= 2                                   # several persons in one call
    assert calls_s["many"] == [] and calls_s["single"] == sum(calls_b["many"])
    assert ids_b == ids_s and sum(len(i) for i in ids_b) > 2 * N
    assert sorted(k3_b) == sorted(k3_s) and len(k3_b) >= 4            # three persons, one of them under two ids
    assert sum(len(a) for _, a in k3_b.values()) > 2 * N
    for k_b, k_s in ((k2_b, k2_s), (k3_b, k3_s)):
        for tid in k_s:
            assert k_b[tid][0] == k_s[tid][0]
            assert np.array_equal(k_b[tid][1], k_s[tid][1]), (numerics, tid)
    assert all(np.isfinite(a).all() and np.abs(a).max() > 0 for _, a in k3_b.values())
