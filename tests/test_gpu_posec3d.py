"""GPU tests of the SkeletonAction stage: pp_pose_target, pp_gather_samples, the PoseC3D programs and the resident model, against
tests/posec3d_ref.py.

Tolerance of network outputs, as tests/test_gpu_poseformer.py: in each test `dev32` is the largest deviation, on that test's inputs and
weights, of the torch float32 CPU evaluation from the float64 twin; the GPU result must lie within FACTOR = 4 x dev32 of the float64
twin.  The measured ratios are printed and recorded in DESIGN_LOG.md.
pp_pose_target: equality with the float64 formula rounded to float32; where the device's exp differs from numpy's in the last place, the
bound is 4 x the largest deviation of a float32 numpy evaluation of the formula from the float64 one on the same inputs.  The test
prints which of the two it was.
"""
import functools

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd import djshim, pipeline as pl
from posepipeline_amd.models import posec3d as PM
from posepipeline_amd.wrappers import mmaction as W
from tests import posec3d_ref as R

pytestmark = pytest.mark.gpu
FACTOR = 4.0
TINY = PM.PoseC3DSpec(base_channels=8, stage_blocks=(1, 2, 1), clip_len=4, height=16, width=16)
REAL = PM.PoseC3DSpec(clip_len=6, height=32, width=32)
SENTINEL = np.float32(7.25)


def _check(got, ref32, ref64, what):
    dev = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    assert dev > 0, what
    print(f"{what}: GPU vs float64 {err:.3e}, float32-on-CPU vs float64 (dev32) {dev:.3e}, ratio {err / dev:.2f} (bound {FACTOR:g}), "
          f"max |ref| {np.abs(ref64).max():.3g}")
    assert err <= FACTOR * dev, (what, err, dev, err / dev)


# ---- pp_pose_target ------------------------------------------------------------------------------------------------------------------
def _target_cases(h, w):
    """(mu_x, mu_y, score) per (frame, joint): every centre class of the issue, cycled over 3 frames x 17 joints"""
    cx, cy = w / 2 + 0.3, h / 2 - 0.2
    centres = [(cx, cy),                                                          # interior
               (0.7, cy), (w - 1.2, cy), (cx, 0.4), (cx, h - 0.9),               # within 3 sigma of each border
               (-2.5, cy), (w + 1.9, cy), (cx, -3.0), (cx, h + 2.2),             # outside on each side: empty patch
               (-1.9, cy), (cx, -1.85),                                           # int() truncates toward zero: int(-0.1) + 1 = 1, one column / row left
               (-2.9, cy), (w + 1.7, cy),                                         # int(-1.1) + 1 = 0: empty; int(w - 0.1) = w - 1: the last column
               (5.0, 7.0), (5.5, 7.5), (0.0, 0.0), (w - 1.0, h - 1.0),           # exactly on a pixel, at .5, the corners
               (1e12, cy), (cx, -1e12)]                                           # far beyond any integer range of the map
    scores = [1.0, 0.37, 1.01e-4, 9.9e-5, 0.0]
    kps = np.zeros((3, 17, 3), np.float64)
    k = 0
    for f in range(3):
        for j in range(17):
            mx, my = centres[k % len(centres)]
            kps[f, j] = (mx, my, scores[(k // len(centres) + (k % 7 == 6)) % len(scores)] if k >= len(centres) else 1.0)
            k += 1
    kps[2, 3] = (cx + 1, cy + 1, 9.9e-5)                                          # just below / just above / zero at an interior centre
    kps[2, 4] = (cx - 1, cy + 2, 1.01e-4)
    kps[2, 5] = (cx, cy, 0.0)
    kps[2, 6] = (cx + 0.25, cy - 0.75, np.float32(0.6180339))                     # a float32 score, as the wrapper passes
    return kps


def _render(ctx, kps, h, w, perm, c_pad, K=17):
    """pp_pose_target into a sentinel-filled buffer -> [2 n][h][w][c_pad]"""
    n = kps.shape[0]
    shape = (2 * n, h, w, c_pad)
    d_kps, d_perm, d_out = ctx.malloc(kps.nbytes), ctx.malloc(perm.nbytes), ctx.malloc(int(np.prod(shape)) * 4)
    try:
        ctx.h2d(d_kps, kps)
        ctx.h2d(d_perm, perm)
        ctx.h2d(d_out, np.full(shape, SENTINEL, np.float32))
        L.check(ctx.lib.pp_pose_target(ctx.handle, L.ptr(d_kps), n, K, h, w, W.SIGMA, L.ptr(d_perm), c_pad, L.ptr(d_out)), "pp_pose_target")
        got = np.empty(shape, np.float32)
        ctx.d2h(got, d_out)
        # argument errors: c_pad not a multiple of 4 / smaller than K, no sample
        for bad in (dict(c_pad=18), dict(c_pad=16), dict(n=0), dict(sigma=0.0)):
            a = {**dict(n=n, c_pad=c_pad, sigma=W.SIGMA), **bad}
            assert ctx.lib.pp_pose_target(ctx.handle, L.ptr(d_kps), a["n"], K, h, w, a["sigma"], L.ptr(d_perm), a["c_pad"], L.ptr(d_out)) != 0
    finally:
        for p in (d_kps, d_perm, d_out):
            ctx.free(p)
    return got


@pytest.mark.parametrize("h,w", [(64, 64), (12, 20)])
def test_pose_target(ctx, h, w):
    kps = _target_cases(h, w)
    n, K, c_pad = kps.shape[0], 17, 20
    perm = W.mirror_perm(K)
    ref64 = R.heatmaps_loop(kps, h, w, perm, c_pad)
    ref32 = R.heatmaps_loop(kps, h, w, perm, c_pad, dtype=np.float32)
    want = ref64.astype(np.float32)
    assert (want[:n] > 0).any(axis=(1, 2)).sum() > 20 and (want[..., K:] == 0).all()
    got = _render(ctx, kps, h, w, perm, c_pad)
    # the mirrored samples are the PLAIN rendering of the flipped key points (x -> w - x where x != 0, joints exchanged): one pixel
    # apart from a mirror image of the plain map, and a key point at x == 0 stays in column 0
    flipped = kps.copy()
    flipped[..., 0] = np.where(kps[..., 0] != 0, w - kps[..., 0], kps[..., 0])
    assert np.array_equal(got[n:], _render(ctx, np.ascontiguousarray(flipped[:, perm]), h, w, perm, c_pad)[:n])
    assert not np.array_equal(got[n:, :, :, :K], got[:n, :, ::-1, :K][..., perm])
    zero_x = [(f, j) for f in range(n) for j in range(K) if kps[f, j, 0] == 0 and kps[f, j, 2] >= 1e-4]
    assert zero_x and all(got[n + f, 0, 0, list(perm).index(j)] > 0 for f, j in zero_x)
    # a permutation entry outside [0, K) reads nothing: that channel of the mirrored samples is zeros, the others are unchanged
    bad_perm = perm.copy()
    bad_perm[3], bad_perm[9] = -1, K
    bad = _render(ctx, kps, h, w, bad_perm, c_pad)
    keep = [c for c in range(c_pad) if c not in (3, 9)]
    assert (bad[n:, :, :, [3, 9]] == 0).all() and np.array_equal(bad[..., keep], got[..., keep]) and np.array_equal(bad[:n], got[:n])
    assert not (got == SENTINEL).any(), "an element was not written"
    assert ((got != 0) == (want != 0)).all(), "the patches' supports differ"
    assert (got[..., K:] == 0).all()
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    dev = float(np.abs(ref32.astype(np.float64) - ref64).max())
    if np.array_equal(got, want):
        print(f"pp_pose_target {h}x{w}: EQUAL to the float64 formula rounded to float32 ({int((want != 0).sum())} non-zero elements)")
    else:
        bad = int((got != want).sum())
        print(f"pp_pose_target {h}x{w}: {bad} elements differ from the rounded float64 formula (device exp vs numpy's); "
              f"error {err:.3e}, float32 evaluation's {dev:.3e}, bound 4 x")
        assert dev > 0 and np.abs(got.astype(np.float64) - ref64).max() <= 4 * dev


# ---- pp_gather_samples ---------------------------------------------------------------------------------------------------------------
def test_gather_samples(ctx):
    rng = np.random.default_rng(3)
    n_src, n, sample = 7, 301, 4 * (2 * 256 + 3)                  # 515 float4s: two full sweeps of a 256-thread block and a tail of 3
    src = rng.standard_normal((n_src, sample)).astype(np.float32)
    idx = rng.integers(0, n_src, n).astype(np.int32)
    idx[:9] = (6, 6, 0, 3, 3, 3, 0, 6, 1)                         # repeats, both ends
    d_src, d_idx, d_dst = ctx.malloc(src.nbytes), ctx.malloc(idx.nbytes), ctx.malloc(n * sample * 4 + 64)
    try:
        ctx.h2d(d_src, src)
        ctx.h2d(d_idx, idx)
        ctx.h2d(d_dst, np.full(n * sample + 16, SENTINEL, np.float32))
        L.check(ctx.lib.pp_gather_samples(ctx.handle, L.ptr(d_src), n_src, L.ptr(d_idx), n, sample, L.ptr(d_dst)), "pp_gather_samples")
        got = np.empty(n * sample + 16, np.float32)
        ctx.d2h(got, d_dst)
        assert np.array_equal(got[:n * sample].reshape(n, sample), src[idx]) and (got[n * sample:] == SENTINEL).all()
        # an index outside [0, n_src) reads nothing: its sample is zeros
        idx2 = np.array([2, -1, n_src, 5], np.int32)
        ctx.h2d(d_idx, idx2)
        L.check(ctx.lib.pp_gather_samples(ctx.handle, L.ptr(d_src), n_src, L.ptr(d_idx), 4, sample, L.ptr(d_dst)), "pp_gather_samples")
        got = np.empty((4, sample), np.float32)
        ctx.d2h(got, d_dst)
        assert np.array_equal(got[[0, 3]], src[[2, 5]]) and (got[1:3] == 0).all()
        for bad in (dict(sample=6), dict(n=0), dict(n=70000), dict(n_src=0)):
            a = {**dict(n=n, sample=sample, n_src=n_src), **bad}
            assert ctx.lib.pp_gather_samples(ctx.handle, L.ptr(d_src), a["n_src"], L.ptr(d_idx), a["n"], a["sample"], L.ptr(d_dst)) != 0
        assert ctx.lib.pp_gather_samples(ctx.handle, L.ptr(d_src + 4), n_src - 1, L.ptr(d_idx), 4, sample, L.ptr(d_dst)) != 0      # alignment
    finally:
        for p in (d_src, d_idx, d_dst):
            ctx.free(p)


# ---- the trunk -----------------------------------------------------------------------------------------------------------------------
def _maps(rng, spec, n_clips):
    """heat-map-like inputs: sparse non-negative blobs, pad channels zero"""
    x = np.zeros((n_clips, spec.clip_len, spec.height, spec.width, spec.c_pad), np.float32)
    body = rng.uniform(0, 1, x.shape[:-1] + (spec.in_channels,)) ** 6
    x[..., :spec.in_channels] = body.astype(np.float32)
    return x


@functools.lru_cache(maxsize=None)
def _case(name):
    spec, n_clips, seed = {"tiny": (TINY, 3, 21), "real": (REAL, 2, 22),
                           # temporal strides: on an inflated stage (T 4 -> 2 at layer3.0); on both later stages, one of them not
                           # inflated (conv1 in the frame view, T 4 -> 2 -> 1)
                           "tiny_ts": (PM.replace(TINY, temporal_strides=(1, 1, 2)), 3, 23),
                           "tiny_ts_mixed": (PM.replace(TINY, inflate=(0, 1, 0), temporal_strides=(1, 2, 2)), 3, 24)}[name]
    sd = PM.synth_params(PM.posec3d_param_shapes(spec), seed)
    x = _maps(np.random.default_rng(seed), spec, n_clips)
    ref64, ref32 = R.logits_ref(spec, sd, x, R.torch.float64), R.logits_ref(spec, sd, x, R.torch.float32)
    for a in (x, ref64, ref32):
        a.setflags(write=False)
    return spec, sd, x, ref64, ref32


def _logit_range(ref64):
    """seeded weights whose logits are O(1): a soft-max over them neither hides an error nor saturates"""
    top, spread = float(np.abs(ref64).max()), float(ref64.max(axis=1).min() - ref64.min(axis=1).max())
    assert 0.5 <= top <= 20 and float(ref64.std()) >= 0.2, (top, spread, float(ref64.std()))


@pytest.mark.parametrize("case", ["tiny", "tiny_ts", "tiny_ts_mixed"])
def test_trunk_tiny(ctx, case):
    """a temporal convolution at t = 0 and t = T - 1 (T = 4), a stride-2 projection block in every stage, both view changes, the head;
    a clip's result does not depend on the clips it shares a batch with"""
    spec, sd, x, ref64, ref32 = _case(case)
    _logit_range(ref64)
    net = PM.PoseC3DNet(ctx, spec, sd, max_clips=3)
    try:
        got = net.forward(x)
        assert got.shape == (3, 81) and got.dtype == np.float32
        _check(got, ref32, ref64, f"trunk {case}, 3 clips")
        for i in range(3):
            assert np.array_equal(net.forward(x[i:i + 1])[0], got[i]), f"clip {i} alone differs from clip {i} in the batch"
        assert np.array_equal(net.forward(x[::-1])[::-1], got)
        # time matters: a clip with two frames exchanged gives another result (the clip view really convolves over t)
        y = x[:1].copy()
        y[0, [0, 3]] = y[0, [3, 0]]
        assert not np.array_equal(net.forward(y)[0], got[0])
    finally:
        net.close()


@pytest.mark.parametrize("numerics", [None, "split"], ids=["suite_numerics", "split"])
def test_trunk_real_widths(ctx, numerics):
    """the default spec's channel widths at T = 6, 32 x 32, 2 clips (about 1.4 GMAC)"""
    spec, sd, x, ref64, ref32 = _case("real")
    _logit_range(ref64)
    net = PM.PoseC3DNet(ctx, spec, sd, numerics=numerics, max_clips=2)
    try:
        for name in ("front", "frame", "clip"):
            nt = net.nets[name]
            kinds = nt.conv_kinds()
            convs = [(i, op) for i, op in enumerate(nt.prog.ops) if op.type == L.PP_OP_CONV]
            print(f"{name}: numerics {nt.numerics} ({nt.split_kind}), conv kinds {[int(kinds[i]) for i, _ in convs]}")
            if numerics == "split":
                assert nt.numerics == "split"
                for i, op in convs:
                    what = (name, nt.prog.op_names[i], op.kh, op.kw, op.stride, op.cin, op.cout)
                    if (op.kh, op.kw) == (3, 1) or op.kh == 7 or nt.prog.op_names[i] == "cls_head.fc_cls":
                        # the split planner takes 3x3, 1x1 and full-cover shapes (conv_split.hip): the temporal convolutions, the 7x7
                        # stem on 20 channels and the 84-channel fc_cls stay on the float32 matrix-core kernels
                        assert kinds[i] == 1, what
                    elif (op.kh, op.kw, op.stride) == (3, 3, 1):
                        assert kinds[i] == 2, what             # every stride-1 3x3 (16 | cin) runs on a split kernel
            else:
                assert all(kinds[i] == 1 for i, _ in convs)
        if numerics == "split":
            assert any((net.nets[n].conv_kinds() == 2).any() for n in ("front", "frame"))
        got = net.forward(x)
        _check(got, ref32, ref64, f"trunk real widths ({net.numerics})")
        assert np.array_equal(net.forward(x), got), "two runs differ"
        assert np.array_equal(net.forward(x[1:])[0], got[1]), "clip 1 alone differs from clip 1 in the batch"
    finally:
        net.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _track(rng, n, h=240, w=320):
    kp = np.zeros((n, 17, 3), np.float32)
    base = np.stack([rng.uniform(90, 210, 17), rng.uniform(40, 200, 17)], axis=1)
    for t in range(n):
        kp[t, :, :2] = base + rng.normal(0, 2, (17, 2)) + t * np.array([2.0, 1.0])
        kp[t, :, 2] = rng.uniform(0.3, 1.0, 17)
    kp[2, 5] = 0.0                                                    # an undetected joint
    return kp


def test_end_to_end_small(ctx):
    """SkeletonActionModel(tiny, 2 clips of 6 frames) on a 12-frame track (5 windows) against the twins chained: sampler, transforms,
    heat-maps, the mirrored clips, network, soft-max and mean.  total_frames = 4 keeps the sampler on the wrapper's branch (fewer
    frames than clip_len); with the wrapper's 10 a 6-frame window cannot be indexed, in the reference either."""
    spec = PM.replace(TINY, clip_len=6)
    sd = PM.synth_params(PM.posec3d_param_shapes(spec), 31)
    kp, shape = _track(np.random.default_rng(31), 12), (240, 320)
    inds = R.sample_frames_loop(4, 6, 2)
    ref = {np.float64: [], np.float32: []}
    logit64 = []
    for start in range(0, 12 - 6 - 1):
        xy, score = R.pipeline_loop(kp[start:start + 6], shape, inds, size=16)
        maps = R.heatmaps_loop(np.concatenate([xy, score[..., None].astype(np.float64)], axis=-1), 16, 16, W.mirror_perm(), spec.c_pad)
        maps = maps.astype(np.float32)                                # the reference's heat-maps are float32 arrays
        clips = np.concatenate([maps[:12].reshape(2, 6, 16, 16, -1), maps[12:].reshape(2, 6, 16, 16, -1)])      # FormatShape
        for dt, tdt in ((np.float64, R.torch.float64), (np.float32, R.torch.float32)):
            lg = R.logits_ref(spec, sd, clips, tdt)
            ref[dt].append(R.average_clips_ref(lg.astype(dt), dt))
            if dt is np.float64:
                logit64.append(lg)
    _logit_range(np.concatenate(logit64))
    ref64, ref32 = np.stack(ref[np.float64]), np.stack(ref[np.float32])
    out = {}
    for dedup in (True, False):
        m = W.SkeletonActionModel(ctx=ctx, state_dict=sd, spec=spec, num_clips=2, clip_len=6, dedup=dedup, total_frames=4)
        try:
            assert m.n_frames == 4 and m.n_clips == 4 and np.array_equal(m.frame_inds, inds)
            got = m.scores(kp, shape)
            assert got.shape == (5, 81) and got.dtype == np.float32 and m.last_timing["windows"] == 5
            _check(got, ref32, ref64, f"end to end small (dedup {dedup})")
            assert np.array_equal(m.scores(kp, shape), got), "two runs differ"
            assert np.array_equal(m.scores(kp, shape, stride=2), got[::2])
            m.timing = True
            assert np.array_equal(m.scores(kp, shape), got)
            assert set(m.last_timing) == {"targets", "front", "gather", "trunk", "head", "total_s", "windows"}
            assert all(m.last_timing[k] > 0 for k in ("targets", "front", "gather", "trunk", "head"))
            assert m.scores(kp[:7], shape).shape == (0, 81)           # 7 - 6 - 1 = 0 windows
            out[dedup] = got
        finally:
            m.close()
    assert np.array_equal(out[True], out[False]), "de-duplicated and plain front stage differ"


def test_end_to_end_full_size(ctx):
    """one window at full size (20 clips of 17 x 48 x 64 x 64) with synthetic weights: dedup on and off agree bit for bit"""
    spec = PM.PoseC3DSpec()
    sd = PM.synth_params(PM.posec3d_param_shapes(spec), 41)
    kp = _track(np.random.default_rng(41), 50)
    out = {}
    for dedup in (True, False):
        m = W.SkeletonActionModel(ctx=ctx, state_dict=sd, spec=spec, dedup=dedup)
        try:
            assert m.n_frames == 10 and m.n_clips == 20 and 1 <= m.clips_per_pass <= 20
            got = m.scores(kp, (240, 320))
            assert got.shape == (1, 81) and got.dtype == np.float32 and np.isfinite(got).all() and (got >= 0).all()
            # "within float32": an entry carries the roundings of exp, the 81-term sum, the division and the 20-term mean, at most about
            # a hundred units in the last place in the worst case: 1e-5 in the sum of entries that add up to 1
            assert abs(float(got[0].astype(np.float64).sum()) - 1) <= 1e-5
            assert 1.5 / 81 < got.max() < 0.99                         # neither flat nor saturated
            out[dedup] = got
        finally:
            m.close()
    assert np.array_equal(out[True], out[False]), "de-duplicated and plain front stage differ"


def test_wrapper_on_the_table_shim(monkeypatch, tmp_path):
    """mmaction_skeleton_action_person through the tables: the reference's keys and shapes for a 52-frame track (3 windows)"""
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    monkeypatch.setattr(W, "_cache", {})
    djshim.reset()
    try:
        key = {a: 1 for a in pl.TopDownPerson.primary_key}
        key.update(video_project="p", filename="v")
        vkey = {a: key[a] for a in pl.VideoInfo.primary_key}
        pl.VideoInfo.insert1({**vkey, "timestamps": [], "delta_time": [], "num_frames": 52, "fps": 30.0, "height": 240, "width": 320})
        pl.TopDownPerson.insert1({**key, "keypoints": _track(np.random.default_rng(7), 52)})
        pl.SkeletonAction.populate(key)
        row = (pl.SkeletonAction & key).fetch1()
        assert row["method"] == "mmaction_skeleton" and row["action_window_len"] == 48 and row["stride"] == 1
        scores = row["action_scores"]
        assert scores.shape == (3, 81) and scores.dtype == np.float32 and np.abs(scores.sum(axis=1) - 1).max() < 1e-5
        assert row["label_map"] == {i: f"class_{i}" for i in range(1, 81)}
        assert len(row["top5"]) == 3
        for t5, p in zip(row["top5"], scores):
            assert len(t5) == 5 and [float(s) for _, s in t5] == [float(v) for v in np.sort(p)[::-1][:5]]
            idx = [int(np.flatnonzero(p == s)[0]) for _, s in t5]
            assert [name for name, _ in t5] == [f"class_{i}" if i else "0" for i in idx]
        # windows 0 .. 2 read frames 0 .. 9, 1 .. 10, 2 .. 11: three different results
        assert not np.array_equal(scores[0], scores[1]) and not np.array_equal(scores[1], scores[2])
    finally:
        for m, _ in W._cache.values():
            m.close()
        djshim.reset()
