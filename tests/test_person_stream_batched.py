"""`PersonStreams(lift_many_fn=...)`: one lifting call per advance() for every followed person (host logic only, no GPU).

The batched form must hand `lift_many_fn` exactly the contexts the per-person form hands `lift_fn` one by one -- same arrays, same
dtype (the reference's float32 / float64 quirk is per stream), same order -- and stitch the same results: keypoints, keypoints_3d and
their frames are compared with `np.array_equal` against a `PersonStreams` built without the keyword, over seeded multi-track
scenarios (gaps of a retained id, ids dropped mid-clip, more ids than max_persons, the end of the clip) fed in several chunkings.
Also here: the C ABI of the batched entry point as far as it can be checked without a device."""
import ctypes

import numpy as np
import pytest

from posepipeline_amd import _lib
from posepipeline_amd.person_stream import PersonStreams, collect

K = 5
SRC = (480, 640)          # not powers of two: float32 and float64 normalisation differ, so the arithmetic a context was normalised in shows


def fake_topdown(jobs):
    out = []
    for tid, t, box in jobs:
        r = np.zeros((K, 3), np.float32)
        r[:, 0] = np.float32(box[0]) + np.float32(1.7) * np.arange(K, dtype=np.float32) + np.float32(100 * tid)
        r[:, 1] = np.float32(box[1]) + np.float32(box[3]) * np.float32(0.3)
        r[:, 2] = np.float32(t % 89) + np.float32(tid) * np.float32(0.25)
        out.append(r)
    return out


def make_fake_lift(pad):
    def fake_lift(kn):
        """a function of the whole +-pad window of every frame, edge-clamped inside the passed context"""
        n = kn.shape[0]
        p = np.pad(kn.astype(np.float32), ((pad, pad), (0, 0), (0, 0)), mode="edge")
        w = np.stack([p[i:i + 2 * pad + 1] for i in range(n)]).astype(np.float64)
        out = np.zeros((n, K, 3))
        out[:, :, :2] = w.mean(axis=1)
        out[:, :, 2] = w[:, 0, :, 0] - w[:, -1, :, 1] + w[:, pad, :, 0] * w[:, pad, :, 1]
        return out.astype(np.float32)
    return fake_lift


def scenario(rng, n, n_ids):
    """per frame rows (id, x1, y1, x2, y2, score) and live sets.  Every id lives over a span of the clip; inside it the tracker keeps
    the id across missed frames (gaps of 1 .. 5 frames: some within the fills' reach, some not), after it the id is gone for good.
    id 0 is there from frame 0 without a gap (a float32 stream); spans overlap, so with max_persons < n_ids some ids are ignored."""
    spans = [(0, int(rng.integers(n // 2, n - 2)))]
    for _ in range(1, n_ids):
        a = int(rng.integers(0, n - 6))
        spans.append((a, min(n, a + int(rng.integers(5, n)))))
    spans[-1] = (spans[-1][0], n)                                    # one id stays to the end of the clip
    tracks, live = [[] for _ in range(n)], [set() for _ in range(n)]
    for tid, (a, b) in enumerate(spans):
        present = np.ones(b - a, bool)
        if tid > 0:
            for _ in range(int(rng.integers(1, 4))):
                g = int(rng.integers(1, max(b - a - 1, 2)))
                present[g:g + int(rng.integers(1, 6))] = False
            present[0] = present[-1] = True
        for t in range(a, b):
            live[t].add(tid)
            if present[t - a]:
                x, y = float(rng.integers(0, 400)), float(rng.integers(0, 200))
                tracks[t].append((tid, np.float32(x), np.float32(y), np.float32(x + 60), np.float32(y + 150), np.float32(0.9)))
    return tracks, live


def chunkings(rng, n):
    yield [n]
    for c in (1, 3, 8):
        yield [c] * (n // c) + ([n % c] if n % c else [])
    out, left = [], n
    while left:
        c = int(rng.integers(1, min(left, 11) + 1))
        out.append(c)
        left -= c
    yield out


def run(tracks, live, chunks, pad, max_persons, batched):
    """-> (advance() results, per advance(): the contexts lift_fn got, per advance(): the lists lift_many_fn got)"""
    fake_lift = make_fake_lift(pad)
    single, many = [], []

    def lift_fn(kn):
        single[-1].append(kn)
        return fake_lift(kn)

    def lift_many_fn(kns):
        many[-1].append(list(kns))
        return [fake_lift(kn) for kn in kns]

    kw = {"lift_many_fn": lift_many_fn} if batched else {}
    ps = PersonStreams(K, pad, SRC, fake_topdown, lift_fn, max_persons=max_persons, **kw)
    outs, i = [], 0
    for c in list(chunks) + [None]:
        single.append([])
        many.append([])
        if c is None:
            outs.append(ps.advance(final=True))
        else:
            ps.ingest(tracks[i:i + c], live[i:i + c])
            i += c
            outs.append(ps.advance())
    assert i == len(tracks) and not ps.streams
    return outs, single, many


@pytest.mark.parametrize("seed,pad,n,n_ids,max_persons", [(0, 3, 60, 5, 3), (1, 6, 90, 6, 3), (2, 4, 48, 4, 8), (3, 121, 300, 4, 2)])
def test_batched_streams_equal_per_person_streams(seed, pad, n, n_ids, max_persons):
    rng = np.random.default_rng(seed)
    tracks, live = scenario(rng, n, n_ids)
    multi = 0
    for chunks in chunkings(rng, n):
        ref_outs, ref_single, ref_many = run(tracks, live, chunks, pad, max_persons, batched=False)
        outs, single, many = run(tracks, live, chunks, pad, max_persons, batched=True)
        assert all(not m for m in ref_many)
        assert all(not s for s in single), "lift_fn must never be called when lift_many_fn is given"
        assert len(many) == len(ref_single) == len(chunks) + 1
        for got, want in zip(many, ref_single):                      # per advance()
            assert len(got) <= 1, "at most one lift_many_fn call per advance()"
            assert bool(got) == bool(want)                           # ... and none when nothing became computable
            if got:
                assert len(got[0]) == len(want)
                multi += len(want) > 1
                for a, b in zip(got[0], want):                       # the same arrays, in the per-person path's order
                    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
        for what in ("keypoints", "keypoints_3d"):
            a, b = collect(outs, what), collect(ref_outs, what)
            assert sorted(a) == sorted(b) and len(a) >= 2
            for tid in b:
                assert a[tid][0] == b[tid][0] and a[tid][1].dtype == b[tid][1].dtype, (what, tid, chunks)
                assert np.array_equal(a[tid][1], b[tid][1]), (what, tid, chunks)
        # advance() by advance(), not only stitched: the same ids, frames and values come out of the same call
        for o, r in zip(outs, ref_outs):
            for key in o:
                assert list(o[key]) == list(r[key]), key
                for tid in r[key]:
                    assert np.array_equal(o[key][tid], r[key][tid]), (key, tid)
        # both branches of the per-stream float32 / float64 normalisation ran: id 0 has a box in every frame from frame 0 on
        # (float32 arithmetic), a stream that starts later in the clip normalises in float64
        k3 = collect(ref_outs, "keypoints_3d")
        assert k3[0][0] == 0 and any(first > 0 for first, _ in k3.values())
        if max_persons < n_ids:
            followed = set(collect(ref_outs, "keypoints"))
            assert followed < {r[0] for fr in tracks for r in fr}    # more ids than max_persons: some were never followed
    assert multi > 0                                                 # some call carried several persons


def test_nothing_to_lift_means_no_call():
    calls = []
    ps = PersonStreams(K, 4, SRC, fake_topdown, None, lift_many_fn=lambda kns: calls.append(len(kns)) or [make_fake_lift(4)(k) for k in kns])
    ps.ingest([[(0, 1.0, 2.0, 30.0, 60.0, 0.9)]] * 3)
    assert ps.advance()["keypoints_3d"] == {} and calls == []        # nothing is 4 frames old yet
    out = ps.advance(final=True)
    assert calls == [1] and out["keypoints_3d"][0].shape == (3, K, 3)


# ---- the C ABI of the batched entry point, without a device ---------------------------------------------------------------------
def test_lift_many_is_bound_and_exported():
    assert "pp_videopose3d_lift_many" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pp_videopose3d_lift_many")
    res, args = _lib.SIGNATURES["pp_videopose3d_lift_many"]
    assert res is ctypes.c_int and len(args) == 11
    assert _lib.load_library().pp_abi_version() == 10                # one symbol added, nothing altered


def test_lift_many_argument_errors_name_the_function():
    lib = _lib.load_library()
    x, out, seg = np.zeros((4, 34), np.float32), np.zeros((4, 51), np.float32), np.array([4], np.int32)
    rc = lib.pp_videopose3d_lift_many(None, 0, 1, _lib.ptr(x), _lib.ptr(seg), 1, 34, 51, 121, _lib.ptr(out), _lib.PP_MEM_HOST)
    assert rc != 0 and "pp_videopose3d_lift_many" in _lib.last_error()
    with pytest.raises(_lib.PosePipeHipError, match="pp_videopose3d_lift_many"):
        _lib.check(rc, "pp_videopose3d_lift_many")
    # the single-track entry still reports under its own name
    rc = lib.pp_videopose3d_lift(None, 0, 1, _lib.ptr(x), 4, 34, 51, 121, _lib.ptr(out))
    assert rc != 0 and "pp_videopose3d_lift:" in _lib.last_error()
