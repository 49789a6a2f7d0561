"""`PersonStreams(lifter="GastNet")`: the GAST-Net temporal rule as a stream (host logic only, no GPU).

GAST-Net drops a track's invalid frames and lifts the compacted sequence of the valid ones.  For every scenario, fed in steps of 1, 3
and 8 frames, the streamed `keypoints_3d` / `keypoints_valid` of a track must equal -- `np.array_equal` -- the eager chain of
wrappers/gastnet.process_gastnet applied to the stacked 2D rows the stream decided for the whole clip:
h36m_coco_format -> revise_kpts -> normalize_screen_coordinates -> lift_chunks -> zeros at the invalid frames.

The compute stages are stubs: `topdown_fn` returns seeded rows, the lifter is a fixed seeded linear map of each window of 2 pad + 1
valid rows (summed in one fixed order), so every output depends on exactly its window and on nothing else: a window that reads a row
too many, too few, or replicates an edge that is not the end of the track's valid sequence changes the result."""
import numpy as np
import pytest

from posepipeline_amd.models.gastnet import GastNetSpec
from posepipeline_amd.person_stream import PersonStreams, collect
from posepipeline_amd.wrappers import gastnet as W

SPEC = GastNetSpec(channels=16, chunk=8)
PAD = SPEC.pad
SRC = (480, 640)
N = 48
_WM = np.random.default_rng(42).standard_normal((17 * (2 * PAD + 1) * 2, 51))


def stub_forward(batch):
    """(b, 17, chunk + 2 pad, 2) joint-major -> (b, 17, chunk, 3): output frame t = the window [t, t + 2 pad] times a fixed matrix, the
    918 terms of every output added in row order (the same sum whatever chunk or call the window falls into)"""
    b, _, t_in, _ = batch.shape
    out = np.empty((b, 17, t_in - 2 * PAD, 3), np.float32)
    for s in range(b):
        for t in range(t_in - 2 * PAD):
            vec = batch[s, :, t:t + 2 * PAD + 1, :].astype(np.float64).reshape(-1)
            out[s, :, t, :] = (vec[:, None] * _WM).sum(axis=0).reshape(17, 3)
    return out


def stub_lift(x):
    return W.lift_chunks(stub_forward, x, SPEC, flip_augment=False)


def eager(rows2d):
    """process_gastnet's chain on the (n, K, 3) float32 rows of one track -> ((n, 17, 3) float32, (n,) bool)"""
    kpts, scores, valid = W.h36m_coco_format(rows2d[:, :17, :2], rows2d[:, :17, 2])
    kpts = W.revise_kpts(kpts, scores, valid)
    out = np.zeros((len(rows2d), 17, 3), np.float32)
    if len(valid):
        x = W.normalize_screen_coordinates(kpts[valid], w=SRC[1], h=SRC[0]).astype(np.float32)
        out[valid] = stub_lift(x)
    is_valid = np.zeros(len(rows2d), bool)
    is_valid[valid] = True
    return out, is_valid


def make_topdown(k, low):
    """seeded rows per (track, frame); `low`: frames whose COCO right ankle (H36M joint 3) scores below revise_kpts' threshold"""
    def topdown(jobs):
        out = []
        for tid, t, box in jobs:
            rng = np.random.default_rng(1000 * tid + t)
            r = np.empty((k, 3), np.float32)
            r[:, :2] = rng.uniform(10, 400, (k, 2))
            r[:, 2] = rng.uniform(0.5, 1.0, k)
            if t in low:
                r[16, 2] = 0.1
            out.append(r)
        return out
    return topdown


def _present(a, b, holes=()):
    return sorted(set(range(a, b)) - set(holes))


# name -> (joints of the 2D head, {track id: (frames with a box, frames the tracker still holds the id)}, low-score frames)
SCENARIOS = {
    "born_at_5": (17, {0: (_present(5, N), range(5, N))}, ()),
    "gaps_1_to_3": (17, {0: (_present(0, N, [10, 15, 16, 22, 23, 24]), range(0, N))}, ()),       # all filled by bfill / ffill
    "gap_of_6": (17, {0: (_present(0, N, range(20, 26)), range(0, N))}, ()),                      # frames 22, 23 stay invalid
    "ends_10_early": (17, {0: (_present(0, N - 10), range(0, N - 10))}, ()),
    "fewer_than_pad_valid": (17, {0: (_present(3, 10), range(3, 10))}, ()),                       # 7 boxes + 4 filled frames < 13
    "two_persons": (17, {0: (_present(0, N, range(30, 36)), range(0, N)), 1: (_present(9, N - 7), range(9, N - 7))}, ()),
    "low_score_leg": (17, {0: (_present(0, N), range(0, N))}, (4, 5, 17, 30, 47)),
    "head_of_136": (136, {0: (_present(2, N, range(12, 18)), range(2, N))}, (8,)),
}


def _tracks(persons):
    tracks, live = [[] for _ in range(N)], [set() for _ in range(N)]
    for tid, (present, held) in persons.items():
        for t in held:
            live[t].add(tid)
        for t in present:
            x, y = 20.0 + 3 * t + 150 * tid, 30.0 + t
            tracks[t].append((tid, np.float32(x), np.float32(y), np.float32(x + 60), np.float32(y + 150), np.float32(0.9)))
    return tracks, live


def _steps(step):
    return [step] * (N // step) + ([N % step] if N % step else [])


def fake_vp3d(kn):
    """stands in for VideoPose3D: (n, K, 2) -> (n, 17, 3), each row a function of its own frame (the contexts are compared directly)"""
    return np.repeat(kn[:, :17].astype(np.float32).sum(axis=2, keepdims=True), 3, axis=2)


def _stream(name, step, batched=True, stub_lift=stub_lift, **kw):
    k, persons, low = SCENARIOS[name]
    tracks, live = _tracks(persons)
    calls = []

    def lift_many_fn(xs):
        calls[-1].append([np.array(x) for x in xs])
        return [stub_lift(x) for x in xs]

    def lift_fn(x):
        calls[-1].append([np.array(x)])
        return stub_lift(x)

    ps = PersonStreams(k, PAD, SRC, make_topdown(k, set(low)), lift_fn, max_persons=len(persons),
                       lift_many_fn=lift_many_fn if batched else None, **kw)
    outs, i = [], 0
    for c in _steps(step) + [None]:
        calls.append([])
        if c is None:
            outs.append(ps.advance(final=True))
        else:
            ps.ingest(tracks[i:i + c], live[i:i + c])
            i += c
            outs.append(ps.advance())
    assert i == N and not ps.streams
    return outs, calls


@pytest.mark.parametrize("step", [1, 3, 8])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_stream_equals_the_eager_chain(name, step):
    outs, calls = _stream(name, step, lifter="GastNet")
    persons = SCENARIOS[name][1]
    k2, k3, kv = collect(outs, "keypoints"), collect(outs, "keypoints_3d"), collect(outs, "keypoints_valid")
    assert sorted(k2) == sorted(k3) == sorted(kv) == sorted(persons)
    for tid, (present, _) in persons.items():
        first, rows = k2[tid]
        assert first == max(0, present[0] - 2) and rows.dtype == np.float32
        want3, want_valid = eager(rows)
        assert k3[tid][0] == first and kv[tid][0] == first
        assert kv[tid][1].dtype == bool and np.array_equal(kv[tid][1], want_valid), (name, step, tid)
        assert k3[tid][1].shape == want3.shape and np.array_equal(k3[tid][1], want3), (name, step, tid)
        assert want_valid.sum() >= 7 and not k3[tid][1][~want_valid].any() and all(r.any() for r in k3[tid][1][want_valid])
    # one advance() makes at most one lift_many_fn call, with every person's range in it
    assert all(len(c) <= 1 for c in calls) and any(calls)
    for o in outs:
        for tid in o["keypoints_3d"]:
            assert np.array_equal(o["keypoints_3d_frames"][tid], o["keypoints_valid_frames"][tid])
            assert len(o["keypoints_valid"][tid]) == len(o["keypoints_3d"][tid]) == len(o["keypoints_3d_frames"][tid])


def test_scenarios_cover_what_they_name():
    """the 6-frame hole leaves invalid frames inside the track, the shorter holes none; revise_kpts acts; the short track stays short"""
    valid = {}
    for name in SCENARIOS:
        outs, _ = _stream(name, 8, lifter="GastNet")
        valid[name] = collect(outs, "keypoints_valid")
    assert valid["gaps_1_to_3"][0][1].all() and len(valid["gaps_1_to_3"][0][1]) == N
    assert valid["gap_of_6"][0][1].tolist() == [t not in (22, 23) for t in range(N)]
    assert valid["born_at_5"][0][0] == 3 and valid["ends_10_early"][0][1].sum() == N - 10 + 2
    assert valid["fewer_than_pad_valid"][0][1].sum() == 11 < PAD
    assert valid["two_persons"][0][0] == 0 and valid["two_persons"][1][0] == 7
    outs, _ = _stream("low_score_leg", 8, lifter="GastNet")
    rows = collect(outs, "keypoints")[0][1]
    kpts, scores, v = W.h36m_coco_format(rows[:, :17, :2], rows[:, :17, 2])
    assert not np.array_equal(W.revise_kpts(kpts, scores, v), kpts)


def test_latency_is_pad_valid_frames():
    """a valid frame comes out once `pad` further valid frames of its track are decided: with a box in every frame, frame t is emitted
    by the advance() that has decided frame t + pad, and the invalid frames of a hole wait for the valid frames before them"""
    outs, _ = _stream("gap_of_6", 1, lifter="GastNet")
    emitted = 0
    for i, o in enumerate(outs[:-1]):
        n_frames = i + 1                                    # frames ingested so far; the box of the last 2 may still be open
        emitted += len(o["keypoints_3d"].get(0, ()))
        decided = sum(len(f) for oo in outs[:i + 1] for f in oo["keypoints_frames"].values())
        assert decided in (n_frames, n_frames - 1, n_frames - 2)
        valid_decided = decided - sum(1 for t in (22, 23) if t < decided)
        # valid frames emitted = valid decided - pad; the invalid frames 22, 23 follow valid frame 21 at once
        want_valid = max(0, valid_decided - PAD)
        want = want_valid + (2 if want_valid >= 22 else 0)
        assert emitted == want, (i, emitted, want)
    assert emitted + len(outs[-1]["keypoints_3d"][0]) == N


def test_one_call_carries_every_person():
    outs, calls = _stream("two_persons", 8, lifter="GastNet")
    assert max(len(c[0]) for c in calls if c) == 2
    single_outs, single_calls = _stream("two_persons", 8, batched=False, lifter="GastNet")
    assert max(len(c) for c in single_calls) == 2                    # without lift_many_fn: one lift_fn call per person
    assert [[x for call in c for x in call] for c in calls if c] != [] and sum(len(c) for c in single_calls) == sum(len(c[0]) for c in calls if c)
    for what in ("keypoints_3d", "keypoints_valid"):
        a, b = collect(outs, what), collect(single_outs, what)
        for tid in b:
            assert a[tid][0] == b[tid][0] and np.array_equal(a[tid][1], b[tid][1])
    # every context is (n, 17, 2) float32: compacted, converted rows
    assert all(x.dtype == np.float32 and x.shape[1:] == (17, 2) for c in calls for call in c for x in call)


@pytest.mark.parametrize("step", [1, 3, 8])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_videopose3d_streams_are_unchanged(name, step):
    """the default policy, named or not, hands the lifter the same contexts and emits the same dict"""
    ref_outs, ref_calls = _stream(name, step, stub_lift=fake_vp3d)
    outs, calls = _stream(name, step, stub_lift=fake_vp3d, lifter="VideoPose3D")
    assert len(outs) == len(ref_outs)
    for o, r in zip(outs, ref_outs):
        assert set(o) == set(r) == {"keypoints", "keypoints_frames", "keypoints_3d", "keypoints_3d_frames"}
        for key in r:
            assert list(o[key]) == list(r[key]), key
            for tid in r[key]:
                assert o[key][tid].dtype == r[key][tid].dtype and np.array_equal(o[key][tid], r[key][tid]), (key, tid)
    for c, rc in zip(calls, ref_calls):
        assert len(c) == len(rc)
        for a, b in zip(c, rc):
            assert len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))
    k = SCENARIOS[name][0]
    assert all(x.shape[1:] == (k, 2) for c in calls for call in c for x in call)      # VideoPose3D contexts: every joint, zero rows kept


def test_lift_many_entry_is_bound_and_names_itself():
    """the C ABI of the one-call entry, as far as it can be checked without a device"""
    import ctypes

    from posepipeline_amd import _lib
    assert "pp_gastnet_lift_many" in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), "pp_gastnet_lift_many")
    res, args = _lib.SIGNATURES["pp_gastnet_lift_many"]
    assert res is ctypes.c_int and len(args) == 11
    lib = _lib.load_library()
    x, seg, out = np.zeros((4, 17, 2), np.float32), np.array([4], np.int32), np.zeros((4, 17, 3), np.float32)
    rc = lib.pp_gastnet_lift_many(None, 0, 1, _lib.ptr(x), _lib.ptr(seg), 1, PAD, 1, _lib.ptr(W.CAMERA_QUATERNION), _lib.ptr(out),
                                  _lib.PP_MEM_HOST)
    assert rc == -1 and "pp_gastnet_lift_many" in _lib.last_error() and not out.any()
    # the mirror permutation the pack and merge kernels hold as a table
    assert W._MIRROR.tolist() == [0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13]
    assert np.array_equal(W._MIRROR[W._MIRROR], np.arange(17))


def test_unknown_policy_is_refused():
    with pytest.raises(ValueError, match="lifter"):
        PersonStreams(17, PAD, SRC, None, None, lifter="PoseFormer")
    with pytest.raises(ValueError, match="17"):
        PersonStreams(5, PAD, SRC, None, None, lifter="GastNet")
