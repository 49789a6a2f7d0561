"""State that one run leaves behind for the next: every assertion is a bit-equality, a refusal with its message, or a count.

  A  pp_net_input_amax promises and graph replay (csrc/net.hip).  A promise is one-shot, and a replay of a captured graph is a run:
     it consumes the promise, so the next eager run (another batch, an op range) takes the maxima of the input it is given.  Whether
     a graph takes the maxima itself is fixed when it is captured (include/posepipe_hip.h).  The reference is a second net of the same
     program that is never captured and never promised: a sample depends neither on the run before nor on its batch
     (tests/test_gpu_amax.py A, B), so `==` is the claim.
  B  pp_detector_margins between pp_detector_enqueue and pp_detector_collect (csrc/detector.hip): refused, like pp_detector_regress;
     the margins of a pass are published by its collect.
  C  the certified cascade's partial re-run (cascade.py, _det_job_certified): the frames the margins do not certify go through the
     float32-MFMA detector (gathered on the device or on the host) and are spliced back; the others keep the fast detector's rows;
     the keep-everything branch; the exact-only policy with its probe every 8th chunk; real thresholds on real margins.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.cascade import CERTIFY_EPS, Cascade
from posepipeline_amd.models import faster_rcnn as fr
from posepipeline_amd.models import synth
from posepipeline_amd.program import Net, ProgramBuilder
from tests.test_gpu_cascade import _setup
from tests.test_gpu_detector import synth_frame

pytestmark = pytest.mark.gpu

F32 = np.float32
H, W = 135, 240


# ---- A: promises and graph replay -------------------------------------------------------------------------------------------------
def _program():
    rng = np.random.default_rng(7)
    pb = ProgramBuilder()
    x = pb.buf(12, 20, 16, name="input")
    w = (rng.standard_normal((32, 16, 3, 3)) / np.sqrt(16 * 9)).astype(F32)
    y = pb.conv(x, w, None, pad=1, out=pb.buf(12, 20, 32, name="output"), name="reader")
    pb.maxpool(y, 1, 1, 0, name="tail")       # a 1x1 tail: run(n, 0, 1) + run(n, 1, None) is the program in two ranges
    return pb.build()


def _split_net(ctx, prog):
    net = Net(ctx, prog, max_batch=3, numerics="split")
    if net.split_kind != "split_f16":
        pytest.skip("the per-sample activation scale belongs to the fp16 form")
    assert net.conv_kinds()[0] == 2, net.conv_kinds()      # without this the cases test nothing
    return net


@pytest.fixture(scope="module")
def amax(ctx):
    """the program, x_a ~ N(0, 1), x_b = 2^20 x_a (exact), and the reference outputs -- from a net that is never captured and never
    promised, at the batch the case runs"""
    prog = _program()
    x_a = np.random.default_rng(8).standard_normal((3, 12, 20, 16)).astype(F32)
    x_b = x_a * F32(2.0 ** 20)
    assert np.array_equal(x_b.astype(np.float64), x_a.astype(np.float64) * 2.0 ** 20)
    ref_net = _split_net(ctx, prog)
    ref = {(k, n): ref_net.forward(x[:n]) for k, x in (("a", x_a), ("b", x_b)) for n in (2, 3)}
    for y in ref.values():
        assert np.isfinite(y).all() and np.abs(y).max() > 0
    # the two magnitudes are told apart by the bits: a stale maximum cannot pass as the right one
    assert not np.array_equal(ref["b", 2], ref["a", 2])
    return prog, x_a, x_b, ref


def _upload(ctx, net, x):
    ctx.h2d(net.buffer("input")[0], x)


def _promise(ctx, net, x=None):
    """pp_net_input_amax for "input"; x given: the caller's array filled with the true per-sample max |x| (uint32 bit patterns)"""
    p = C.c_void_p()
    L.check(ctx.lib.pp_net_input_amax(net.handle, net.prog.named["input"], C.byref(p)), "pp_net_input_amax")
    assert p.value, "no fp16-form convolution reads the input: the case tests nothing"
    if x is not None:
        _fill(ctx, p.value, x)
    return int(p.value)


def _fill(ctx, dptr, x):
    m = np.abs(x).reshape(x.shape[0], -1).max(axis=1).astype(F32)
    ctx.h2d(dptr, m.view(np.uint32))


def _report(case, y, want):
    """printed before the assertion: how many values are non-finite, and how far the finite ones are from the reference"""
    ok = np.isfinite(y)
    dev = float(np.abs(y[ok].astype(np.float64) - want[ok]).max(initial=0.0) / np.abs(want).max())
    print(f"[run state {case}] {int((~ok).sum())} of {y.size} values non-finite, the others within {dev:.2e} of the reference's range, "
          f"{int((y != want).sum())} differ in their bits")


def _replay_under_a_promise(ctx, net, x):
    """capture(3) with no promise, then a promised replay on x"""
    net.capture(3)
    _upload(ctx, net, x)
    _promise(ctx, net, x)
    net.run(3)


def test_a1_replay_then_a_smaller_batch(ctx, amax):
    prog, x_a, x_b, ref = amax
    net = _split_net(ctx, prog)
    _replay_under_a_promise(ctx, net, x_a)
    assert np.array_equal(net.read("output", 3), ref["a", 3]), "the promised replay itself"
    _upload(ctx, net, x_b[:2])
    net.run(2)                                  # eager, no new promise: it must take the maxima of x_b itself
    y = net.read("output", 2)
    _report("A1", y, ref["b", 2])
    assert np.isfinite(y).all(), "x_b scaled by x_a's maxima left the float16 range"
    assert np.array_equal(y, ref["b", 2])


def test_a2_replay_then_an_op_range(ctx, amax):
    prog, x_a, x_b, ref = amax
    net = _split_net(ctx, prog)
    _replay_under_a_promise(ctx, net, x_a)
    _upload(ctx, net, x_b)
    net.run(3, 0, 1)
    net.run(3, 1, None)
    y = net.read("output", 3)
    _report("A2", y, ref["b", 3])
    assert np.isfinite(y).all()
    assert np.array_equal(y, ref["b", 3])


def test_a3_large_then_small(ctx, amax):
    """a stale LARGE maximum costs precision, not finiteness: only the bits tell (without the fix: every value finite, 98 % of them
    with other bits, up to 2e-6 of the range away -- DESIGN_LOG.md 5s)"""
    prog, x_a, x_b, ref = amax
    net = _split_net(ctx, prog)
    _replay_under_a_promise(ctx, net, x_b)
    assert np.array_equal(net.read("output", 3), ref["b", 3]), "the promised replay itself"
    _upload(ctx, net, x_a[:2])
    net.run(2)
    y = net.read("output", 2)
    _report("A3", y, ref["a", 2])
    assert np.array_equal(y, ref["a", 2])


def test_a4_capture_made_under_a_promise(ctx, amax):
    """the graph holds no maxima pass: every replay reads the caller's array as it stands (include/posepipe_hip.h)"""
    prog, x_a, x_b, ref = amax
    net = _split_net(ctx, prog)
    slot = _promise(ctx, net)
    net.capture(3)
    for k, x in (("a", x_a), ("b", x_b)):
        _upload(ctx, net, x)
        _fill(ctx, slot, x)
        net.run(3)
        assert np.array_equal(net.read("output", 3), ref[k, 3]), k
    # an eager run with no promise takes its own maxima (the array still holds x_b's)
    _upload(ctx, net, x_a[:2])
    net.run(2)
    assert np.array_equal(net.read("output", 2), ref["a", 2])


def test_a5_forward_after_a_promise_and_a_replay_voids_the_promise(ctx, amax):
    prog, x_a, x_b, ref = amax
    net = _split_net(ctx, prog)
    _replay_under_a_promise(ctx, net, x_a)
    assert np.array_equal(net.forward(x_b[:2]), ref["b", 2])        # eager
    _promise(ctx, net, x_a)                                          # a promise about what forward is about to overwrite
    assert np.array_equal(net.forward(x_b), ref["b", 3])            # the replay
    _promise(ctx, net, x_a)
    assert np.array_equal(net.forward(x_b[:2]), ref["b", 2])


# ---- B: margins and in-flight passes --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def margins(ctx):
    sd = synth.synth_state_dict(fr.faster_rcnn_param_shapes(), seed=2)
    for k, g in (("detector.rpn_head.rpn_cls.weight", 0.5), ("detector.rpn_head.rpn_reg.weight", 0.1),
                 ("detector.roi_head.bbox_head.fc_reg.weight", 0.2)):       # tamed heads: tests/test_gpu_detector.py::setup
        sd[k] = (sd[k] * g).astype(F32)
    rng = np.random.default_rng(2)
    frames = np.stack([synth_frame(rng, H, W) for _ in range(4)])
    det = fr.Detector(ctx, sd, H, W, max_frames=4, numerics="split")
    det.enable_margins(True)
    det.run(frames[:4])
    m_run = det.margins(4)
    assert m_run.shape == (4, 8) and (m_run >= 0).all()
    assert len({m_run[i].tobytes() for i in range(4)}) == 4, "the frames' margins must differ, or a stale row could pass"
    return det, frames, m_run


@contextlib.contextmanager
def _in_flight(det, frames):
    """a pass enqueued and not collected; collected on the way out whatever happened in between, so a failure stays one failure"""
    det.enqueue(frames)
    try:
        yield
    finally:
        if getattr(det, "_inflight", None) is not None:
            det.collect()


def test_b1_margins_are_refused_while_a_pass_is_in_flight(margins):
    det, frames, m_run = margins
    det.run(frames[:4])
    assert np.array_equal(det.margins(4), m_run)
    with _in_flight(det, frames[:4]):
        with pytest.raises(L.PosePipeHipError, match="in flight"):
            det.margins(4)
        det.collect()
        assert np.array_equal(det.margins(4), m_run)


def test_b2_margins_after_a_shorter_pass(margins):
    det, frames, m_run = margins
    det.run(frames[:4])
    with _in_flight(det, frames[:2]):
        # not the 4 frames of the pass before as stale data, and not a count mismatch that happens to refuse
        with pytest.raises(L.PosePipeHipError, match="in flight"):
            det.margins(4)
        with pytest.raises(L.PosePipeHipError, match="in flight"):
            det.margins(2)
        det.collect()
        assert np.array_equal(det.margins(2), m_run[:2])        # the detector is per-frame independent
        with pytest.raises(L.PosePipeHipError, match="the last run had 2 frames, 4 asked for"):
            det.margins(4)


def test_b3_margins_off_then_enqueue_and_collect(margins):
    det, frames, m_run = margins
    det.enable_margins(False)
    try:
        with _in_flight(det, frames[:4]):
            det.collect()
            with pytest.raises(L.PosePipeHipError, match="not enabled"):
                det.margins(4)
    finally:
        det.enable_margins(True)
    # switched on again: nothing is published until a pass has run under the new setting
    with pytest.raises(L.PosePipeHipError, match="the last run had 0 frames"):
        det.margins(4)
    det.run(frames[:4])
    assert np.array_equal(det.margins(4), m_run)


# ---- C: partial certification -----------------------------------------------------------------------------------------------------------
SCORE_WEIGHT = CERTIFY_EPS["rpn_nms"] / (2.0 * CERTIFY_EPS["rpn_cut"])      # what Cascade hands pp_detector_enable_margins
NEVER = {k: -1.0 for k in CERTIFY_EPS}                                       # no margin is <= -1


@pytest.fixture(scope="module")
def cert(ctx):
    """one certified cascade, eight frames (two chunks of 4), and the two references, each from a detector of its own:
    E[i] the float32-MFMA detector's rows, F[i] the fast detector's (margins on, the cascade's score_weight)"""
    det_sd, pose_spec, pose_sd, lift_sd = _setup(H, W)
    rng = np.random.default_rng(6)
    frames = np.stack([synth_frame(rng, H, W) for _ in range(8)])
    det_e = fr.Detector(ctx, det_sd, H, W, max_frames=4, numerics="exact")
    det_f = fr.Detector(ctx, det_sd, H, W, max_frames=4, numerics="split")
    det_f.enable_margins(True, SCORE_WEIGHT)
    E = det_e.run(frames[:4]) + det_e.run(frames[4:])
    Fr = det_f.run(frames[:4]) + det_f.run(frames[4:])
    for d in (det_e, det_f):
        d.close()
    # the splice is visible only where the two detectors' rows differ in their bits
    differ = [not np.array_equal(e, f) for e, f in zip(E, Fr)]
    assert all(differ), differ
    cas = Cascade(ctx, det_sd, pose_sd, lift_sd, H, W, chunk=4, max_persons=1, pose_spec=pose_spec, numerics="split", id_numerics="certified")
    assert cas.detector.net_a.numerics == "split" and cas.detector_exact.net_a.numerics == "exact"
    yield cas, frames, E, Fr
    cas.release()


@pytest.fixture
def cas_state(cert, monkeypatch):
    """the shared cascade with its policy state and counters as after construction, and run counters on both detectors"""
    cas = cert[0]
    cas._exact_only, cas._since_probe = False, 0
    cas.certify_stats = {"frames": 0, "certified": 0, "exact_only_frames": 0}
    runs = {"fast": 0, "exact": 0}
    for key, det in (("fast", cas.detector), ("exact", cas.detector_exact)):
        def counted(*a, _run=det.run, _key=key, **kw):
            runs[_key] += 1
            return _run(*a, **kw)
        monkeypatch.setattr(det, "run", counted)
    return runs


def _force(monkeypatch, cas, subset):
    monkeypatch.setattr(cas, "uncertified_frames", lambda dets, margins: np.array(subset, np.int64))


def _assert_rows(dets, want, what):
    assert len(dets) == len(want)
    for i, (a, b) in enumerate(zip(dets, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: frame {i}"


def _spliced(E, Fr, first, redo, n=4):
    return [E[first + i] if i in redo else Fr[first + i] for i in range(n)]


def test_c1_forced_strict_subset_host_frames(cert, cas_state, monkeypatch):
    cas, frames, E, Fr = cert
    _force(monkeypatch, cas, [1, 2])
    dets, _ = cas._det_job(frames[:4], None)
    _assert_rows(dets, _spliced(E, Fr, 0, {1, 2}), "host frames, redo [1, 2]")
    assert cas.last_certified.tolist() == [True, False, False, True]
    assert cas.certify_stats == {"frames": 4, "certified": 2, "exact_only_frames": 0}
    assert cas._exact_only is False
    assert cas_state == {"fast": 1, "exact": 1}


def test_c2_forced_strict_subset_device_frames(ctx, cert, cas_state, monkeypatch):
    cas, frames, E, Fr = cert
    chunk = np.ascontiguousarray(frames[4:])
    ptr = ctx.malloc(chunk.nbytes)
    try:
        ctx.h2d(ptr, chunk)
        _force(monkeypatch, cas, [1, 2])
        dets, _ = cas._det_job(None, (ptr, 4))
        _assert_rows(dets, _spliced(E, Fr, 4, {1, 2}), "device frames, redo [1, 2]")
        assert cas.last_certified.tolist() == [True, False, False, True]
        assert cas.certify_stats["certified"] == 2 and cas._exact_only is False
        # another subset through the same gather scratch: frame 0 is the exact detector's, not a row left from frames 1 / 2
        _force(monkeypatch, cas, [0])
        dets, _ = cas._det_job(None, (ptr, 4))
        _assert_rows(dets, _spliced(E, Fr, 4, {0}), "device frames, redo [0]")
        assert cas.last_certified.tolist() == [False, True, True, True]
        assert cas.certify_stats == {"frames": 8, "certified": 5, "exact_only_frames": 0}
        assert cas_state == {"fast": 2, "exact": 2}
    finally:
        ctx.synchronize()
        ctx.free(ptr)


def test_c3_nothing_to_redo(cert, cas_state, monkeypatch):
    cas, frames, E, Fr = cert
    monkeypatch.setattr(cas, "certify_eps", dict(NEVER))
    dets, _ = cas._det_job(frames[:4], None)
    _assert_rows(dets, Fr[:4], "every frame certified")
    assert cas.last_certified.tolist() == [True] * 4
    assert cas.certify_stats == {"frames": 4, "certified": 4, "exact_only_frames": 0}
    assert cas._exact_only is False
    assert cas_state == {"fast": 1, "exact": 0}


def test_c4_exact_only_policy_and_its_probe(cert, cas_state, monkeypatch):
    cas, frames, E, Fr = cert
    _force(monkeypatch, cas, [0, 1, 3])
    dets, _ = cas._det_job(frames[:4], None)
    _assert_rows(dets, _spliced(E, Fr, 0, {0, 1, 3}), "redo [0, 1, 3]")
    assert cas._exact_only is True
    assert cas_state == {"fast": 1, "exact": 1} and cas.certify_stats["exact_only_frames"] == 0
    for k in range(8):
        first = 4 * (k % 2)
        dets, _ = cas._det_job(frames[first:first + 4], None)
        _assert_rows(dets, E[first:first + 4], f"exact-only call {k}")
        assert cas.last_certified.tolist() == [False] * 4
        assert cas_state == {"fast": 1, "exact": 2 + k}
    assert cas.certify_stats == {"frames": 36, "certified": 1, "exact_only_frames": 32}
    cas._det_job(frames[:4], None)              # the 9th: the fast pass is probed again
    assert cas_state == {"fast": 2, "exact": 10}
    assert cas.certify_stats == {"frames": 40, "certified": 2, "exact_only_frames": 32}


def test_c5_real_thresholds_on_real_margins(cert, cas_state, monkeypatch):
    """the unpatched uncertified_frames: one margin column's eps between two of the values the frames really have"""
    cas, frames, E, Fr = cert
    names = fr.Detector.MARGIN_NAMES
    best = None                                  # (gap, first frame of the chunk, column, midpoint)
    for first in (0, 4):
        cas.detector.run(frames[first:first + 4])
        m = cas.detector.margins(4)
        assert m.shape == (4, len(names)) and (m >= 0).all()
        for col in range(len(names)):
            v = np.unique(m[np.isfinite(m[:, col]), col].astype(np.float64))
            for lo, hi in zip(v[:-1], v[1:]):
                if best is None or hi - lo > best[0]:
                    best = (hi - lo, first, col, 0.5 * (lo + hi))
    assert best is not None, "no margin column has two distinct finite values on these frames: the case cannot be built from them"
    _, first, col, mid = best
    eps = dict(NEVER)
    eps[names[col]] = mid
    monkeypatch.setattr(cas, "certify_eps", eps)
    fast_dets = cas.detector.run(frames[first:first + 4])
    m = cas.detector.margins(4)
    want = np.flatnonzero(m[:, col].astype(np.float64) <= mid)
    assert 0 < len(want) < 4, (names[col], m[:, col], mid)
    got = cas.uncertified_frames(fast_dets, m)
    assert got.tolist() == want.tolist(), (names[col], m[:, col], mid)
    # ... and through the job: the frames at or below the threshold are the exact detector's, the others the fast one's
    dets, _ = cas._det_job(frames[first:first + 4], None)
    _assert_rows(dets, _spliced(E, Fr, first, set(want.tolist())), f"eps[{names[col]}] = {mid}")
    assert cas.last_certified.tolist() == [i not in set(want.tolist()) for i in range(4)]
    assert cas.certify_stats["certified"] == 4 - len(want)


def test_c6_certified_ids_refuse_blob_fn(ctx):
    """the exact detector of the re-runs is built from det_sd, which blob_fn makes a placeholder on every rank but the source.
    Refused before anything is built: the state dicts are not even looked at."""
    with pytest.raises(ValueError, match="blob_fn"):
        Cascade(ctx, None, None, None, H, W, chunk=4, max_persons=1, numerics="split", id_numerics="certified",
                blob_fn=lambda name, prog: None)


def test_c7_release_closes_the_look_ahead_context(ctx, monkeypatch):
    monkeypatch.delenv("POSEPIPE_OVERLAP_DETECTOR", raising=False)
    det_sd, pose_spec, pose_sd, lift_sd = _setup(H, W)
    cas = Cascade(ctx, det_sd, pose_sd, lift_sd, H, W, chunk=2, max_persons=1, pose_spec=pose_spec, numerics="split",
                  overlap_detector="stream")
    det_ctx = cas.det_ctx
    assert det_ctx is not ctx and det_ctx.handle
    rng = np.random.default_rng(9)
    frames = np.stack([synth_frame(rng, H, W) for _ in range(2)])
    assert len(cas._det_job(frames, None)[0]) == 2          # the context has been used
    cas.release()
    assert det_ctx.handle is None and cas.det_ctx is det_ctx
    assert ctx.handle
    p = ctx.malloc(1 << 16)                                  # the caller's context is untouched
    ctx.h2d(p, np.arange(1 << 14, dtype=np.int32))
    back = np.empty(1 << 14, np.int32)
    ctx.d2h(back, p)
    ctx.free(p)
    assert np.array_equal(back, np.arange(1 << 14, dtype=np.int32))
