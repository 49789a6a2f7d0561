"""The top-K and arg-max selection kernels beyond one workgroup: pp_bottomup_candidates on three tiles, pp_bottomup_refine on two
and three spans, pp_fairmot_decode / pp_trades_decode with more than 256 peaks per frame (several chunks of the rank count, several
rank workgroups, K cutting the list), and the decoders' device-output mode.

The shapes are the smallest that reach these paths and follow kernel constants that are not exported (tests/selection_cases.py
names them: BU_TILE 4096, refine span 8192, rank chunk 256); if those change, the shapes must follow.

What is compared: indices, ranks, values and comparison bits are EXACT against the float64 references (tests/bottomup_ref.py,
tests/fairmot_ref.py, tests/trades_ref.py) -- the heat-maps are written to the device directly, so no arithmetic lies between the
input and a comparison.  Interpolated tags and normalised embeddings follow the project's convention: FACTOR = 4 times the deviation
of the reference's own float32 run from its float64 run, computed here and printed.  The inputs' properties (which tile, span or
chunk holds what; the refine margins) are asserted from the references before anything is compared, as tests/test_selection_cases.py
does without a GPU."""
import ctypes as C

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd import ops
from tests import bottomup_ref as ref
from tests import selection_cases as S
from tests.test_gpu_fairmot import _check

pytestmark = pytest.mark.gpu

FACTOR = 4
K = S.K
f32 = np.float32


def _mapset(ctx, case, f=2, h0=8, w0=12):
    from posepipeline_amd import bottomup as bu
    maps = bu.MapSet(ctx, case["s0"], case["s1"], f, K, (h0, w0), (2 * h0, 2 * w0), case["hr"], case["wr"], np.asarray(ref.FLIP_INDEX), True)
    ctx.h2d(maps.hm, case["hm"])
    return maps


# ---- A. pp_bottomup_candidates ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cand_maps(ctx):
    case = S.candidates_case()
    S.check_candidates_case(case)
    maps = _mapset(ctx, case)
    yield case, maps
    maps.close()


@pytest.mark.parametrize("max_people", S.CAND_MAX_PEOPLE)
def test_candidates_three_tiles(cand_maps, max_people):
    case, maps = cand_maps
    cand = maps.candidates(max_people)
    assert np.array_equal(cand, maps.candidates(max_people))            # run-to-run
    want = S.candidates_expected(max_people)
    tags32 = [ref.top_k(case["hm"][fr].astype(np.float64), case["tags32"][fr], max_people)["tag"] for fr in range(case["f"])]
    err_t = dev_t = 0.0
    for fr in range(case["f"]):
        top = want[fr]
        on = top["val"] > 0
        got = cand[fr]
        assert np.array_equal(got[:, :, 0] > 0, on)
        assert np.array_equal(got[:, :, 7][on], top["ind"][on]) and np.array_equal(got[:, :, 0][on], top["val"][on].astype(f32))
        assert np.array_equal(got[:, :, 1][on], top["x"][on]) and np.array_equal(got[:, :, 2][on], top["y"][on])
        assert np.array_equal(got[:, :, 5][on] > 0, top["by"][on]) and np.array_equal(got[:, :, 6][on] > 0, top["bx"][on])
        assert np.array_equal(got[~on], np.broadcast_to(S.NONE_ROW, got[~on].shape))
        err_t = max(err_t, float(np.abs(got[:, :, 3:5][on] - top["tag"][on]).max()))
        dev_t = max(dev_t, float(np.abs(tags32[fr][on].astype(np.float64) - top["tag"][on]).max()))
    print(f"candidates max_people={max_people}: tags, GPU vs float64 {err_t:.3e}; float32 reference vs float64 {case['dev_t']:.3e} over the "
          f"map, {dev_t:.3e} at the candidates")
    assert case["dev_t"] > 0 and err_t <= FACTOR * case["dev_t"]           # the module's convention: the deviation over the whole map
    # the cases by name, frame 0 (frame 1 holds them in reverse plane order and was compared above)
    m = max_people
    assert np.array_equal(cand[0, 3, :, 7], np.arange(m))                                           # flat plane: indices 0 .. m - 1
    assert np.array_equal(cand[0, 5, :, 7], (S.PAIRS_WANT + [-1] * m)[:m])                           # pairs across the tile boundaries
    assert np.array_equal(cand[1, K - 1 - 5, :, 7], (S.PAIRS_WANT + [-1] * m)[:m])
    assert (cand[0, 4, :, 7] >= 0).sum() == min(m, 7) and (cand[:, 6:K - 6, :, 7] == -1).all()
    if m == 30:
        assert set(cand[0, 0, :, 7].astype(int) // S.BU_TILE) == {0, 1, 2} and (cand[0, 1, :, 7] >= 2 * S.BU_TILE).all()
        assert (cand[0, 2, 5:, 0] == f32(0.5)).all() and (np.diff(cand[0, 2, 5:, 7]) > 0).all()


def test_candidates_refuses_before_any_launch(ctx, cand_maps):
    from posepipeline_amd import bottomup as bu
    case, maps = cand_maps
    before = maps.candidates(30)
    for bad in (0, 65):
        with pytest.raises(L.PosePipeHipError, match=r"max_people %d not in 1 \.\. 64" % bad):
            maps.candidates(bad)
    # 65552 planes of 1 x 1 pixels: more than the 65535 a launch grid's second dimension takes
    f = 65552 // 16
    tiny = bu.MapSet(ctx, np.zeros((2 * f, 32, 1, 1), f32), np.zeros((2 * f, 16, 1, 1), f32), f, 16, (1, 1), (1, 1), 1, 1, np.arange(16), True)
    try:
        with pytest.raises(L.PosePipeHipError, match="65552 planes in one call \\(at most 65535\\)"):
            tiny.candidates(30)
    finally:
        tiny.close()
    ctx.synchronize()
    assert np.array_equal(maps.candidates(30), before)                  # the context is as it was


# ---- B. pp_bottomup_refine -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", S.REFINE_SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_refine_exact_across_spans(ctx, hw):
    """zero tag planes: the score is the heat-map value (mean tag (0, 0)) or the value minus exactly 5 (mean tag (3, 4)), so the
    winner is np.argmax of the plane, the lowest index among equal maxima, with no tolerance; the second, smaller call must show
    nothing of the first (the per-span partial results live in scratch memory both calls use)"""
    case = S.refine_exact_case(hw)
    S.check_refine_exact_case(case)
    maps = _mapset(ctx, case)
    try:
        got = [maps.refine(*call) for call in case["calls"]]
        again = [maps.refine(*call) for call in case["calls"]]
    finally:
        maps.close()
    for call, g, a in zip(case["calls"], got, again):
        want = S.refine_exact_expected(case, call)
        assert g.shape == want.shape and np.array_equal(g, want)
        assert np.array_equal(a, g)
        assert not g[call[2] == 0].any() and (g[call[2] != 0][:, 2] != 0).all()
    span = S.span_len(hw[0] * hw[1])
    winners = (got[0][..., 1] * hw[1] + got[0][..., 0]).astype(int)[case["calls"][0][2] != 0]
    assert set(winners // span) == set(range(S.n_split(hw[0] * hw[1])))          # winners in every span, the last pixel among them
    assert hw[0] * hw[1] - 1 in winners and (got[0][..., 2] < 0).any()


@pytest.mark.parametrize("hw", S.REFINE_SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_refine_by_tag_picks_the_later_span(ctx, hw):
    """two tag regions; the plane's maximum lies in the wrong one, in span 0, the winner of hm - round(distance) in a later span of
    the right one.  Exact against the float64 rule, which holds its margins (asserted first, from the reference alone)."""
    case = S.refine_tag_case(hw)
    scans, dev_h = S.refine_tag_scans(case)
    S.check_refine_tag_case(case, scans, dev_h)
    print(f"refine {hw}: float32 reference vs float64: tags {case['dev_t']:.3e}, scores {dev_h:.3e}; margins: distances "
          f"{10 * 4 * case['dev_t']:.3e} off a rounding step, winners ahead by more than {10 * dev_h:.3e}")
    maps = _mapset(ctx, case)
    try:
        got = maps.refine(case["frames"], case["mean_tag"], case["need"])
        again = maps.refine(case["frames"], case["mean_tag"], case["need"])
    finally:
        maps.close()
    want = S.refine_tag_expected(case, scans)
    assert np.array_equal(got, want) and np.array_equal(again, got)
    assert not got[case["need"] == 0].any() and (got[case["need"] != 0][:, 2] == f32(0.6)).all()


# ---- C. pp_fairmot_decode / pp_trades_decode ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_dev(ctx):
    """the four frames and both decoders' side maps on the device: (peak counts, fairmot pointers, trades pointers)"""
    maps = S.decode_maps()
    counts = S.check_decode_maps(maps)
    arrays = [maps["hm"], *maps["fairmot"], *maps["trades"]]
    dev = [ctx.malloc(a.nbytes) for a in arrays]
    for d, a in zip(dev, arrays):
        ctx.h2d(d, a)
    yield counts, dev[:4], [dev[0]] + dev[4:]
    for d in dev:
        ctx.free(d)


def _assert_decoded(kind, count, k, inds, dets, hm):
    if k > count:
        assert (inds[count:] == -1).all() and not dets[count:].any() and (inds[:count] >= 0).all()
    else:
        assert (inds >= 0).all()
    if kind == "flat":
        assert inds.tolist() == list(range(k))
    if kind == "lattice":
        tied = inds[:count][hm.reshape(-1)[inds[:count]] == S.TIED]
        assert len(tied) == min(60, max(0, k - int((hm.reshape(-1) > S.TIED).sum()))) and (np.diff(tied) > 0).all()
    if kind == "saturated":
        assert (np.diff(inds[:min(k, 300)]) > 0).all() and (dets[:min(k, 300), -1] == 1).all()


@pytest.mark.parametrize("k", S.DECODE_KS)
def test_fairmot_decode_many_peaks(ctx, decode_dev, k):
    counts, dev, _ = decode_dev
    h, w = S.DECODE_HW
    n = len(S.DECODE_FRAMES)
    dets, feats, inds = ops.fairmot_decode(ctx, *dev, n, h, w, k)
    again = ops.fairmot_decode(ctx, *dev, n, h, w, k)                   # the peaks are appended in another order every run
    assert all(np.array_equal(a, b) for a, b in zip((dets, feats, inds), again))
    for f, kind in enumerate(S.DECODE_FRAMES):
        rd, rf64, ri = S.fairmot_expected(f, k)
        _, rf32, _ = S.fairmot_expected(f, k, f32)
        assert inds[f].tolist() == ri.tolist(), kind
        assert np.array_equal(dets[f], rd), kind
        _check(feats[f], rf32, rf64, f"decode {h}x{w} K={k} {kind} embeddings")
        assert not feats[f][ri < 0].any()
        _assert_decoded(kind, counts[f], k, inds[f], dets[f], S.decode_maps()["hm"][f])


@pytest.mark.parametrize("k", S.DECODE_KS)
def test_trades_decode_many_peaks(ctx, decode_dev, k):
    counts, _, dev = decode_dev
    h, w = S.DECODE_HW
    n = len(S.DECODE_FRAMES)
    dets, inds = ops.trades_decode(ctx, *dev, n, h, w, k)
    again = ops.trades_decode(ctx, *dev, n, h, w, k)
    assert np.array_equal(dets, again[0]) and np.array_equal(inds, again[1])
    for f, kind in enumerate(S.DECODE_FRAMES):
        rd, ri = S.trades_expected(f, k)
        assert inds[f].tolist() == ri.tolist(), kind
        assert np.array_equal(dets[f], rd), kind
        _assert_decoded(kind, counts[f], k, inds[f], dets[f], S.decode_maps()["hm"][f])


SENTINEL = -777


def _device_outputs(ctx, shapes_dtypes, call):
    """buffers filled with SENTINEL on the device -> call(pointers) -> synchronise -> the buffers' contents"""
    out = [np.full(shape, SENTINEL, dt) for shape, dt in shapes_dtypes]
    dev = [ctx.malloc(a.nbytes) for a in out]
    try:
        for d, a in zip(dev, out):
            ctx.h2d(d, a)
        call([C.c_void_p(d) for d in dev])
        ctx.synchronize()                                               # the device-output mode returns with the work in flight
        for d, a in zip(dev, out):
            ctx.d2h(a, d)
    finally:
        for d in dev:
            ctx.free(d)
    return out


def test_decoders_device_output_mode(ctx, decode_dev):
    """mem != PP_MEM_HOST: the results are written straight to the caller's device memory, no staging, no synchronise.  The same
    arrays as the host mode, every slot written (none keeps the sentinel)."""
    _, fm, tr = decode_dev
    h, w = S.DECODE_HW
    n, k, dim = len(S.DECODE_FRAMES), 500, 128
    host = ops.fairmot_decode(ctx, *fm, n, h, w, k)
    got = _device_outputs(ctx, [((n, k, 5), f32), ((n, k, dim), f32), ((n, k), np.int32)], lambda o: L.check(ctx.lib.pp_fairmot_decode(
        ctx.handle, *(C.c_void_p(p) for p in fm), n, h, w, k, dim, o[0], o[1], o[2], L.PP_MEM_DEVICE), "pp_fairmot_decode"))
    for a, b, name in zip(got, host, ("dets", "feats", "inds")):
        assert np.array_equal(a, b), name
    for f in range(n):
        assert got[2][f].tolist() == S.fairmot_expected(f, k)[2].tolist() and np.array_equal(got[0][f], S.fairmot_expected(f, k)[0])
    host = ops.trades_decode(ctx, *tr, n, h, w, k)
    got = _device_outputs(ctx, [((n, k, 9), f32), ((n, k), np.int32)], lambda o: L.check(ctx.lib.pp_trades_decode(
        ctx.handle, *(C.c_void_p(p) for p in tr), n, h, w, k, o[0], o[1], L.PP_MEM_DEVICE), "pp_trades_decode"))
    for a, b, name in zip(got, host, ("dets", "inds")):
        assert np.array_equal(a, b), name
    for f in range(n):
        assert got[1][f].tolist() == S.trades_expected(f, k)[1].tolist() and np.array_equal(got[0][f], S.trades_expected(f, k)[0])
