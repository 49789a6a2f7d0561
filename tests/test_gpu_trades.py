"""TraDeS stage on the GPU against tests/trades_ref.py.

Tolerances follow the project's convention (tests/test_gpu_fairmot.py): a GPU result is compared with the FLOAT64 reference, and the
bound is FACTOR = 4 times the deviation of the same reference evaluated in float32 on the CPU from float64.  The deviation is
computed here from the reference alone and asserted positive; the observed ratios are printed.  Selections and data movement (the
decode's indices and boxes, the difference, the broadcast product, the zero set of the pre-heat-map, the unit mask) are bit-equal."""
import os

import numpy as np
import pytest

from posepipeline_amd import ops
from posepipeline_amd.models import trades as T
from posepipeline_amd.program import Net
from tests import fairmot_ref as F
from tests import trades_ref as R

pytestmark = pytest.mark.gpu
FACTOR = 4.0
f32 = np.float32


def _check(got, ref32, ref64, what):
    dev = float(np.abs(ref32.astype(np.float64) - ref64).max())
    assert dev > 0, what
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{what}: GPU error {err:.3e}, float32-on-CPU deviation {dev:.3e}, ratio {err / dev:.2f}")
    assert err <= FACTOR * dev, (what, err, dev)
    return err / dev


def _check_stored(got, ref32, ref64, what):
    """end-to-end quantities, which both chains STORE as float32: the plain FACTOR rule; where the float32 chain's stored values equal
    the float64 chain's (measured deviation 0) the rule demands equality, and equality is asserted"""
    dev = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{what}: GPU error {err:.3e}, float32-on-CPU deviation {dev:.3e}")
    if dev == 0:
        assert np.array_equal(got.astype(np.float64), ref64), (what, err)
    else:
        assert err <= FACTOR * dev, (what, err, dev)


# ---- pp_trades_cva ----------------------------------------------------------------------------------------------------------------------
def _cva_refs(cur, prev):
    r64 = [R.cva(c, p, np.float64) for c, p in zip(cur, prev)]
    r32 = [R.cva(c, p, np.float32) for c, p in zip(cur, prev)]
    return [np.stack([r[k] for r in r64]) for k in range(3)], [np.stack([r[k] for r in r32]) for k in range(3)]


@pytest.mark.parametrize("hc,wc", [(5, 7), (20, 28), (9, 33)])
def test_cva_against_float64(ctx, hc, wc):
    """batch 2 (the pair stride); P and wc are no multiples of the 32-query / 128-key tiles, (20, 28) and (9, 33) take several of both"""
    rng = np.random.default_rng(hc * 100 + wc)
    cur, prev = (rng.standard_normal((2, hc, wc, 128)) * 0.2).astype(f32), (rng.standard_normal((2, hc, wc, 128)) * 0.2).astype(f32)
    (off64, sh64, sw64), (off32, sh32, sw32) = _cva_refs(cur, prev)
    for s, n in ((sh64, hc), (sw64, wc)):                     # neither flat nor one-hot
        ent = R.entropy(s) / np.log(n)
        print(f"cva {hc}x{wc}: softmax entropy / log n in [{ent.min():.3f}, {ent.max():.3f}]")
        assert 0.05 < ent.min() and ent.max() < 0.995
    span = 5 * np.ptp(R.cva(cur[0], prev[0])[3], axis=1)
    assert 1.0 < np.median(span) < 20.0                       # 5 c spans a few units
    off, sh, sw = ops.trades_cva(ctx, cur, prev, want_soft=True)
    again = ops.trades_cva(ctx, cur, prev, want_soft=True)
    assert all(np.array_equal(a, b) for a, b in zip((off, sh, sw), again)), "two runs differ"
    _check(sh, sh32, sh64, f"cva {hc}x{wc} softmax over rows")
    _check(sw, sw32, sw64, f"cva {hc}x{wc} softmax over columns")
    _check(off, off32, off64, f"cva {hc}x{wc} tracking_offset")
    off_only, _, _ = ops.trades_cva(ctx, cur, prev)
    assert np.array_equal(off_only, off)


def test_cva_maximum_in_the_last_row_and_column_and_padding_ignored(ctx):
    """Pair 0: every query's best key is the LAST cell (last valid row and column); the embeddings are small integers / 4, so every
    product and sum is exact in float32 and the maxima have one correct value.  Pair 1's keys -- what lies behind pair 0's P keys
    in memory, i.e. what a staging tile reads past the end -- are 1000 times larger: a padded key that entered a maximum would win it."""
    hc, wc = 9, 33
    rng = np.random.default_rng(5)
    cur = (rng.integers(-2, 3, (2, hc, wc, 128)) / 4).astype(f32)
    prev = (rng.integers(-2, 3, (2, hc, wc, 128)) / 4).astype(f32)
    cur[0, ..., :32] = 0.5                       # a component every query shares ...
    prev[0] *= f32(0.25)
    prev[0, -1, -1] = 0
    prev[0, -1, -1, :32] = 0.125                 # ... and only the last cell answers: c = 2 there, |c| < 1.5 elsewhere
    prev[1] *= f32(1000)
    (off64, sh64, sw64), (off32, sh32, sw32) = _cva_refs(cur, prev)
    _, _, _, ch64, cw64 = R.cva(cur[0], prev[0], np.float64)
    _, _, _, ch32, cw32 = R.cva(cur[0], prev[0], np.float32)
    assert np.array_equal(ch64, ch32) and np.array_equal(cw64, cw32)            # exact in float32
    assert (ch64.argmax(1) == hc - 1).all() and (cw64.argmax(1) == wc - 1).all() and ch64.max() == 2.0
    off, sh, sw = ops.trades_cva(ctx, cur, prev, want_soft=True)
    assert np.array_equal(sh[0].argmax(1), sh64[0].argmax(1)) and np.array_equal(sw[0].argmax(1), sw64[0].argmax(1))
    # with exact maxima the softmax differs from the float32 evaluation only in exp and the sums
    _check(sh, sh32, sh64, "cva last-cell softmax over rows")
    _check(sw, sw32, sw64, "cva last-cell softmax over columns")
    _check(off, off32, off64, "cva last-cell tracking_offset")
    # THIS IS THE EXACTNESS ASSERTION for the maxima (the kernel has no maxima output): p_k / p_max = exp(5 (ch_k - m)); 5 (ch_k - m) is
    # exact here, so the GPU's ratio must equal the quotient of the two correctly rounded exponentials up to the two divisions'
    # roundings (4 ulp); a maximum that was off by one step of the inputs' grid (1 / 64), let alone a padded key 1000 times larger,
    # changes the ratio by a factor exp(5 / 64)
    m = ch64.max(1, keepdims=True)
    want = np.exp(5 * (ch64 - m))
    got = sh[0].astype(np.float64) / sh[0].max(1, keepdims=True)
    keep = want > 1e-30
    assert np.abs(got[keep] / want[keep] - 1).max() < 4 * 2.0 ** -23


def test_cva_shift_gives_nearest_x2_offsets_in_w_h_order(ctx):
    """prev = cur shifted by (+2 rows, -3 columns), near-orthogonal embeddings: every interior query finds itself 2 rows down and 3
    columns left, so tracking_offset = (2 * -3, 2 * +2) = (-6, +4) in (w, h) order, constant over each 2 x 2 block"""
    hc, wc = 12, 20
    rng = np.random.default_rng(12)
    v = rng.standard_normal((hc, wc, 128))
    cur = (v / np.linalg.norm(v, axis=-1, keepdims=True) * np.sqrt(8)).astype(f32)
    u = rng.standard_normal((hc, wc, 128))
    prev = (u / np.linalg.norm(u, axis=-1, keepdims=True) * np.sqrt(8)).astype(f32)
    prev[2:, :wc - 3] = cur[:hc - 2, 3:]
    off64 = R.cva(cur, prev, np.float64)[0]
    off32 = R.cva(cur, prev, np.float32)[0]
    off, _, _ = ops.trades_cva(ctx, cur[None], prev[None])
    _check(off[0], off32, off64, "cva shifted pair")
    cells = off[0].reshape(hc, 2, wc, 2, 2)
    assert np.array_equal(cells[:, 0, :, 0], cells[:, 1, :, 1]) and np.array_equal(cells[:, 0, :, 0], cells[:, 0, :, 1]) \
        and np.array_equal(cells[:, 0, :, 0], cells[:, 1, :, 0])
    interior = cells[:hc - 2, 0, 3:, 0]
    assert np.abs(interior[..., 0] + 6).max() < 1e-3 and np.abs(interior[..., 1] - 4).max() < 1e-3


# ---- pp_trades_render_prehm ----------------------------------------------------------------------------------------------------------------
IDENTITY = np.array([[1.0, 0, 0], [0, 1.0, 0]])


def test_render_prehm(ctx):
    hp, wp = 64, 96
    src = np.array([[20, 10, 60, 40], [-10, -8, 30, 22], [50, 30, 50, 45],      # ordinary; clipped to the input; zero width: skipped
                    [70, 5, 71, 6], [60, 40, 130, 90]], f32)                      # radius 0; clipped at the bottom-right corner
    from_boxes = T.prehm_boxes(src, IDENTITY, hp, wp)
    want = []
    for b in src:
        cb = b.copy()
        cb[[0, 2]], cb[[1, 3]] = np.clip(cb[[0, 2]], 0, wp - 1), np.clip(cb[[1, 3]], 0, hp - 1)
        want.append(R.radius_centre(cb))
    assert from_boxes.tolist() == [list(b) for b in want if b is not None] and len(from_boxes) == len(src) - 1
    assert (from_boxes[:, 2] == 0).any() and (from_boxes[:, 2] >= 3).any()
    explicit = np.array([[40, 25, 9], [46, 28, 9],                              # overlapping: max, not sum
                         [2, 3, 6], [94, 62, 7], [50, 0, 5], [0, 30, 4], [95, 40, 3], [48, 63, 5]], np.int32)      # clipped at each border
    boxes = np.concatenate([explicit, from_boxes]).astype(np.int32)
    ref64, ref32 = R.render_prehm(boxes, hp, wp, np.float64), R.render_prehm(boxes, hp, wp, np.float32)
    got = ops.trades_render_prehm(ctx, boxes, hp, wp)
    assert got.shape == (16, 24) and np.array_equal(got == 0, ref64 == 0) and (got == 0).any() and (got > 0).any()
    _check(got, ref32, ref64, "pre_hm / 4")
    summed = sum(R.render_prehm(boxes[k:k + 1], hp, wp) for k in range(2))
    both = R.render_prehm(boxes[:2], hp, wp)
    assert (summed > both + 1e-3).any()                            # the overlap is where max and sum differ
    _check(ops.trades_render_prehm(ctx, boxes[:2], hp, wp), R.render_prehm(boxes[:2], hp, wp, np.float32), both, "pre_hm / 4, overlapping pair")
    none = ops.trades_render_prehm(ctx, np.zeros((0, 3), np.int32), hp, wp)
    assert none.shape == (16, 24) and not none.any()


# ---- pp_trades_decode ----------------------------------------------------------------------------------------------------------------------
def _decode_case(rng, h, w, kind):
    hm = rng.uniform(-6, 1, (h, w, 1)).astype(f32)
    if kind == "ties":
        for y, x in ((2, 3), (5, 9), (8, 15), (h - 3, 4)):
            hm[y, x] = 2.5
    elif kind == "borders":
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            hm[y, x] = 4.0 + 0.01 * (y + x)
    return hm, rng.uniform(0, 1, (h, w, 2)).astype(f32), (rng.uniform(0.5, 6, (h, w, 4)) * [-1, -1, 1, 1]).astype(f32), \
        rng.uniform(-3, 3, (h, w, 2)).astype(f32)


@pytest.mark.parametrize("K", [16, 100])
def test_decode_is_bit_equal(ctx, K):
    h, w = 16, 24
    rng = np.random.default_rng(K)
    kinds = ("random", "ties", "borders")
    cases = [_decode_case(rng, h, w, k) for k in kinds]
    maps = [np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in range(4)]
    dev = [ctx.malloc(m.nbytes) for m in maps]
    try:
        for d, m in zip(dev, maps):
            ctx.h2d(d, m)
        dets, inds = ops.trades_decode(ctx, *dev, len(cases), h, w, K)
    finally:
        for d in dev:
            ctx.free(d)
    for f, kind in enumerate(kinds):
        rd, ri = R.decode(*cases[f], K)
        assert inds[f].tolist() == ri.tolist(), kind
        assert np.array_equal(dets[f], rd), kind
        if kind == "ties":
            tied = [i for i in ri.tolist() if i >= 0 and cases[f][0].reshape(-1)[i] == f32(2.5)]
            assert len(tied) >= 2 and tied == sorted(tied)
        if kind == "borders":
            assert {0, w - 1, (h - 1) * w, h * w - 1} <= set(ri.tolist())
    if K == 100:
        assert (inds == -1).any() and not dets[inds == -1].any()          # fewer peaks than K


# ---- program B ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    return T.synth_trades_state_dict(T.trades_param_shapes(), 11)


def _program_b_inputs(rng, h, w):
    cur = rng.standard_normal((h, w, 64)).astype(f32)
    prev = (cur + 0.3 * rng.standard_normal((h, w, 64))).astype(f32)
    trk = rng.uniform(-4, 4, (h, w, 2)).astype(f32)
    pre_hm = R.render_prehm(np.array([[30, 20, 9], [60, 40, 12], [5, 5, 4]]), 4 * h, 4 * w, np.float64).astype(f32)
    return cur, prev, trk, pre_hm


def _run_b(net, cur, prev, trk, pre_hm):
    for name, a in (("feat_cur", cur), ("feat_prev", prev), ("tracking_offset", trk), ("pre_hm", pre_hm)):
        net.ctx.h2d(net.buffer(name)[0], np.ascontiguousarray(a, f32))
    net.run(1)
    return {k: net.read(k, 1)[0] for k in net.prog.named}


def _fma32(a, b, c):
    """correctly rounded float32 fma of float32 arrays: the product is exact in float64, the sum is rounded to odd (its float64 rounding
    error decides), and one rounding to float32 follows"""
    t = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = t + c
    bb = s - t
    err = (t - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def test_program_b_small_ops_against_float64(ctx, seeded):
    h, w = 16, 24
    cur, prev, trk, pre_hm = _program_b_inputs(np.random.default_rng(3), h, w)
    net = Net(ctx, T.build_program_b(seeded, h, w), 1, numerics="exact")
    got = _run_b(net, cur, prev, trk, pre_hm)
    r64, r32 = R.program_b(seeded, cur, prev, trk, pre_hm, np.float64), R.program_b(seeded, cur, prev, trk, pre_hm, np.float32)
    # difference + concatenation and the broadcast product: one float32 operation each, bit-equal
    cat = got["diff_cat"]
    assert np.array_equal(cat[..., 0:2], trk) and not cat[..., 2:4].any() and np.array_equal(cat[..., 4:], cur - prev)
    assert np.array_equal(got["gated"], pre_hm[..., None] * prev) and (pre_hm > 0).any() and (pre_hm == 0).any()
    # interleave order: channel 2k = dy = conv_offset_h[k], 2k + 1 = dx = conv_offset_w[k]; the nine mask logits are the constant
    _check(got["offset_mask"][..., :18], r32["offsets"], r64["offsets"], "program B offsets (interleaved)")
    swapped = r64["offsets"].reshape(h, w, 9, 2)[..., ::-1].reshape(h, w, 18)
    assert np.abs(got["offset_mask"][..., :18] - swapped).max() > 100 * np.abs(got["offset_mask"][..., :18] - r64["offsets"]).max()
    assert (got["offset_mask"][..., 18:] == f32(T.MASK_LOGIT)).all()
    _check(got["prop"], r32["prop"], r64["prop"], "program B prop (dcn1_1)")
    _check(got["enhanced"], r32["enhanced"], r64["enhanced"], "program B enhanced (two-way softmax blend)")
    a0 = r64["attention"][..., 0]
    assert np.ptp(a0) > 0.2 and (np.abs(a0 - 0.5) < 0.45).mean() > 0.5            # the blend is neither constant nor saturated
    for head, _ in T.HEADS:
        _check(got[head], r32[head], r64[head], f"program B head {head}")


def test_unit_mask_dcn_is_bit_equal_to_the_mask_multiplied_out(ctx, seeded):
    """dcn1_1 takes mask = 1 upstream; PP_OP_DCN3X3 applies a sigmoid to the logit the offset convolution wrote (MASK_LOGIT).  The
    kernel's result must equal, bit for bit, the float32 restatement WITHOUT a mask factor (the header's rule: float32 bilinear
    samples, one fmaf chain over (tap, channel), then the bias) -- which holds only if sigmoid(MASK_LOGIT) is exactly 1.0f."""
    assert f32(1.0 / (1.0 + np.exp(-np.float64(T.MASK_LOGIT)))) == f32(1.0)
    assert f32(1.0 / (1.0 + np.exp(-np.float64(12.0)))) != f32(1.0)                # an ordinary "large" logit would not do
    h, w = 16, 24
    cur, prev, trk, pre_hm = _program_b_inputs(np.random.default_rng(4), h, w)
    net = Net(ctx, T.build_program_b(seeded, h, w), 1, numerics="exact")
    got = _run_b(net, cur, prev, trk, pre_hm)
    om = got["offset_mask"].copy()
    assert np.abs(om[..., :18]).max() > 0.05                                      # the warp does move taps
    om[..., 18:] = 1e4                                                            # the restatement's sigmoid is exactly 1: no mask factor
    cols = F.dcn_columns(got["gated"], om, f32).reshape(h * w, 9 * 64)            # float32 samples, (tap, channel) order
    wk = np.transpose(seeded["dcn1_1.weight"].reshape(64, 64, 9), (2, 1, 0)).reshape(9 * 64, 64)
    acc = np.zeros((h * w, 64), f32)
    for k in range(9 * 64):
        acc = _fma32(cols[:, k:k + 1], wk[k][None, :], acc)
    want = (acc + seeded["dcn1_1.bias"][None, :]).reshape(h, w, 64)
    assert want.dtype == f32 and np.array_equal(got["prop"], want)


# ---- the network at 96 x 160 (cost volume 12 x 20) ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(seeded):
    """two frames through the float64 and the float32 chain: trunk -> emb' -> CVA -> program B (pre_hm from two boxes)"""
    rng = np.random.default_rng(21)
    hp, wp = 96, 160
    x = np.zeros((2, hp, wp, 4), f32)
    base = rng.integers(0, 256, (hp, wp, 3))
    x[0, ..., :3] = (base / 255.0 - T.MEAN) / T.STD
    x[1, ..., :3] = (np.roll(base, (4, -8), (0, 1)) / 255.0 - T.MEAN) / T.STD
    boxes = np.array([[40, 30, 10], [120, 70, 6]], np.int32)
    out = {"x": x, "boxes": boxes}
    for dt in (np.float64, np.float32):
        trunk = R.TrunkRef(seeded, dt)
        (f0, e0), (f1, e1) = trunk.forward(x[0]), trunk.forward(x[1])
        trk = R.cva(e1, e0, dt)[0]
        pre_hm = R.render_prehm(boxes, hp, wp, dt)
        b = R.program_b(seeded, f1, f0, trk, pre_hm, dt)
        out[dt] = dict(feat=np.stack([f0, f1]), emb=np.stack([e0, e1]), tracking_offset=trk, **{k: b[k] for k in ("enhanced",) + tuple(h for h, _ in T.HEADS)})
    return out


@pytest.mark.parametrize("numerics", ["exact", "split"])
def test_network_96x160_against_the_float64_chain(ctx, seeded, chain, numerics):
    hp, wp = 96, 160
    r64, r32 = chain[np.float64], chain[np.float32]
    a = Net(ctx, T.build_program_a(seeded, hp, wp), 2, numerics=numerics)
    b = Net(ctx, T.build_program_b(seeded, hp // 4, wp // 4), 1, numerics=numerics)
    if numerics == "split":
        assert (a.conv_kinds() == 2).any()
    a.forward(chain["x"], out_name="feat")
    feat, emb = a.read("feat", 2), a.read("emb", 2)
    assert emb.shape == (2, 12, 20, 128)
    _check(feat, r32["feat"], r64["feat"], f"{numerics}: feat")
    _check(emb, r32["emb"], r64["emb"], f"{numerics}: emb'")
    trk, _, _ = ops.trades_cva(ctx, emb[1:2], emb[0:1])
    _check(trk[0], r32["tracking_offset"], r64["tracking_offset"], f"{numerics}: tracking_offset")
    pre_hm = ops.trades_render_prehm(ctx, chain["boxes"], hp, wp)
    got = _run_b(b, feat[1], feat[0], trk[0], pre_hm)
    for k in ("enhanced",) + tuple(h for h, _ in T.HEADS):
        _check(got[k], r32[k], r64[k], f"{numerics}: {k}")


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "trades_e2e.npz")


@pytest.fixture()
def synthetic(monkeypatch, tmp_path):
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path / "no_checkpoints"))
    from posepipeline_amd.wrappers import trades as w

    def drop():
        for _, det in w._cache.values():
            det.close()
        w._cache.clear()
    drop()
    yield w
    drop()


@pytest.mark.parametrize("clip", ["landscape", "portrait"])
def test_wrapper_against_the_float64_chain(ctx, synthetic, tmp_path, clip):
    """tests/golden/trades_e2e.npz (tests/golden/make_goldens_trades.py): per frame the ids, boxes (source pixels) and scores of the
    float64 chain of tests/trades_ref.py at the full 480 x 864 / 864 x 480 network size, and of the same chain with the network in
    float32 (their difference, times FACTOR, bounds boxes and scores).  The recorded margins say that every decoded peak's score and
    every greedy gap and size gate of the chain clears FACTOR times the float32 deviation, so ids and membership must be EQUAL, in
    every frame; no frame is left out."""
    from posepipeline_amd import video
    g = np.load(GOLDEN)
    (h, w), n, seed = g[f"{clip}_size"], int(g[f"{clip}_frames"]), int(g[f"{clip}_seed"])
    assert n == 8 and T.input_size(h, w) == ((864, 480) if clip == "portrait" else (480, 864))
    assert g[f"{clip}_score_margin"] > FACTOR * g[f"{clip}_score_dev"] > 0 and g[f"{clip}_gap_margin"] > FACTOR * g[f"{clip}_gap_dev"] > 0
    frames = F.rectangles_clip(n, int(h), int(w), seed=seed)
    path = str(tmp_path / f"{clip}.ppvid")
    video.write_ppvid(path, frames, 30.0)
    tracks = synthetic.trades_bounding_boxes(path)
    assert len(tracks) == n
    ids = [g[f"{clip}_ids{f}"].tolist() for f in range(n)]
    assert [[t["track_id"] for t in fr] for fr in tracks] == ids
    assert sum(len(i) for i in ids) > len({i for fr in ids for i in fr}) > 0 and min(i for fr in ids for i in fr) == 1      # tracks persist
    cat = lambda key: np.concatenate([g[f"{clip}_{key}_{f}"] for f in range(n)])          # noqa: E731
    _check_stored(np.concatenate([np.array([t["tlbr"] for t in fr], np.float64).reshape(-1, 4) for fr in tracks]), cat("bbox32"), cat("bbox64"),
                  f"end to end {clip}: boxes")
    _check_stored(np.array([t["confidence"] for fr in tracks for t in fr]), cat("score32"), cat("score64"), f"end to end {clip}: scores")
    for fr in tracks:
        for t in fr:
            assert isinstance(t["track_id"], int) and isinstance(t["confidence"], float) and t["confidence"] >= 0.5
            np.testing.assert_allclose(t["tlhw"], np.r_[t["tlbr"][:2], t["tlbr"][2:] - t["tlbr"][:2]], rtol=0, atol=0)
    again = synthetic.trades_bounding_boxes(path)            # ids start at 1 again; the carried frame does not leak between calls
    assert [[t["track_id"] for t in fr] for fr in again] == ids
    assert all(np.array_equal(a["tlbr"], b["tlbr"]) for fa, fb in zip(again, tracks) for a, b in zip(fa, fb))
