"""The product kernel's two wave arrangements (conv_split_gemm_kernel, fp16 form): four waves 2 x 2 with wave tiles of 128 pixels x 64
channels, or 4 x 1 with 64 pixels x 128 channels, where every activation is read from LDS and split into its two float16 terms once
per workgroup instead of twice.  Both accumulate, per output element, the same products in the same order (stage by stage g1 h0,
g0 h1, g0 h0) and run the same epilogue arithmetic, so they give the same BITS: every case below runs under
pp_debug_knob("split_gemm_wave_tile", 0) and (.., 1) in one process and compares with np.array_equal.  The 4 x 1 form (the default)
is also held against float64 with the helpers and bounds of the product-kernel tests in test_gpu_split.py / test_gpu_split_fold.py.

Inputs are heavy-tailed (the low float16 term matters) and the samples of a batch span magnitudes 1e-3 .. 1e2, so a sample scaled
by a neighbour's maximum loses its low bits and shows up.  Shapes are the smallest at which the per-wave bookkeeping changes: what
a wave owns went from 128 to 64 pixels (ragged tiles, sample boundaries inside a wave and between its two pixel blocks, the
one-sample-per-pixel atomics of the RoI head, the maxima a wave commits) and from 2 to 4 channel blocks (both epilogues)."""
import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.program import Net, ProgramBuilder
from tests.helpers import hip_conv_op
from tests.test_gpu_split import check_layer, conv64
from tests.test_gpu_split_fold import _pair_program, _ref_pair, _yardstick

pytestmark = pytest.mark.gpu
LAST, FIRST = L.PP_RELU_LAST, L.PP_RELU_FIRST


@pytest.fixture
def lib16(ctx):
    """the fp16 form as the split form of single ops; every knob back to the environment's choice afterwards"""
    L.check(ctx.lib.pp_conv_split_kind(1), "pp_conv_split_kind")
    yield ctx.lib
    for knob in (b"split_gemm_wave_tile", b"split_gemm_epilogue"):
        L.check(ctx.lib.pp_debug_knob(knob, -1), "pp_debug_knob")
    L.check(ctx.lib.pp_conv_split_kind(-1), "pp_conv_split_kind")
    L.check(ctx.lib.pp_conv_exact(1), "pp_conv_exact")


def _heavy(rng, shape):
    """as test_gpu_split_digests._heavy, times a magnitude per sample: 1e-3 .. 1e2 over the batch"""
    n = shape[0]
    mag = (10.0 ** np.linspace(-3, 2, n)).reshape((n,) + (1,) * (len(shape) - 1))
    return (rng.standard_normal(shape) * np.exp(2 * rng.standard_normal(shape)) * mag).astype(np.float32)


def _under_both_tiles(lib, fn, epilogues=(-1,)):
    """fn() on the split kernels under wave tile 0 (2 x 2) and 1 (4 x 1), for each epilogue setting: all the same bits.  Returns
    the 4 x 1 form's result"""
    out = []
    L.check(lib.pp_conv_exact(0), "pp_conv_exact")
    try:
        for epi in epilogues:
            L.check(lib.pp_debug_knob(b"split_gemm_epilogue", epi), "pp_debug_knob")
            for tile in (0, 1):
                L.check(lib.pp_debug_knob(b"split_gemm_wave_tile", tile), "pp_debug_knob")
                out.append((epi, tile, fn()))
    finally:
        L.check(lib.pp_debug_knob(b"split_gemm_wave_tile", -1), "pp_debug_knob")
        L.check(lib.pp_debug_knob(b"split_gemm_epilogue", -1), "pp_debug_knob")
        L.check(lib.pp_conv_exact(1), "pp_conv_exact")
    ref = out[-1][2]
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    for epi, tile, y in out[:-1]:
        assert np.array_equal(y, ref), f"epilogue {epi}, wave tile {tile} differs from epilogue {out[-1][0]}, wave tile 1"
    return ref


def _layer(rng, n, h, w, cin, cout, k=1, stride=1):
    x = _heavy(rng, (n, h, w, cin))
    wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
    r1, r2 = (rng.standard_normal((n, ho, wo, cout)).astype(np.float32) for _ in range(2))
    return x, wt, b, r1, r2


# (n, h, w, cin, cout, k, stride)
SHAPES = {
    # ragged M: 65 px (waves 1 .. 3 of the only tile partly or wholly past the tensor), 129 px, 255 px
    "ragged_65": (1, 5, 13, 64, 128, 1, 1),
    "ragged_129": (1, 3, 43, 64, 128, 1, 1),
    "ragged_255": (1, 15, 17, 64, 128, 1, 1),
    # 35 px per sample: two or three samples in every 64-pixel wave, boundaries inside and between its two pixel blocks
    "samples_35px": (9, 5, 7, 64, 128, 1, 1),
    # full cover, a sample per pixel (the RoI head's fc6 form): per-lane scales, per-pixel maxima
    "roi_full_cover": (300, 7, 7, 64, 128, 7, 1),
    # one, two (column remap of the 1-D launch) and three channel columns
    "columns_1": (2, 12, 20, 256, 128, 1, 1),
    "columns_2": (2, 12, 20, 256, 256, 1, 1),
    "columns_3": (2, 12, 20, 256, 384, 1, 1),
    # K: 4 and 5 stages (the pipeline's start-up edge: two stages are requested before the loop), and the long loop
    "k_64": (2, 12, 20, 64, 256, 1, 1),
    "k_80": (2, 12, 20, 80, 256, 1, 1),
    "k_1024": (2, 12, 20, 1024, 256, 1, 1),
    # 1x1 stride 2
    "stride_2": (2, 20, 34, 256, 512, 1, 2),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_wave_tiles_give_the_same_bits(ctx, lib16, name):
    n, h, w, cin, cout, k, stride = SHAPES[name]
    rng = np.random.default_rng(sum(SHAPES[name]))
    x, wt, b, r1, _ = _layer(rng, n, h, w, cin, cout, k, stride)
    for relu, res in ((0, None), (LAST, r1)):
        y = _under_both_tiles(lib16, lambda: hip_conv_op(ctx, x, wt, b, stride=stride, relu=relu, res1=res))
        # the 4 x 1 form (the default) against float64: the bounds of test_split_1x1_and_full_cover_layers
        check_layer(lib16, ctx, x, wt, b, 0, stride=stride, res=res, relu=relu)
        L.check(lib16.pp_conv_exact(0), "pp_conv_exact")
        assert np.array_equal(hip_conv_op(ctx, x, wt, b, stride=stride, relu=relu, res1=res), y), "the default is not the 4 x 1 form's bits"
        L.check(lib16.pp_conv_exact(1), "pp_conv_exact")


def _check64(ref, exact, split):
    """check_layer's three bounds, for the epilogues its reference does not cover"""
    scale = np.abs(ref).max()
    e_exact, e_split = np.abs(exact - ref).max() / scale, np.abs(split - ref).max() / scale
    r_exact, r_split = np.sqrt(np.mean((exact - ref) ** 2)) / scale, np.sqrt(np.mean((split - ref) ** 2)) / scale
    print(f"max split {e_split:.3e} exact {e_exact:.3e}; rms split {r_split:.3e} exact {r_exact:.3e}")
    assert not np.array_equal(exact, split)
    assert e_split <= 1.5 * e_exact + 1e-7, (e_split, e_exact)
    assert r_split <= 1.1 * r_exact + 1e-8, (r_split, r_exact)
    assert np.abs(split - exact).max() <= 1e-5 * scale


def test_epilogue_variants_under_both_tiles_and_both_epilogues(ctx, lib16):
    """2 x 12 x 20 x 128 -> 256 (two columns; 240 px per sample: a boundary inside the last wave of the first tile, a ragged second
    tile): no residual, res1 with ReLU last / first, res1 + res2, Mish; then res1 read shifted on an odd fine map.  Register and
    LDS-transposed epilogue x both wave tiles: four runs, one set of bits"""
    rng = np.random.default_rng(83)
    x, wt, b, r1, r2 = _layer(rng, 2, 12, 20, 128, 256)
    for relu, ra, rb in ((0, None, None), (LAST, r1, None), (FIRST, r1, None)):
        _under_both_tiles(lib16, lambda: hip_conv_op(ctx, x, wt, b, relu=relu, res1=ra, res2=rb), epilogues=(0, 1))
        check_layer(lib16, ctx, x, wt, b, 0, res=ra, relu=relu)
    y = _under_both_tiles(lib16, lambda: hip_conv_op(ctx, x, wt, b, relu=LAST, res1=r1, res2=r2), epilogues=(0, 1))
    _check64(conv64(x, wt, b, 0, res=r1.astype(np.float64) + r2, relu=LAST), hip_conv_op(ctx, x, wt, b, relu=LAST, res1=r1, res2=r2), y)
    y = _under_both_tiles(lib16, lambda: hip_conv_op(ctx, x, wt, b, relu=L.PP_ACT_MISH, res1=r1), epilogues=(0, 1))
    exact = hip_conv_op(ctx, x, wt, b, relu=L.PP_ACT_MISH, res1=r1)         # (test_split_activation_epilogues' bound)
    assert not np.array_equal(exact, y) and np.abs(y - exact).max() <= 1e-5 * np.abs(exact).max()
    # FPN lateral: the coarser map read at (y >> 1, x >> 1), odd fine map 21 x 35 over 11 x 18
    xs = _heavy(rng, (2, 21, 35, 128))
    rs = rng.standard_normal((2, 11, 18, 256)).astype(np.float32)
    y = _under_both_tiles(lib16, lambda: hip_conv_op(ctx, xs, wt, b, res1=rs, res1_shift=1), epilogues=(0, 1))
    up = np.repeat(np.repeat(rs, 2, axis=1), 2, axis=2)[:, :21, :35]
    _check64(conv64(xs, wt, b, 0, res=up), hip_conv_op(ctx, xs, wt, b, res1=rs, res1_shift=1), y)


@pytest.mark.parametrize("stride", [1, 2])
def test_folded_shortcut_under_both_tiles(ctx, lib16, stride):
    """the SEG2 instance: tests/test_gpu_split_fold's pair program at 2 x 20 x 13 (260 px per sample at stride 1: the tile straddles
    the samples and the last one is ragged), the shortcut read at its own stride"""
    n, h, w, cx, ch, cout = 2, 20, 13, 64, 64, 256
    rng = np.random.default_rng(100 + stride)
    prog, wts = _pair_program(h, w, cx, ch, cout, stride, rng)
    x = _heavy(rng, (n, h, w, cx + ch))
    exact, fused = Net(ctx, prog, max_batch=n, numerics="exact"), Net(ctx, prog, max_batch=n, numerics="split_f16")
    assert int((fused.folded_into() >= 0).sum()) == 1
    y = _under_both_tiles(lib16, lambda: fused.forward(x), epilogues=(0, 1))
    _yardstick(y, exact.forward(x), _ref_pair(x, stride, cx, wts), f"folded, stride {stride}, 4 x 1")
    fused.close()
    exact.close()


def test_committed_maxima_under_both_tiles(ctx, lib16):
    """product -> 3x3 on a zero-halo buffer, 3 samples of 27 x 36 (972 px: the sample boundaries fall inside a wave's first and
    second pixel block): the 3x3 scales each sample by the maximum the product's epilogue committed, so a maximum filed under the
    wrong sample, or missed, changes the final output between the two wave tiles"""
    n, h, w, cin, c = 3, 27, 36, 64, 128
    rng = np.random.default_rng(57)
    pb = ProgramBuilder()
    xin = pb.buf(h, w, cin, name="input")
    y1 = pb.conv(xin, (rng.standard_normal((c, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32), rng.standard_normal(c).astype(np.float32), relu=LAST)
    pb.conv(y1, (rng.standard_normal((32, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32), rng.standard_normal(32).astype(np.float32), pad=1,
            out=pb.buf(h, w, 32, name="output"))
    prog = pb.build()
    assert max(prog.buf_pad) > 0
    x = _heavy(rng, (n, h, w, cin))
    exact, net = Net(ctx, prog, max_batch=n, numerics="exact"), Net(ctx, prog, max_batch=n, numerics="split_f16")
    assert (net.conv_kinds() == 2).all()
    y = _under_both_tiles(lib16, lambda: net.forward(x), epilogues=(0, 1))
    ye = exact.forward(x)
    scale = np.abs(ye).reshape(n, -1).max(1).reshape(n, 1, 1, 1)          # per sample (test_f16_form_strided_patch_inside_a_program's bound)
    assert not np.array_equal(ye, y) and (np.abs(y - ye) <= 1e-5 * scale).all()
    net.close()
    exact.close()


def test_knob_is_validated(ctx):
    assert ctx.lib.pp_debug_knob(b"split_gemm_wave_tile", 2) != 0
    assert ctx.lib.pp_debug_knob(b"split_gemm_wave_tile", -1) == 0
