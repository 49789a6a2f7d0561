"""The fp16 form's per-sample running maxima (csrc/pp_amax.h), through every op that feeds a fp16-form convolution.

Every case is a tiny program  producer op(s) -> reader convolution -> copy of the output  run as Net(ctx, prog, max_batch,
numerics="split_f16").  The copy is there so that an op range can hold every producer and the reader without being the whole program.
The reader is asserted to be on a split kernel: a 3x3 / stride 1 / pad 1 layer with cin % 16 == 0 (the tap kernels), or a 1x1 with
cin >= 64 and cout % 128 == 0 (the product kernel, whose x_amax read path is its own).  pp_net_conv_kinds only tells split from
float32: that such a 1x1 runs on the PRODUCT kernel rests on the selection rule of pp_conv_split_plan with its knobs
(POSEPIPE_SPLIT_GEMM8, POSEPIPE_SPLIT_GEMM4_MIN_C) at their defaults, which no test here can see.  The maxima are observed only through
results.  The reader's scale is 2^k with max |x| 2^k in [2^14, 2^15) per sample, so a maximum that is too small overflows float16 (D
fails: non-finite or far off), and one that is too large by 2^j -- stale from an earlier run, a block neighbour's, or taken over old
buffer content -- moves the float16 split point and changes bits (A, B, C fail).

  A  independence, bit for bit: samples at 2^-27 .. 2^27 (one all-zero) together == each alone == reversed == on a net with a larger
     max_batch == a second run; where the test feeds the producer directly, with every sample's largest element at the sample's first
     float, its last float and next to a boundary of the element-wise kernels' 2048-float4 blocks (amax_ref.peak_offset);
  B  history independence, bit for bit: after a run on 2^20 x, a run on x == a fresh net's -- whole program, op ranges, graph replay;
  C  power-of-two covariance, bit for bit (programs of homogeneous ops, biases zero): sample i times 2^k, k in {-20, 7, 33}, gives
     the output times 2^k; every intermediate's per-sample maximum stays in [2^-100, 2^100] (asserted on the float64 reference);
  D  accuracy: error against the float64 reference of the whole program, per sample and relative to the sample's reference range:
     rms <= 1.25 x and max <= 1.5 x (+ 1e-7) that of the same program on numerics="exact" (the yardstick of
     test_f16_form_keeps_the_yardstick_at_any_magnitude); concat cases again with each slice's producer 2^10 larger in turn;
  E  an op range that begins between the two producers of a concat buffer is refused, and nothing is written.

C is not claimed for LAYERNORM (eps), GELU_ADD and ATTENTION (softmax): not homogeneous.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.program import Net, ProgramBuilder
from tests.amax_ref import RefBuilder, peak_offset

pytestmark = pytest.mark.gpu

RELU = L.PP_RELU_LAST
F32 = np.float32


def _w(rng, co, ci, k, gain=1.0):
    return (rng.standard_normal((co, ci, k, k)) * (gain / np.sqrt(ci * k * k))).astype(F32)


def _tail(pb, y):
    """one op AFTER the reader (a copy of its output): the op range [0, n - 1) then holds every producer and the reader and is not the
    whole program"""
    pb.maxpool(y, 1, 1, 0, name="tail")


def _reader3(pb, rng, x, cout=32):
    h, w, c = pb.dims(x)
    _tail(pb, pb.conv(x, _w(rng, cout, c, 3), None, pad=1, out=pb.buf(h, w, cout, name="output"), name="reader"))


def _reader1(pb, rng, x, cout=128):
    h, w, c = pb.dims(x)
    assert c >= 64 and cout % 128 == 0
    _tail(pb, pb.conv(x, _w(rng, cout, c, 1), None, pad=0, out=pb.buf(h, w, cout, name="output"), name="reader"))


# ---- 1 / 2: PP_OP_UPSAMPLE_ADD, PP_OP_BILINEAR_ADD fed from program inputs ------------------------------------------------------
def _fuse(kind, h, w, c, ups, res1, res2=False, relu=False, reader=3):
    """ups: up_log2 of the 1 .. 3 coarse terms (inputs t0, t1, t2); res1 / res2: inputs r1 / r2 of the output's shape"""
    def make(pb, rng, boost):
        ts = [pb.buf(h >> u, w >> u, c, name=f"t{i}") for i, u in enumerate(ups)]
        r1 = pb.buf(h, w, c, name="r1") if res1 else -1
        kw = dict(up_log2=ups[0], res1=r1, relu=RELU if relu else L.PP_RELU_NONE, more=[(t, u) for t, u in zip(ts[1:], ups[1:])])
        if kind == "ua":
            y = pb.upsample_add(ts[0], res2=pb.buf(h, w, c, name="r2") if res2 else -1, **kw)
        else:
            y = pb.bilinear_add(ts[0], **kw)
        (_reader3 if reader == 3 else _reader1)(pb, rng, y)
    return make


def _bilinear_concat(pb, rng, boost):
    """HRNetv2's resize + concatenate: a convolution writes channels [0, 16), PP_OP_BILINEAR_ADD channels [16, 32) of one buffer"""
    x = pb.buf(12, 20, 16, name="x")
    t = pb.buf(6, 10, 16, name="t0")
    cat = pb.buf(12, 20, 32)
    pb.conv(x, _w(rng, 16, 16, 3, 1024.0 if boost == 0 else 1.0), None, pad=1, relu=RELU, out=cat, out_c_off=0)
    pb.bilinear_add(t, up_log2=1, out=cat, out_c_off=16)
    _reader3(pb, rng, cat)


# ---- 3: convolution producers -----------------------------------------------------------------------------------------------------
def _conv_producer(h, w, cin, cout, k, stride=1, reader=3):
    def make(pb, rng, boost):
        x = pb.buf(h, w, cin, name="x")
        y = pb.conv(x, _w(rng, cout, cin, k), None, pad=k // 2, stride=stride, relu=RELU)
        (_reader3 if reader == 3 else _reader1)(pb, rng, y)
    return make


# ---- 4: producers without a fused maximum (stand-alone pass) ----------------------------------------------------------------------
def _maxpool(pb, rng, boost):
    _reader3(pb, rng, pb.maxpool(pb.buf(12, 20, 16, name="x"), 3, 1, 1))


def _spp(pb, rng, boost):
    """YOLO's SPP: a convolution and three pools of ITS slice fill the four slices of one buffer (out_c_off / in_c_off).  The pools
    have no weights and take their values from slice 0, so D cannot make one pool slice alone 2^10 larger: its boost scales the
    convolution, and every slice with it."""
    x = pb.buf(12, 20, 16, name="x")
    cat = pb.buf(12, 20, 64)
    pb.conv(x, _w(rng, 16, 16, 1, 1024.0 if boost == 0 else 1.0), None, pad=0, out=cat, out_c_off=0)
    for j, k in enumerate((5, 9, 13)):
        pb.maxpool(cat, k, 1, k // 2, out=cat, out_c_off=16 * (j + 1), in_c_off=0, c=16)
    _reader1(pb, rng, cat)


def _avgpool(pb, rng, boost):
    _reader3(pb, rng, pb.avgpool(pb.buf(13, 21, 16, name="x"), 2, 2, 1))


def _depth_to_space(pb, rng, boost):
    _reader3(pb, rng, pb.depth_to_space(pb.buf(6, 10, 64, name="x")))


def _dwconv(pb, rng, boost):
    _reader3(pb, rng, pb.dwconv3x3(pb.buf(12, 20, 16, name="x"), (rng.standard_normal((16, 1, 3, 3)) / 3).astype(F32), None))


def _gelu_add(pb, rng, boost):
    x = pb.buf(12, 20, 16, name="x")
    _reader3(pb, rng, pb.gelu_add(x, res1=pb.buf(12, 20, 16, name="r1")))


def _layernorm(pb, rng, boost):
    x = pb.buf(12, 20, 16, name="x")
    _reader3(pb, rng, pb.layernorm(x, (1 + 0.2 * rng.standard_normal(16)).astype(F32), (0.2 * rng.standard_normal(16)).astype(F32)))


def _dwdeconv(pb, rng, boost):
    _reader3(pb, rng, pb.dwdeconv(pb.buf(6, 10, 16, name="x"), (rng.standard_normal((16, 1, 4, 4)) / 2).astype(F32), 2))


def _dcn(pb, rng, boost):
    x = pb.buf(12, 20, 16, name="x")
    om = pb.buf(12, 20, 28, name="om")        # 18 offsets, 9 mask logits, one padding channel: a fixed input, never scaled
    _reader3(pb, rng, pb.dcn3x3(x, om, _w(rng, 16, 16, 3), None))


def _attention(pb, rng, boost):
    """64 tokens of 64 channels, two heads; the 1x1 read (64 -> 128) is a product-kernel shape, so the case is in"""
    _reader1(pb, rng, pb.attention(pb.buf(8, 8, 192, name="x"), c_real=64, heads=2))


# ---- 5 / 6 --------------------------------------------------------------------------------------------------------------------------
def _partly_covered(pb, rng, boost):
    """a convolution writes channels [0, 16) of the named 32-channel buffer `half`; the host fills [16, 32) before the run"""
    x = pb.buf(12, 20, 16, name="x")
    half = pb.buf(12, 20, 32, name="half")
    pb.conv(x, _w(rng, 16, 16, 3, 1024.0 if boost == 0 else 1.0), None, pad=1, out=half, out_c_off=0)
    _reader3(pb, rng, half)


def _recycled(pb, rng, boost):
    """x -> a -> b (weights 2^-12) -> c -> reader: c's output takes a's physical buffer, at 2^-12 of its magnitude"""
    y = pb.buf(12, 20, 16, name="x")
    for gain in (1.0, 2.0 ** -12, 1.0):
        y = pb.conv(y, _w(rng, 16, 16, 3, gain), None, pad=1, relu=RELU)
    _reader3(pb, rng, y)


@dataclass
class Case:
    make: object
    batch: int
    peak: str = None              # the input whose layout decides where the producer's largest element sits (None: not controlled)
    peak_kw: dict = field(default_factory=dict)   # amax_ref.peak_offset: channels the peak may sit on / the output a coarse input maps to
    homogeneous: bool = True      # C applies
    fixed: tuple = ()             # inputs that are not scaled with the sample (DCN's offsets / mask)
    boosts: dict = field(default_factory=dict)    # D: slice index -> input scaled by 2^10 (None: the make function scales weights)
    s2: bool = False              # POSEPIPE_SPLIT_S2_MIN_CIN=16 while the nets are created
    split_at: int = None          # B: the program also runs as [0, split_at) + [split_at, n)
    check: object = None          # extra assertion on (prog, net)


def _assert_reuse(prog, net):
    assert prog.ops[2].out == prog.ops[0].out and prog.ops[2].out not in (prog.ops[1].out, prog.ops[3].out), [(o.in_, o.out) for o in prog.ops]


def _assert_producer_split(prog, net):
    assert net.conv_kinds()[0] == 2, net.conv_kinds()


CASES = {
    # 8x8x16 = 1024 floats: a block spans 8 samples; 12x20x16 = 3840: blocks straddle two or three; 24x20x32 = 15360: inside a sample
    "ua-8x8-1term": Case(_fuse("ua", 8, 8, 16, (1,), True), 11, "r1"),
    "ua-8x8-3terms-res2-relu": Case(_fuse("ua", 8, 8, 16, (1, 2, 3), True, True, True), 11, "r1"),
    "ua-12x20-2terms-res2": Case(_fuse("ua", 12, 20, 16, (1, 2), True, True), 5, "r1"),
    "ua-12x20-1term-relu": Case(_fuse("ua", 12, 20, 16, (1,), True, False, True), 5, "r1"),
    "ua-24x20-3terms-relu": Case(_fuse("ua", 24, 20, 32, (1, 2, 2), True, False, True), 3, "r1"),
    "ua-24x20-2terms-res2-relu": Case(_fuse("ua", 24, 20, 32, (2, 1), True, True, True), 3, "r1"),
    "ua-4x4x64-read1x1": Case(_fuse("ua", 4, 4, 64, (1, 2), True, True, reader=1), 11, "r1"),
    "bl-8x8-1term-res1": Case(_fuse("bl", 8, 8, 16, (1,), True), 11, "r1"),
    "bl-12x20-2terms-relu": Case(_fuse("bl", 12, 20, 16, (1, 2), False, relu=True), 5, "t0", dict(coarse=(12, 20, 16, 1))),
    "bl-24x20-3terms-res1": Case(_fuse("bl", 24, 20, 32, (1, 2, 2), True), 3, "r1"),
    "bl-4x4x64-read1x1": Case(_fuse("bl", 4, 4, 64, (1, 2), True, reader=1), 11, "r1"),
    "bl-concat-slice": Case(_bilinear_concat, 5, "t0", dict(coarse=(12, 20, 16, 1)), boosts={0: None, 1: "t0"}),
    # 64 output pixels: fused, a 256-pixel workgroup spans four samples; 36: stand-alone pass, amax_kernel's per * n grid at n = 70
    "conv-3x3-8x8-fused": Case(_conv_producer(8, 8, 16, 32, 3), 9, split_at=1),
    "conv-3x3-6x6-pass": Case(_conv_producer(6, 6, 16, 32, 3), 70),
    "conv-1x1-product": Case(_conv_producer(8, 8, 64, 128, 1, reader=1), 5, check=_assert_producer_split),
    "conv-3x3-stride2": Case(_conv_producer(16, 16, 16, 32, 3, stride=2), 5, s2=True, check=_assert_producer_split),
    "maxpool": Case(_maxpool, 5, "x"),
    "maxpool-spp-concat": Case(_spp, 5, "x", boosts={0: None}),
    "avgpool": Case(_avgpool, 5, "x"),
    "depth-to-space": Case(_depth_to_space, 5, "x"),
    "dwconv3x3": Case(_dwconv, 5, "x"),
    "gelu-add": Case(_gelu_add, 5, "r1", homogeneous=False),
    "layernorm": Case(_layernorm, 5, "x", homogeneous=False),
    "dwdeconv": Case(_dwdeconv, 5, "x"),
    "dcn3x3": Case(_dcn, 5, "x", fixed=("om",)),
    "attention-read1x1": Case(_attention, 5, "x", homogeneous=False),
    "partly-covered-buffer": Case(_partly_covered, 5, "half", dict(channels=32, c_min=16), boosts={0: None, 1: "half"}),
    "recycled-buffer": Case(_recycled, 5, check=_assert_reuse, split_at=2),
}


@functools.lru_cache(maxsize=None)
def _built(name, boost=None):
    """(the program, its float64 twin): the same function on both builders, the same seed"""
    seed = sorted(CASES).index(name) + 1
    pb, rb = ProgramBuilder(), RefBuilder()
    CASES[name].make(pb, np.random.default_rng(seed), boost)
    CASES[name].make(rb, np.random.default_rng(seed), boost)
    return pb.build(), rb


def _net(ctx, monkeypatch, name, boost=None, extra_batch=0, numerics="split_f16"):
    case = CASES[name]
    prog, _ = _built(name, boost)
    if case.s2:
        monkeypatch.setenv("POSEPIPE_SPLIT_S2_MIN_CIN", "16")      # read when the net is planned
    net = Net(ctx, prog, max_batch=case.batch + extra_batch, numerics=numerics)
    if case.s2:
        monkeypatch.delenv("POSEPIPE_SPLIT_S2_MIN_CIN")
    if numerics == "split_f16":
        # without this the case tests nothing
        assert net.split_kind == "split_f16" and net.conv_kinds()[len(prog.ops) - 2] == 2, (net.split_kind, net.conv_kinds())
        if case.check:
            case.check(prog, net)
    return net


def _inputs(name, exps, where=None, seed=0):
    """heavy-tailed inputs, sample i times 2^exps[i] (None: an all-zero sample); `where`: the peak input's largest element"""
    case = CASES[name]
    _, rb = _built(name)
    rng = np.random.default_rng(1000 + seed)
    n = len(exps)
    out = {}
    for nm in sorted(k for k in rb.named if k != "output"):
        shape = (n,) + rb.shapes[rb.named[nm]]
        if nm in case.fixed:
            out[nm] = (1.5 * rng.standard_normal(shape)).astype(F32)
            continue
        x = (rng.standard_normal(shape) * np.exp(rng.standard_normal(shape))).astype(F32)
        if where is not None and nm == case.peak:
            flat = x.reshape(n, -1)
            co = case.peak_kw.get("coarse")
            per = co[0] * co[1] * co[2] if co else flat.shape[1]       # floats per sample of what the producer kernel writes
            for i in range(n):
                flat[i, peak_offset(where, per, i, **case.peak_kw)] = 64 * np.abs(flat[i]).max()
        scale = np.array([0.0 if e is None else 2.0 ** e for e in exps], F32).reshape(-1, 1, 1, 1)
        out[nm] = x * scale
    return out


def _spread(n):
    """2^-27 .. 2^27 over the batch, the middle sample all-zero"""
    e = [int(v) for v in np.round(np.linspace(-27, 27, n))]
    e[n // 2] = None
    return e


def _scaled(name, inputs, pow2):
    """every scaled input of sample i times 2^pow2[i] (exact)"""
    f = (2.0 ** np.asarray(pow2, np.float64)).astype(F32).reshape(-1, 1, 1, 1)
    return {k: v if k in CASES[name].fixed else v * f for k, v in inputs.items()}


def _run(ctx, net, inputs, first=0, last=None, sel=None):
    n = 0
    for nm, arr in inputs.items():
        arr = arr if sel is None else arr[sel]
        n = arr.shape[0]
        ctx.h2d(net.buffer(nm)[0], arr)
    net.run(n, first, last)
    return net.read("output", n)


@pytest.mark.parametrize("name", list(CASES))
def test_a_sample_is_independent_of_its_batch(ctx, monkeypatch, name):
    """A.  A wrong img_first / last, a neighbour's maximum folded into a block's register pair, a slot stride taken from batch
    instead of max_batch, or a maximum kept from the run before all change some sample's bits here."""
    case = CASES[name]
    net = _net(ctx, monkeypatch, name)
    wide = _net(ctx, monkeypatch, name, extra_batch=3)
    n = case.batch
    for where in (("first", "last", "block") if case.peak else (None,)):
        x = _inputs(name, _spread(n), where)
        together = _run(ctx, net, x)
        assert np.isfinite(together).all(), where
        assert np.array_equal(_run(ctx, net, x), together), (where, "second run")
        rev = {k: v[::-1].copy() for k, v in x.items()}
        assert np.array_equal(_run(ctx, net, rev)[::-1], together), (where, "reversed")
        assert np.array_equal(_run(ctx, wide, x), together), (where, "larger max_batch")
        for i in range(n):
            alone = _run(ctx, net, x, sel=slice(i, i + 1))
            assert np.array_equal(alone[0], together[i]), (where, "alone", i)


@pytest.mark.parametrize("name", list(CASES))
def test_b_a_run_does_not_depend_on_the_run_before(ctx, monkeypatch, name):
    """B.  The maxima are zeroed ahead of every run (net_reset_amax) -- eager, over op ranges, and inside a captured graph."""
    case = CASES[name]
    n, n_ops = case.batch, len(_built(name)[0].ops)
    e = [int(v) for v in np.round(np.linspace(-7, 7, n))]
    x = _inputs(name, e, "block" if case.peak else None, seed=1)
    big = _scaled(name, x, [20] * n)
    fresh = _run(ctx, _net(ctx, monkeypatch, name), x)
    assert np.isfinite(fresh).all()
    net = _net(ctx, monkeypatch, name)
    _run(ctx, net, big)
    assert np.array_equal(_run(ctx, net, x), fresh), "whole program"
    # an op range that holds all producers and the reader and is NOT the whole program (the last op is a copy of the output)
    _run(ctx, net, big, 0, n_ops - 1)
    assert np.array_equal(_run(ctx, net, x, 0, n_ops - 1), fresh), "run(batch, 0, n - 1)"
    if case.split_at:
        _run(ctx, net, big)
        _run(ctx, net, x, 0, case.split_at)
        assert np.array_equal(_run(ctx, net, x, case.split_at, n_ops - 1), fresh), "run in two ranges"
    # a captured graph replayed on inputs of another magnitude
    net = _net(ctx, monkeypatch, name)
    net.capture(n)
    _run(ctx, net, big)
    assert np.array_equal(_run(ctx, net, x), fresh), "graph replay"


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c.homogeneous])
def test_c_power_of_two_covariance(ctx, monkeypatch, name):
    """C.  x s, both float16 terms and every product are the same numbers whatever power of two the sample is multiplied by, and the
    un-scaling is exact: a maximum that does not follow the data moves the split point and changes bits."""
    case = CASES[name]
    n = case.batch
    _, rb = _built(name)
    x = _inputs(name, [int(v) for v in np.round(np.linspace(-7, 7, n))], "block" if case.peak else None, seed=2)
    net = _net(ctx, monkeypatch, name)
    y = _run(ctx, net, x)
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    for turn in range(3):      # every sample at every k, neighbours at the other two
        ks = [(-20, 7, 33)[(i + turn) % 3] for i in range(n)]
        xk = _scaled(name, x, ks)
        for inp in ((x, xk) if turn == 0 else (xk,)):      # float32 normals everywhere, far from pp_amax_exp's clamp: the premise
            for m in rb.run({k: v.astype(np.float64) for k, v in inp.items()})[1]:
                assert (m >= 2.0 ** -100).all() and (m <= 2.0 ** 100).all(), m
        yk = _run(ctx, net, xk)
        f = (2.0 ** np.asarray(ks, np.float64)).astype(F32).reshape(-1, 1, 1, 1)
        for i in range(n):
            assert np.array_equal(yk[i], y[i] * f[i]), (i, ks[i], float(np.abs(yk[i] / f[i] - y[i]).max() / np.abs(y[i]).max()))


@pytest.mark.parametrize("name", list(CASES))
def test_d_accuracy_against_float64(ctx, monkeypatch, name):
    """D.  The fp16 form's yardstick on the whole tiny program, per sample; a slice the maximum missed overflows float16 here.

    Bounded run: the yardstick's own input distribution (normal x log-normal) at the magnitudes of A, one fixed seed.  On an MI355X
    the worst per-sample ratios are rms 1.16 and max 1.73; the two cases above 1.5 on the max (`conv-3x3-6x6-pass` 1.73,
    `bl-4x4x64-read1x1` 1.67) are inside the bound only through its + 1e-7 term, and over other seeds the per-sample max ratio of
    such small maps reaches 1.8 - 2.0 (DESIGN_LOG.md 5n): the fixed seed is part of why this passes.
    Second run: A's peak element in the input.  Around one element at 64 x everything else the outputs are ONE product each; there
    two 22-bit operands cost up to 2^-22 of the output by themselves where the float32 chain's fmaf has an exact product, so up to
    twice the chain's error follows from the formats and the constants for sums of many comparable products do not apply.  That run
    asserts finite outputs (a maximum that missed the peak overflows float16) and prints its ratios (up to 2.07)."""
    case = CASES[name]
    n = case.batch
    for boost, boost_input in ([(None, None)] + list(case.boosts.items())):
        for where in ((None, "block") if case.peak else (None,)):
            x = _inputs(name, _spread(n), where, seed=3)
            if boost_input:
                x[boost_input] = x[boost_input] * F32(1024)
            ref, _ = _built(name, boost)[1].run({k: v.astype(np.float64) for k, v in x.items()})
            split = _run(ctx, _net(ctx, monkeypatch, name, boost), x)
            exact = _run(ctx, _net(ctx, monkeypatch, name, boost, numerics="exact"), x)
            assert np.isfinite(split).all(), (boost, where)
            scale = np.abs(ref).reshape(n, -1).max(1) + 1e-300
            err = lambda y: (np.sqrt(np.mean(((y - ref) ** 2).reshape(n, -1), 1)) / scale, np.abs(y - ref).reshape(n, -1).max(1) / scale)
            (rs, ms), (re, me) = err(split), err(exact)
            nz = re > 0
            print(f"[amax D] {name} boost={boost} peak={where}: rms {rs.max():.2e} vs exact {re.max():.2e} (worst ratio {(rs[nz] / re[nz]).max():.2f}), "
                  f"max {ms.max():.2e} vs exact {me.max():.2e} (worst ratio {(ms[nz] / me[nz]).max():.2f})")
            if where is None:
                assert (rs <= 1.25 * re + 1e-9).all(), (boost, rs, re)
                assert (ms <= 1.5 * me + 1e-7).all(), (boost, ms, me)


def test_e_range_that_splits_the_producers_is_refused(ctx, monkeypatch):
    """E.  ops 0 (convolution) and 1 (PP_OP_BILINEAR_ADD) fill one concat buffer: run(batch, 1, 3) would keep op 0's share of the
    maxima from an earlier run, so it is an error, raised before anything is launched."""
    name = "bl-concat-slice"
    n = CASES[name].batch
    net = _net(ctx, monkeypatch, name)
    x = _inputs(name, [0] * n)
    _run(ctx, net, x)
    dptr, _, (h, w, c) = net.buffer("output")
    sentinel = np.random.default_rng(5).standard_normal((n, h, w, c)).astype(F32)
    ctx.h2d(dptr, sentinel)
    with pytest.raises(L.PosePipeHipError, match="splits the producers"):
        net.run(n, 1, 3)
    assert np.array_equal(net.read("output", n), sentinel)
    # the ranges that hold both producers, or only the reader, run (the trailing copy has recycled the concat buffer: refill it first)
    net.run(n, 0, 2)
    net.run(n, 2, 3)
    assert np.array_equal(net.read("output", n), _run(ctx, net, x))
