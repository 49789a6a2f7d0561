"""Projection shortcuts folded into conv3's product (conv_split_gemm_kernel<.., SEG2>, pp_net_folded_into): fp16-form nets evaluate
relu(W3 h + b3 + Ws x + bs) as ONE product over the concatenated input channels, under one activation scale per sample and one weight
scale per output channel.

Yardstick (the project's, from test_f16_form_3x3_stride_2_strided_patch): against the float64 evaluation of the UNFUSED two-op
definition, per sample and relative to that sample's max |ref|, the fused program's rms error is at most 1.25 x the float32-kernel
(exact) program's + 1e-9 and its maximum error at most 1.5 x the exact program's + 1e-7.

The programs feed the two operands as channel slices of ONE input (1x1 max-pools = slice copies), so that every sample's h and x can
be given any magnitude independently.  In the unequal-segment case conv3 is the 256-channel side (the product kernel takes layers
from 64 input channels; a 16-channel conv3 would not be on it and the pattern would not match) and the shortcut the 16-channel one."""
import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.program import Net, ProgramBuilder
from tests.test_gpu_split import conv64

pytestmark = pytest.mark.gpu
R = L.PP_RELU_LAST


def _w(rng, cout, cin, k=1):
    return (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)


def _pair_program(h, w, cx, ch, cout, stride, rng, *, relu_a=L.PP_RELU_NONE, second_reader=False):
    """input [h][w][cx + ch] -> x = channels [0, cx), h = channels [cx, cx + ch) at the output geometry; shortcut A: 1x1 / stride on x;
    conv3 B: 1x1 on h, + A, ReLU -> "output".  Returns (program, weights for the reference)"""
    pb = ProgramBuilder()
    inp = pb.buf(h, w, cx + ch, name="input")
    xs = pb.maxpool(inp, 1, 1, 0, c=cx, in_c_off=0, name="x")
    hs = pb.maxpool(inp, 1, stride, 0, c=ch, in_c_off=cx, name="h")
    ws, bs, w3, b3 = _w(rng, cout, cx), rng.standard_normal(cout).astype(np.float32), _w(rng, cout, ch), rng.standard_normal(cout).astype(np.float32)
    idn = pb.conv(xs, ws, bs, stride=stride, relu=relu_a, name="shortcut")
    ho, wo, _ = pb.dims(hs)
    pb.conv(hs, w3, b3, relu=R, res1=idn, out=pb.buf(ho, wo, cout, name="output"), name="conv3")
    if second_reader:
        pb.maxpool(idn, 1, 1, 0, name="reader2", out=pb.buf(ho, wo, cout, name="idn_copy"))
    return pb.build(), (ws, bs, w3, b3)


def _ref_pair(x, stride, cx, wts, relu_a=L.PP_RELU_NONE):
    ws, bs, w3, b3 = wts
    idn = conv64(x[..., :cx], ws, bs.astype(np.float64), 0, stride, relu=relu_a)
    return conv64(x[:, ::stride, ::stride, cx:], w3, b3.astype(np.float64), 0, 1, res=idn, relu=R)


def _nets(ctx, prog, n, monkeypatch):
    """the program as an exact net, an fp16-form net (shortcuts folded where the pattern matches) and an fp16-form net created
    with the knob off"""
    monkeypatch.delenv("POSEPIPE_SPLIT_FOLD", raising=False)
    monkeypatch.delenv("POSEPIPE_SPLIT_FOLD_OFF", raising=False)
    exact, fused = Net(ctx, prog, max_batch=n, numerics="exact"), Net(ctx, prog, max_batch=n, numerics="split_f16")
    monkeypatch.setenv("POSEPIPE_SPLIT_FOLD", "0")         # read when the net is created
    plain = Net(ctx, prog, max_batch=n, numerics="split_f16")
    monkeypatch.delenv("POSEPIPE_SPLIT_FOLD")
    return exact, fused, plain


def _yardstick(y, y_exact, ref, what):
    n = ref.shape[0]
    assert y.shape == ref.shape and np.isfinite(y).all(), what
    scale = np.abs(ref).reshape(n, -1).max(1).reshape(n, 1, 1, 1) + 1e-300
    rms = lambda v: float(np.sqrt(np.mean(((v - ref) / scale) ** 2)))
    mx = lambda v: float(np.abs((v - ref) / scale).max())
    print(f"{what}: rms fused {rms(y):.3e} exact {rms(y_exact):.3e}; max fused {mx(y):.3e} exact {mx(y_exact):.3e}")
    assert rms(y) <= 1.25 * rms(y_exact) + 1e-9, (what, rms(y), rms(y_exact))
    assert mx(y) <= 1.5 * mx(y_exact) + 1e-7, (what, mx(y), mx(y_exact))


def _folds(net):
    return int((net.folded_into() >= 0).sum())


# (n, h, w, cx = shortcut's input channels, ch = conv3's, cout, shortcut stride):
#   stride 1, 260 pixels per sample: the 256-pixel tile straddles samples and the last tile is ragged;
#   stride 2 from an input that is odd on both axes, unequal segments (8 + 4 stages);
#   unequal segments (16 + 1 stages) onto 512 output channels = four channel columns: the column remap of the 1-D launch
CASES = [(2, 20, 13, 64, 64, 256, 1), (3, 23, 17, 128, 64, 256, 2), (2, 20, 13, 16, 256, 512, 1)]


@pytest.mark.parametrize("case", CASES)
def test_folded_shortcut_is_as_accurate_as_the_float32_chain(ctx, monkeypatch, case):
    n, h, w, cx, ch, cout, stride = case
    rng = np.random.default_rng(sum(case))
    prog, wts = _pair_program(h, w, cx, ch, cout, stride, rng)
    exact, fused, plain = _nets(ctx, prog, n, monkeypatch)
    assert _folds(fused) == 1 and _folds(plain) == 0 and _folds(exact) == 0
    i_sc, i_c3 = prog.op_names.index("shortcut"), prog.op_names.index("conv3")
    assert fused.folded_into()[i_sc] == i_c3 and fused.conv_kinds()[i_c3] == 2 and fused.conv_kinds()[i_sc] == 2
    # heavy-tailed activations, samples at magnitudes 1e-3 .. 1e2
    x = (rng.standard_normal((n, h, w, cx + ch)) * np.exp(2 * rng.standard_normal((n, h, w, cx + ch))) *
         (10.0 ** np.linspace(-3, 2, n)).reshape(-1, 1, 1, 1)).astype(np.float32)
    ref = _ref_pair(x, stride, cx, wts)
    ye, yf, yp = exact.forward(x), fused.forward(x), plain.forward(x)
    assert not np.array_equal(yf, yp) and not np.array_equal(yf, ye), "the folded product did not run"
    _yardstick(yf, ye, ref, f"fused {case}")
    _yardstick(yp, ye, ref, f"two launches {case}")
    assert np.array_equal(fused.forward(x), yf)            # (a second run: the maxima are reset per run)


def test_joint_scale_of_the_two_segments(ctx, monkeypatch):
    """one activation scale per sample for BOTH inputs: h ~1e4 below x, x ~1e4 below h, an all-zero x, an all-zero h"""
    n, h, w, cx, ch, cout = 4, 20, 13, 64, 64, 256
    rng = np.random.default_rng(77)
    prog, wts = _pair_program(h, w, cx, ch, cout, 1, rng)
    exact, fused, _ = _nets(ctx, prog, n, monkeypatch)
    assert _folds(fused) == 1
    x = (rng.standard_normal((n, h, w, cx + ch)) * np.exp(rng.standard_normal((n, h, w, cx + ch)))).astype(np.float32)
    x[0, ..., cx:] *= 1e-4
    x[1, ..., :cx] *= 1e-4
    x[2, ..., :cx] = 0
    x[3, ..., cx:] = 0
    ref = _ref_pair(x, 1, cx, wts)
    _yardstick(fused.forward(x), exact.forward(x), ref, "joint scale")


def test_knob_off_classes_and_exact_nets_are_not_rewritten(ctx, monkeypatch):
    """POSEPIPE_SPLIT_FOLD=0 and the per-class list keep the two launches -- the one-segment kernel, same bits either way; an exact
    net is never rewritten and does not see the knobs"""
    n, h, w, cx, ch, cout = 2, 20, 13, 64, 64, 256
    rng = np.random.default_rng(5)
    prog, _ = _pair_program(h, w, cx, ch, cout, 1, rng)
    x = rng.standard_normal((n, h, w, cx + ch)).astype(np.float32)
    exact, fused, plain = _nets(ctx, prog, n, monkeypatch)
    monkeypatch.setenv("POSEPIPE_SPLIT_FOLD_OFF", f"{ch}+{cx}")
    by_class = Net(ctx, prog, max_batch=n, numerics="split_f16")
    monkeypatch.setenv("POSEPIPE_SPLIT_FOLD_OFF", f"128+64,{ch}+{cx}@{h}x{w}")
    by_class_map = Net(ctx, prog, max_batch=n, numerics="split_f16")
    monkeypatch.setenv("POSEPIPE_SPLIT_FOLD_OFF", f"{ch}+{cx}@{h + 1}x{w}")
    other_map = Net(ctx, prog, max_batch=n, numerics="split_f16")
    monkeypatch.delenv("POSEPIPE_SPLIT_FOLD_OFF")
    monkeypatch.setenv("POSEPIPE_SPLIT_FOLD", "0")
    exact_off = Net(ctx, prog, max_batch=n, numerics="exact")
    bf16 = Net(ctx, prog, max_batch=n, numerics="split_bf16")
    monkeypatch.delenv("POSEPIPE_SPLIT_FOLD")
    bf16_on = Net(ctx, prog, max_batch=n, numerics="split_bf16")
    assert [_folds(m) for m in (exact, fused, plain, by_class, by_class_map, other_map, exact_off, bf16, bf16_on)] == [0, 1, 0, 0, 0, 1, 0, 0, 0]
    yp = plain.forward(x)
    assert np.array_equal(by_class.forward(x), yp) and np.array_equal(by_class_map.forward(x), yp)
    assert np.array_equal(other_map.forward(x), fused.forward(x)) and not np.array_equal(fused.forward(x), yp)
    assert np.array_equal(exact.forward(x), exact_off.forward(x))
    assert np.array_equal(bf16.forward(x), bf16_on.forward(x))
    assert (exact.conv_kinds() == exact_off.conv_kinds()).all() and (plain.conv_kinds() == fused.conv_kinds()).all()


def test_patterns_that_are_not_folded(ctx, monkeypatch):
    """a second reader of the shortcut tensor, a shortcut with ReLU, a residual read with a shift (FPN's top-down add): two launches,
    the bits of a net created with the knob off"""
    n, h, w, cx, ch, cout = 2, 20, 13, 64, 64, 256
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n, h, w, cx + ch)).astype(np.float32)
    progs = [_pair_program(h, w, cx, ch, cout, 1, rng, second_reader=True)[0], _pair_program(h, w, cx, ch, cout, 1, rng, relu_a=R)[0]]
    # FPN: the 1x1 "shortcut" lives on the coarser map and conv3 reads it at (y >> 1, x >> 1)
    pb = ProgramBuilder()
    inp = pb.buf(h, w, cx + ch, name="input")
    xs = pb.maxpool(inp, 1, 2, 0, c=cx, in_c_off=0, name="x")                 # [10][7][cx]
    hs = pb.maxpool(inp, 1, 1, 0, c=ch, in_c_off=cx, name="h")
    top = pb.conv(xs, _w(rng, cout, cx), rng.standard_normal(cout).astype(np.float32), name="shortcut")
    pb.conv(hs, _w(rng, cout, ch), rng.standard_normal(cout).astype(np.float32), relu=R, res1=top, res1_shift=1,
            out=pb.buf(h, w, cout, name="output"), name="conv3")
    progs.append(pb.build())
    for prog in progs:
        _, fused, plain = _nets(ctx, prog, n, monkeypatch)
        assert _folds(fused) == 0 and fused.conv_kinds()[prog.op_names.index("conv3")] == 2
        assert np.array_equal(fused.forward(x), plain.forward(x))


def test_folded_op_inside_a_program(ctx, monkeypatch):
    """a bottleneck as the models emit it (conv1, conv2, shortcut, conv3) followed by an fp16-form 3x3: the folded op reads a tensor
    with fused maxima (conv2's) and one with a stand-alone pass (x), and its own y_amax feeds the 3x3's scale.  One launch fewer."""
    n, h, w, cx, planes, cout = 3, 23, 17, 64, 64, 256
    rng = np.random.default_rng(21)
    pb = ProgramBuilder()
    inp = pb.buf(h, w, cx, name="input")
    xs = pb.maxpool(inp, 1, 1, 0, name="x")
    wts = [(_w(rng, planes, cx), rng.standard_normal(planes).astype(np.float32)), (_w(rng, planes, planes, 3), rng.standard_normal(planes).astype(np.float32)),
           (_w(rng, cout, cx), rng.standard_normal(cout).astype(np.float32)), (_w(rng, cout, planes), rng.standard_normal(cout).astype(np.float32)),
           (_w(rng, 64, cout, 3), rng.standard_normal(64).astype(np.float32))]
    y = pb.conv(xs, *wts[0], relu=R, name="conv1")
    y = pb.mark_output(pb.conv(y, *wts[1], pad=1, relu=R, name="conv2"), "h")
    idn = pb.conv(xs, *wts[2], name="shortcut")
    y = pb.mark_output(pb.conv(y, *wts[3], relu=R, res1=idn, name="conv3"), "y")
    pb.conv(y, *wts[4], pad=1, out=pb.buf(h, w, 64, name="output"), name="next3x3")
    prog = pb.build()
    exact, fused, plain = _nets(ctx, prog, n, monkeypatch)
    assert _folds(fused) == 1 and _folds(plain) == 0
    launches = lambda net: len(prog.ops) - _folds(net)
    assert launches(fused) == launches(plain) - 1
    assert fused.conv_kinds()[prog.op_names.index("next3x3")] == 2
    x = (rng.standard_normal((n, h, w, cx)) * np.exp(rng.standard_normal((n, h, w, cx))) * (10.0 ** np.linspace(-3, 2, n)).reshape(-1, 1, 1, 1)).astype(np.float32)
    out, mid = {}, {}
    for name, net in (("exact", exact), ("fused", fused), ("plain", plain)):
        out[name] = net.forward(x)
        mid[name] = (net.read("h", n), net.read("y", n))
    # every net against the float64 evaluation of ITS OWN inputs of the op under test
    ref_y = {k: conv64(mid[k][0], wts[3][0], wts[3][1].astype(np.float64), 0, res=conv64(x, wts[2][0], wts[2][1].astype(np.float64), 0), relu=R) for k in mid}
    ref_z = {k: conv64(mid[k][1], wts[4][0], wts[4][1].astype(np.float64), 1) for k in mid}
    rel = lambda y, ref: (y - ref) / (np.abs(ref).reshape(n, -1).max(1).reshape(n, 1, 1, 1) + 1e-300)
    rms, mx = lambda e: float(np.sqrt(np.mean(e ** 2))), lambda e: float(np.abs(e).max())
    # conv3 + shortcut, then the 3x3 behind it, which scales by the maxima the folded op's epilogue tracked: same yardstick
    for what, e_f, e_e in (("conv3 in a program", rel(mid["fused"][1], ref_y["fused"]), rel(mid["exact"][1], ref_y["exact"])),
                           ("3x3 behind it", rel(out["fused"], ref_z["fused"]), rel(out["exact"], ref_z["exact"]))):
        print(f"{what}: rms fused {rms(e_f):.3e} exact {rms(e_e):.3e}; max fused {mx(e_f):.3e} exact {mx(e_e):.3e}")
        assert np.isfinite(e_f).all()
        assert rms(e_f) <= 1.25 * rms(e_e) + 1e-9, (what, rms(e_f), rms(e_e))
        assert mx(e_f) <= 1.5 * mx(e_e) + 1e-7, (what, mx(e_f), mx(e_e))
    # run() in op ranges that cut between the shortcut and conv3 still works (the shortcut's input is unchanged in between)
    i_sc = prog.op_names.index("shortcut")
    fused.forward(x)
    fused.run(n, 0, i_sc + 1)
    fused.run(n, i_sc + 1, len(prog.ops))
    assert np.array_equal(fused.read("output", n), out["fused"])
