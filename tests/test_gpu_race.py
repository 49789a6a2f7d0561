"""Race screen for the hand-synchronised kernels of the default numerics.

conv_split_kernel's 8-wave form and conv_split_gemm_kernel issue `global_load_lds_dwordx4` as raw instructions the compiler cannot
see and order their LDS traffic by COUNTED `s_waitcnt vmcnt(n)` and by barriers placed by hand (csrc/conv_split_*.hip, conv_split_tap.h).  A
miscounted wait or a missing barrier does not fail deterministically: it shows as an occasional wrong tile when the memory
system is busy.  So every such form -- 8-wave tile and stream forms, the 4-wave ring form (RING4), COB 1 and 2, even and odd chunk
counts, conv_split_gemm_kernel<2,4> / <4,2> / <2,2> -- is launched 50 times inside layer programs that run on 4 HIP streams (the forms
overlap each other), WHILE a second context on another thread runs the detector on 1080p frames -- the configuration of
bench.py's timed region (Cascade's detector look-ahead).  Every repetition must reproduce the first one bit for bit, and the first
one must agree with the float32 MFMA kernels.
"""
import threading

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.models import faster_rcnn as fr
from posepipeline_amd.models import synth
from posepipeline_amd.program import Net, ProgramBuilder

pytestmark = pytest.mark.gpu

REPS = 50


def _w(rng, cout, cin, k):
    return (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32), rng.standard_normal(cout).astype(np.float32)


def tap_program(rng, cin, hw):
    """3x3 layers: 8-wave TILE forms straight from the (dense) input -- Cout 256 (two channel blocks per wave), 96 (one) and
    128 --, and conv -> conv chains whose second layer reads a zero-halo buffer (8-wave STREAM form)"""
    pb = ProgramBuilder()
    x = pb.buf(hw, hw, cin, name="input")
    outs = []
    for i, cout in enumerate((256, 96, 128)):
        o = pb.buf(hw, hw, cout, name=f"tile{i}")
        pb.conv(x, *_w(rng, cout, cin, 3), pad=1, relu=L.PP_RELU_LAST, out=o)
        outs.append(f"tile{i}")
    for i, cmid in enumerate((cin, 256)):
        y = pb.conv(x, *_w(rng, cmid, cin, 3), pad=1, relu=L.PP_RELU_LAST)
        y2 = pb.conv(y, *_w(rng, cmid, cmid, 3), pad=1, relu=L.PP_RELU_LAST)
        o = pb.buf(hw, hw, 64, name=f"stream{i}")
        pb.conv(y2, *_w(rng, 64, cmid, 3), pad=1, out=o)
        outs.append(f"stream{i}")
    return pb.build(), outs


def gemm_program(rng, cin, hw):
    """1x1 layers: Cout % 256 == 0 -> conv_split_gemm_kernel<2,4> (from 512 input channels) or <2,2> (256 .. 511), Cout % 128 == 0
    -> <4,2> / <2,2>; chained so that the program has >= 8 ops (4 streams)"""
    pb = ProgramBuilder()
    x = pb.buf(hw, hw, cin, name="input")
    outs = []
    for i, cout in enumerate((256, 384, 128, 512)):
        y = pb.conv(x, *_w(rng, cout, cin, 1), relu=L.PP_RELU_LAST)
        o = pb.buf(hw, hw, 128, name=f"g{i}")
        pb.conv(y, *_w(rng, 128, cout, 1), res1=-1, out=o)
        outs.append(f"g{i}")
    return pb.build(), outs


class _Background:
    """a second context on its own thread: detector passes over 1080p frames until stopped"""

    def __init__(self, device):
        self.stop = threading.Event()
        self.passes = 0
        self.error = None
        self.ready = threading.Event()
        self.t = threading.Thread(target=self._run, args=(device,), daemon=True)

    def _run(self, device):
        try:
            ctx2 = L.Context(device)
            sd = synth.synth_state_dict(fr.faster_rcnn_param_shapes(), seed=2)
            with L.default_numerics("split"):
                det = fr.Detector(ctx2, sd, 1080, 1920, max_frames=4)
            frames = np.random.default_rng(0).integers(0, 256, (4, 1080, 1920, 3)).astype(np.uint8)
            dptr = ctx2.malloc(frames.nbytes)
            ctx2.h2d(dptr, frames)
            first = det.run(None, frames_dev=(dptr, 4))
            self.ready.set()
            while not self.stop.is_set():
                again = det.run(None, frames_dev=(dptr, 4))
                # the detector's own hand-synchronised layers under the same pressure: same detections every pass
                assert all(np.array_equal(a, b) for a, b in zip(first, again)), "detector pass differs from its first pass"
                self.passes += 1
            ctx2.free(dptr)
            det.close()
        except BaseException as e:          # noqa: BLE001 -- reported by the test
            self.error = e
            self.ready.set()

    def __enter__(self):
        self.t.start()
        assert self.ready.wait(300), "the background detector did not start"
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.t.join(300)
        if self.error is not None and exc[0] is None:
            raise self.error


# tap cases: >= 512 workgroups and >= 16 channel chunks select the 8-wave form; 88 x 88 maps do not tile evenly -> stream form on halo buffers
# 48 / 96 input channels: too few chunks for the 8-wave form -> the 4-wave ring form (RING4: single-buffered patch, weights through
# the LDS ring, two workgroups per CU), tile form on 64 x 64 maps, stream form on 44 x 44
CASES = [("tap", 256, 96, 12), ("tap", 272, 88, 16), ("tap", 48, 64, 12), ("tap", 96, 44, 24), ("gemm", 512, 80, 8), ("gemm", 528, 72, 10), ("gemm", 256, 80, 8), ("gemm", 272, 72, 9)]


@pytest.mark.parametrize("kind,cin,hw,batch", CASES)
def test_hand_synchronised_forms_are_deterministic_under_load(ctx, kind, cin, hw, batch):
    rng = np.random.default_rng(cin + hw)
    prog, outs = (tap_program if kind == "tap" else gemm_program)(rng, cin, hw)
    assert len(prog.ops) >= 8                                            # 4 HIP streams inside the program
    x = rng.standard_normal((batch, hw, hw, cin)).astype(np.float32)
    net = Net(ctx, prog, max_batch=batch, numerics="split")
    kinds = net.conv_kinds()
    assert (kinds == 2).sum() >= len(outs), "the split kernels were not selected"
    exact = Net(ctx, prog, max_batch=batch, numerics="exact")
    ref = {k: exact.forward(x, out_name=k) for k in outs}
    exact.close()

    def one_pass():
        first = net.forward(x, out_name=outs[0])
        return {outs[0]: first, **{k: net.read(k, batch) for k in outs[1:]}}
    with _Background(ctx.device) as bg:
        base = one_pass()
        for k in outs:                                                   # the first pass is right (float32-accurate) ...
            assert np.abs(base[k] - ref[k]).max() <= 1e-5 * np.abs(ref[k]).max(), k
            assert not np.array_equal(base[k], ref[k]), k
        for rep in range(REPS):                                          # ... and every later one reproduces it bit for bit
            again = one_pass()
            for k in outs:
                if not np.array_equal(again[k], base[k]):
                    bad = np.argwhere(again[k] != base[k])
                    raise AssertionError(f"{kind} cin {cin}: output {k} differs in repetition {rep}: {len(bad)} elements, first at {bad[0]}")
        passes = bg.passes
    assert passes >= 1, "no detector pass overlapped the repetitions"
