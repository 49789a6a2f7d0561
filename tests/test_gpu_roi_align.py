"""RoIAlign on chosen RoIs (tests/roi_align_cases.py): roi_align_kernel (exact numerics) bit for bit against the oracle's sample loop,
roi_align_sep_kernel (the default numerics) against the same loop in float64, the level cut, and the per-RoI maxima the fp16-form
fc6 scales its input by.  pp_detector_regress runs RoIAlign on caller-supplied boxes over the FPN maps of the last pass; the fixtures
overwrite those maps (Net.buffer + ctx.h2d) with the seeded maps of the cases module.  Every call goes through a NaN-filled `roi_in`,
so a row or a bin the kernel leaves unwritten shows, and so does a write past the call's rows.

The default numerics follow the rule of tests/test_gpu_trades.py: the GPU's error against float64 may be FACTOR = 4 times the deviation
of the oracle's own float32 evaluation from float64, family by family; the ratios are printed."""
import ctypes as C

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.models import faster_rcnn as fr
from posepipeline_amd.models import synth
from tests import roi_align_cases as RC
from tests.test_gpu_detector import synth_frame

pytestmark = pytest.mark.gpu
FACTOR = 4.0
f32, f64 = np.float32, np.float64
GUARD = 4                    # rows of roi_in past the call's that must stay NaN


class Rig:
    """a detector whose last pass's FPN maps are the cases module's"""

    def __init__(self, ctx, numerics):
        self.ctx = ctx
        sd = synth.synth_state_dict(fr.faster_rcnn_param_shapes(), seed=2)
        # the weights matter to the batch-path test alone, which needs frames with FEWER than MAX_ROIS proposals: every anchor grows
        # twentyfold (dw = dh = 3, no other delta), neighbouring proposals overlap almost wholly, and the RPN's NMS leaves a few hundred
        sd["detector.rpn_head.rpn_cls.weight"] = (sd["detector.rpn_head.rpn_cls.weight"] * 0.5).astype(f32)
        sd["detector.rpn_head.rpn_reg.weight"] = np.zeros_like(sd["detector.rpn_head.rpn_reg.weight"])
        sd["detector.rpn_head.rpn_reg.bias"] = np.tile(np.array([0, 0, 3, 3], f32), 3)
        rng = np.random.default_rng(7)
        self.frames = np.stack([synth_frame(rng, RC.SRC_H, RC.SRC_W) for _ in range(RC.N_FRAMES)])
        self.det = fr.Detector(ctx, sd, RC.SRC_H, RC.SRC_W, max_frames=RC.N_FRAMES, numerics=numerics)
        assert self.det.net_a.numerics == self.det.net_b.numerics == numerics
        assert (self.det.nh, self.det.nw, self.det.hp, self.det.wp) == RC.INPUT_SIZE
        # the per-RoI maxima: the address is stable, and the pass that follows makes and consumes its own promise
        p = C.c_void_p()
        L.check(ctx.lib.pp_net_input_amax(self.det.net_b.handle, self.det.prog_b.named["roi_in"], C.byref(p)), "pp_net_input_amax")
        self.amax_ptr = p.value
        self.roi_in = self.det.net_b.buffer("roi_in")[0]
        self.load_maps()

    def load_maps(self):
        """one pass (the maps become resident), then p2 .. p5 of both frames overwritten"""
        self.det.run(self.frames)
        for lv, (h, w) in enumerate(RC.MAP_HW):
            dptr, nbytes, dims = self.det.net_a.buffer(f"p{lv + 2}")
            assert dims == (h, w, RC.C) and nbytes == h * w * RC.C * 4
            self.ctx.h2d(dptr, np.stack([RC.feature_maps(f)[lv] for f in range(RC.N_FRAMES)]))

    def align(self, frame, rois):
        """RoIAlign of `rois` (input pixels) on frame `frame` -> roi_in rows [0, n + GUARD), rows [0, n + GUARD) NaN before the call"""
        n = len(rois)
        self.ctx.h2d(self.roi_in, np.full((n + GUARD, 7, 7, RC.C), np.nan, f32))
        self.det.regress(frame, RC.source_boxes(rois))
        return self.det.net_b.read("roi_in", n + GUARD)

    def maxima(self, n):
        out = np.zeros(n, np.uint32)
        self.ctx.d2h(out, self.amax_ptr)
        return out


@pytest.fixture(scope="module", autouse=True)
def _release_the_cases():
    """the cached maps and references (about 150 MB of host memory) go with the module"""
    yield
    RC.feature_maps.cache_clear()
    RC.reference.cache_clear()


@pytest.fixture(scope="module")
def exact(ctx):
    return Rig(ctx, "exact")


@pytest.fixture(scope="module")
def split(ctx):
    return Rig(ctx, "split")


def check_rows_written(got, n, what):
    assert not np.isnan(got[:n]).any(), f"{what}: NaN left in the call's rows (bins {np.argwhere(np.isnan(got[:n]).any(axis=-1))[:4].tolist()})"
    assert np.isnan(got[n:]).all(), f"{what}: rows past the call's were written"


@pytest.mark.parametrize("name", RC.FAMILY_NAMES)
def test_exact_kernel_is_the_oracle_bit_for_bit(exact, name):
    rois = RC.families()[name]
    n = len(rois)
    for frame in range(RC.N_FRAMES):
        ref = RC.reference(frame, name)
        got = exact.align(frame, rois)
        check_rows_written(got, n, f"{name} frame {frame}")
        bad = np.flatnonzero((got[:n].view(np.uint32) != ref["ref32"].view(np.uint32)).any(axis=(1, 2, 3)))
        assert bad.size == 0, (name, frame, bad.tolist(), rois[bad[0]].tolist(), float(np.abs(got[bad[0]] - ref["ref32"][bad[0]]).max()))


@pytest.mark.parametrize("name", RC.FAMILY_NAMES)
def test_separable_kernel_against_float64(split, name):
    """zero rows exact; every other family err = max |got - ref64| <= 4 x dev = max |ref32 - ref64|, both over the family"""
    rois = RC.families()[name]
    n = len(rois)
    for frame in range(RC.N_FRAMES):
        ref = RC.reference(frame, name)
        got = split.align(frame, rois)
        check_rows_written(got, n, f"{name} frame {frame}")
        zero = ~ref["ref64"].any(axis=(1, 2, 3))
        assert not got[:n][zero].any(), (name, frame, np.flatnonzero(got[:n][zero].any(axis=(1, 2, 3))).tolist())
        # bins the reference has no sample for are zero in nonzero rows, too
        assert not got[:n][~ref["ref64"].any(axis=-1)].any(), (name, frame)
        if name in RC.ZERO_FAMILIES:
            assert zero.all()
            continue
        e = np.abs(got[:n].astype(f64) - ref["ref64"]).max(axis=(1, 2, 3))
        d = np.abs(ref["ref32"].astype(f64) - ref["ref64"]).max(axis=(1, 2, 3))
        for lv in sorted(set(ref["levels"].tolist())):
            m = ref["levels"] == lv
            if d[m].max() > 0:
                print(f"  {name} frame {frame} level {lv}: {int(m.sum())} RoIs, GPU error {e[m].max():.3e}, float32 deviation {d[m].max():.3e}, "
                      f"ratio {e[m].max() / d[m].max():.2f}")
        err, dev = float(e.max()), float(d.max())
        assert dev > 0, (name, frame)
        print(f"{name} frame {frame}: GPU error {err:.3e}, float32-on-CPU deviation {dev:.3e}, ratio {err / dev:.2f}")
        assert err <= FACTOR * dev, (name, frame, err, dev, int(e.argmax()), rois[int(e.argmax())].tolist())


@pytest.mark.parametrize("name", RC.FAMILY_NAMES)
def test_per_roi_maxima(split, name):
    """word r of the maxima array is the bit pattern of max |roi_in[r]|, 0 for a zero row: what the fp16-form fc6 scales row r by"""
    if split.det.net_b.split_kind != "split_f16":
        pytest.skip("the per-sample activation scale belongs to the fp16 form")
    assert split.amax_ptr
    rois = RC.families()[name]
    n = len(rois)
    for frame in range(RC.N_FRAMES):
        split.ctx.h2d(split.amax_ptr, np.full(n + GUARD, 0x7fc00000, np.uint32))
        got = split.align(frame, rois)
        check_rows_written(got, n, f"{name} frame {frame}")
        words = split.maxima(n + GUARD)
        want = np.abs(got[:n]).max(axis=(1, 2, 3)).astype(f32).view(np.uint32)
        assert np.array_equal(words[:n], want), (name, frame, np.flatnonzero(words[:n] != want).tolist())
        assert (words[n:] == 0x7fc00000).all()
        zero = ~RC.reference(frame, name)["ref64"].any(axis=(1, 2, 3))
        assert (words[:n][zero] == 0).all() and (words[:n][~zero] != 0).all()


def test_batch_path_rows_past_the_proposals(split):
    """pp_detector_run: rows of roi_in past a frame's proposal count are zero and their maxima words 0; the rows before carry their
    own maxima"""
    det = split.det
    m = det.MAX_ROIS
    try:
        split.ctx.h2d(split.roi_in, np.full((RC.N_FRAMES * m, 7, 7, RC.C), np.nan, f32))
        if split.amax_ptr:
            split.ctx.h2d(split.amax_ptr, np.full(RC.N_FRAMES * m, 0x7fc00000, np.uint32))
        _, props = det.run(split.frames, want_proposals=True)
        got = det.net_b.read("roi_in", RC.N_FRAMES * m).reshape(RC.N_FRAMES, m, -1)
        counts = [len(p) for p in props]
        print(f"proposals per frame: {counts}")
        assert 0 < min(counts) and max(counts) < m, "a frame leaves no row past its proposals"
        assert not np.isnan(got).any()
        for f, n in enumerate(counts):
            assert n > 0 and got[f, :n].any() and not got[f, n:].any()
        if det.net_b.split_kind == "split_f16":
            words = split.maxima(RC.N_FRAMES * m).reshape(RC.N_FRAMES, m)
            assert np.array_equal(words, np.abs(got).max(axis=2).astype(f32).view(np.uint32))
            for f, n in enumerate(counts):
                assert (words[f, n:] == 0).all()
    finally:
        split.load_maps()
