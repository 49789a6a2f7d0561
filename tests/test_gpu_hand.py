"""The hand stage on the GPU: PP_OP_BILINEAR_ADD and the HRNetv2-W18 program bit for bit against tests/hand_ref.py (exact
numerics, the suite's autouse fixture), the default (fp16-split) numerics against the exact ones in decoded pixels, and the
`mmpose_HPE` wrapper through the table shim against the CPU chain."""
import datetime

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd import ops
from posepipeline_amd.models import hrnetv2, synth
from posepipeline_amd.program import Net, ProgramBuilder
from tests import hand_ref

pytestmark = pytest.mark.gpu


# ---- 1. the op ---------------------------------------------------------------------------------------------------------------
# (batch, out h, out w, c, [up_log2 of the coarse inputs], res1, relu, (out buffer channels, out_c_off) or None)
# (the kernel is a template over its index type; these launches take the 32-bit instantiation -- the 64-bit one is the same code and
# starts at float4 indices past 2^31, a 32 GiB buffer, which no quick test can hold)
OP_CASES = [
    (1, 6, 10, 4, [1], False, False, None),              # one input, x2, one block, odd coarse map 3x5
    (3, 8, 24, 20, [2, 3], True, True, None),            # two inputs, x4 and x8 (a 1x3 coarse map), residual, ReLU, batch 3
    (2, 16, 8, 36, [1, 2, 3], True, True, None),         # the full fuse layer of branch 0: three inputs; two blocks
    (2, 8, 16, 12, [3], False, False, (32, 8)),          # a channel slice of a wider buffer, x8 from a 1x2 map
    (2, 12, 20, 8, [2, 1], True, False, (24, 16)),       # slice + residual, the last slice of the buffer, terms in another order
    (5, 24, 40, 8, [1, 2], False, True, None),           # 1920 float4 per sample: blocks (2048 float4) straddle samples
    (1, 64, 64, 4, [3, 1, 2], True, True, None),         # square, two blocks within one sample
]


@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "n%d_%dx%dx%d_u%s%s%s%s" % (c[0], c[1], c[2], c[3], "".join(map(str, c[4])),
                                                                                      "_res" if c[5] else "", "_relu" if c[6] else "",
                                                                                      "_slice" if c[7] else ""))
def test_bilinear_add_op_bit_exact(ctx, case):
    n, h, w, c, ups, has_res, relu, slc = case
    rng = np.random.default_rng(n * 1000 + h * 10 + c)
    pb = ProgramBuilder()
    ins = [pb.buf(h >> u, w >> u, c, name=f"t{i}") for i, u in enumerate(ups)]
    res = pb.buf(h, w, c, name="res") if has_res else -1
    cbuf, coff = slc if slc else (c, 0)
    out = pb.buf(h, w, cbuf, name="out")
    pb.bilinear_add(ins[0], up_log2=ups[0], res1=res, relu=L.PP_RELU_LAST if relu else L.PP_RELU_NONE,
                    more=list(zip(ins[1:], ups[1:])), out=out, out_c_off=coff)
    prog = pb.build()
    assert len(prog.ops) == 1 and prog.ops[0].type == L.PP_OP_BILINEAR_ADD == 10
    net = Net(ctx, prog, max_batch=n)
    data = [(rng.standard_normal((n, h >> u, w >> u, c)) * 3).astype(np.float32) for u in ups]
    for i, d in enumerate(data):
        ctx.h2d(net.buffer(f"t{i}")[0], d)
    r = rng.standard_normal((n, h, w, c)).astype(np.float32) if has_res else None
    if has_res:
        ctx.h2d(net.buffer("res")[0], r)
    sentinel = rng.standard_normal((n, h, w, cbuf)).astype(np.float32)
    ctx.h2d(net.buffer("out")[0], sentinel)
    net.run(n)
    got = net.read("out", n)
    want = sentinel.copy()
    want[..., coff:coff + c] = hand_ref.bilinear_add(list(zip(data, ups)), res1=r, relu_last=relu)
    assert np.array_equal(got[..., coff:coff + c], want[..., coff:coff + c])
    assert np.array_equal(got, want)                      # the channels outside the slice are untouched
    if relu:
        assert (got[..., coff:coff + c] == 0).any() and (got[..., coff:coff + c] > 0).any()
    net.close()


def test_bilinear_add_op_is_validated(ctx):
    pb = ProgramBuilder()
    t = pb.buf(4, 4, 8, name="t")
    pb.bilinear_add(t, up_log2=1)
    prog = pb.build()
    prog.ops[0].up_log2 = 2                                # 4x4 << 2 is not the 8x8 out buffer
    with pytest.raises(L.PosePipeHipError, match="bilinear_add"):
        Net(ctx, prog, max_batch=1)
    prog.ops[0].up_log2 = 1
    prog.ops[0].res2 = prog.ops[0].in_
    with pytest.raises(L.PosePipeHipError, match="res2"):
        Net(ctx, prog, max_batch=1)


# ---- 2. the network --------------------------------------------------------------------------------------------------------------
def test_hrnetv2_program_bit_exact(ctx):
    spec = hrnetv2.HRNetV2Spec(18, 21, 96, 64)             # non-square; branch maps 24x16, 12x8, 6x4, 3x2
    sd = synth.synth_state_dict(hrnetv2.hrnetv2_param_shapes(spec), seed=3)
    net = Net(ctx, hrnetv2.build_hrnetv2_program(spec, sd), max_batch=3)
    assert net.numerics == "exact"
    x = np.random.default_rng(0).standard_normal((3, 3, 96, 64)).astype(np.float32)
    xin = np.zeros((3, 96, 64, 4), np.float32)
    xin[..., :3] = np.transpose(x, (0, 2, 3, 1))
    hm = net.forward(xin).reshape(3, 21, 24, 16)
    ref = hand_ref.HRNetV2Ref(sd, 18).forward(x)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 1e-3
    assert np.array_equal(hm, ref), np.abs(hm - ref).max() / np.abs(ref).max()
    net.close()


# ---- 3. default numerics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("post,shift", [("unbiased", True), ("udp", False)])
def test_hand_stage_default_numerics_vs_exact(ctx, post, shift):
    """The fused hand stage on the default (fp16-split) kernels against the exact ones, same crops, in decoded pixels: the
    project's contract, 1e-3 px (BASELINE.json), on the smooth weights of tests/test_gpu_parity_modes.py.  The amax plan is
    exercised: the fuse passes and the four slice writers of the concatenation track the maxima the split convolutions scale
    by; an input scaled by 1e4 must not overflow float16 anywhere."""
    spec = hrnetv2.hrnetv2_w18_256x256()
    sd = synth.smooth_state_dict(hrnetv2.hrnetv2_param_shapes(spec), seed=11)
    prog = hrnetv2.build_hrnetv2_program(spec, sd)
    n = 4
    x = synth.blob_crops(np.random.default_rng(5), n, spec.in_h, spec.in_w)
    # (cx, cy, sx, sy) of hand boxes in a 1080p frame: square, side = box * 1.25 / 200
    cs = np.array([[960.0, 540.0, 1.5, 1.5], [300.5, 700.25, 1.1, 1.1], [1700.0, 400.0, 2.2, 2.2], [1020.0, 750.0, 12.75, 12.75]], np.float32)
    kps, hms, big = {}, {}, {}
    for numerics in ("exact", "split"):
        net = Net(ctx, prog, max_batch=2 * n, numerics=numerics)
        assert net.numerics == numerics and (numerics == "split") == bool((net.conv_kinds() == 2).any())
        td = ops.TopDown(net, 21, flip_perm=np.arange(21, dtype=np.int32), shift_heatmap=shift, post=post, blur_kernel=11)
        kps[numerics] = td.run_precropped(x, cs)
        hms[numerics] = net.read("output", 2 * n)
        td.run_precropped(x * np.float32(1e4), cs)
        big[numerics] = net.read("output", 2 * n)
        td.close()
        net.close()
    assert hms["exact"].min() > 0 and np.isfinite(hms["exact"]).all()          # well-conditioned by construction
    assert not np.array_equal(hms["split"], hms["exact"]), "the split kernels did not run"
    gap_hm = np.abs(hms["split"] - hms["exact"]).max() / np.abs(hms["exact"]).max()
    d = np.abs(kps["split"][:, :, :2] - kps["exact"][:, :, :2]).max(axis=2)
    print(f"[{post}] HRNetv2-W18 256x256 split vs exact: {d.size} joints, max deviation {d.max():.2e} px, heat-maps {gap_hm:.2e} of range")
    assert d.max() <= 1e-3, d
    assert np.abs(kps["split"][:, :, 2] - kps["exact"][:, :, 2]).max() <= 1e-5 * np.abs(kps["exact"][:, :, 2]).max()
    # no fp16 overflow at 1e4 times the input: finite, and the same maps up to the scale
    for numerics in ("exact", "split"):
        assert np.isfinite(big[numerics]).all()
    assert np.abs(big["split"] - big["exact"]).max() <= 2e-5 * np.abs(big["exact"]).max()


# ---- 4. the wrapper ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand_clip(tmp_path_factory):
    """a 3-frame 1080p clip and a Halpe track whose hands sit on bright textured patches; frame 1's right hand is at the left
    edge, so its box is the fallback [0, 0, 2040, 1500] -- a crop that is mostly outside the frame"""
    from posepipeline_amd import video
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, (3, 1080, 1920, 3)).astype(np.uint8)
    kp = np.zeros((3, 136, 3))
    kp[:, :, 2] = 0.9
    kp[:, :94, :2] = 500.0
    centres = {(0, "l"): (600, 400), (0, "r"): (1300, 700), (1, "l"): (900, 300), (1, "r"): (40, 600), (2, "l"): (1500, 250),
               (2, "r"): (400, 850)}
    for (t, side), (cx, cy) in centres.items():
        sl = slice(94, 115) if side == "l" else slice(115, 136)
        kp[t, sl, :2] = np.array([cx, cy]) + rng.uniform(-70, 70, (21, 2))
        y0, y1, x0, x1 = max(cy - 90, 0), cy + 90, max(cx - 90, 0), cx + 90
        frames[t, y0:y1, x0:x1] = np.clip(rng.normal(170, 40, (y1 - y0, x1 - x0, 3)), 0, 255).astype(np.uint8)
    path = str(tmp_path_factory.mktemp("hand") / "clip.ppvid")
    video.write_ppvid(path, frames, fps=30.0)
    return path, frames, kp


@pytest.mark.parametrize("method,post", [("HRNet_dark", "unbiased"), ("HRNet_udp", "udp")])
def test_hand_wrapper_through_the_tables(ctx, hand_clip, monkeypatch, method, post):
    """HandBbox.populate -> HandPoseEstimation.populate (-> mmpose_HPE) on the table shim against the CPU chain: hand boxes ->
    oracle crop -> hand_ref -> oracle decode.  Same equality as the body wrapper's test (tests/test_gpu_pipeline.py): scores
    bit for bit, positions within 1e-3 px.  A 128x128 member of the family keeps the CPU side to a few seconds."""
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    from posepipeline_amd import djshim, pipeline as pl
    from posepipeline_amd.wrappers import hand_estimation as he
    path, frames, kp = hand_clip
    djshim.reset()
    small = lambda k: hrnetv2.HRNetV2Spec(18, k, 128, 128)      # noqa: E731
    monkeypatch.setitem(he._METHODS, method, (small,) + he._METHODS[method][1:])
    he._cache.clear()
    vkey = {"video_project": "test", "filename": "hands"}
    pl.Video().insert1({**vkey, "video": path, "start_time": datetime.datetime(2024, 1, 1)})
    pl.TopDownPerson().insert1({**vkey, "tracking_method": 5, "video_subject_id": 0, "top_down_method": 2, "keypoints": kp})
    bkey = {**vkey, "detection_method": 1}
    pl.HandBboxMethod().insert1(bkey)
    pl.HandBbox().populate(bkey)
    boxes = np.array((pl.HandBbox & bkey).fetch1("bboxes"))
    assert boxes.shape == (3, 2, 4)
    fb = (boxes == np.array([0.0, 0.0, 2040.0, 1500.0])).all(axis=2)
    assert fb.tolist() == [[False, False], [True, False], [False, False]]
    ekey = {**bkey, "estimation_method": {"HRNet_dark": 3, "HRNet_udp": 4}[method]}
    pl.HandPoseEstimationMethod().insert1(ekey)
    pl.HandPoseEstimation().populate(ekey)
    k2 = (pl.HandPoseEstimation & ekey).fetch1("keypoints_2d")
    assert k2.shape == (3, 42, 3) and k2.dtype == np.float32
    assert np.array_equal(k2, he.mmpose_HPE(ekey, method))
    spec = small(21)
    sd = synth.synth_state_dict(hrnetv2.hrnetv2_param_shapes(spec), seed=1)
    ref = hand_ref.hand_chain(sd, spec, frames, boxes, post)
    assert np.array_equal(k2[:, :, 2], ref[:, :, 2])                             # scores bit-exact
    err = np.abs(k2[:, :, :2] - ref[:, :, :2]).max()
    assert err <= 1e-3, err                                                      # north_star tolerance, px
    # row order: rows 0-20 belong to the first (right-hand) box, 21-41 to the second -- swapping the boxes swaps the halves
    stage = he._cache[(method, 0)]
    swapped = stage.run(frames[:1], boxes[:1, ::-1])
    assert np.array_equal(swapped[0, :21], k2[0, 21:]) and np.array_equal(swapped[0, 21:], k2[0, :21])
    he._cache.clear()
    djshim.reset()
