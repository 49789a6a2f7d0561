"""The hand stage on the CPU: hand boxes against the reference's output, module paths and tables of the shim, the float32
bilinear restatement against torch in float64, and the HRNetv2-W18 model (parameter inventory, program, CPU restatement
against an independently assembled torch float64 model).  The GPU side is tests/test_gpu_hand.py."""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from posepipeline_amd import _lib as L
from posepipeline_amd import djshim, pipeline as pl
from posepipeline_amd.models import hrnet, hrnetv2, synth
from tests import hand_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand_bbox.npz")


@pytest.fixture(autouse=True)
def clean():
    djshim.reset()
    yield
    djshim.reset()


# ---- 1. hand boxes == the reference's, exactly ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_hand_boxes_equal_the_reference(case):
    from posepipeline_amd.wrappers.hand_bbox import make_bbox_from_keypoints
    g = np.load(GOLDEN)
    kp, ref = g[f"kp_{case}"], g[f"boxes_{case}"]
    w, h = (int(v) for v in g[f"wh_{case}"])
    boxes = make_bbox_from_keypoints(kp) if (w, h) == (120, 120) else make_bbox_from_keypoints(kp, width=w, height=h)
    # the contract: a per-frame list [right (4,), left (4,)] of xyxy float64
    assert isinstance(boxes, list) and len(boxes) == len(kp)
    for fr in boxes:
        assert isinstance(fr, list) and len(fr) == 2
        assert all(isinstance(b, np.ndarray) and b.shape == (4,) and b.dtype == np.float64 for b in fr)
    got = np.array(boxes)
    assert got.shape == ref.shape and (got == ref).all()
    # the fixture carries the cases the contract is about (asserted on the reference's output when it was generated)
    fb = (ref == np.array([0.0, 0.0, 2040.0, 1500.0])).all(axis=2)
    assert (~fb).all(axis=1).sum() >= len(kp) // 2 and (fb[:, 0] & ~fb[:, 1]).any() and (~fb[:, 0] & fb[:, 1]).any() and fb[5].all()
    # right hand = the last 21 joints
    i = int(np.flatnonzero(~fb.any(axis=1))[0])
    assert got[i, 0, 0] == kp[i, -21:, 0].min() - w / 2 and got[i, 1, 3] == kp[i, -42:-21, 1].max() + h / 2


# ---- 2. module paths, tables, populate ----------------------------------------------------------------------------------------
def test_module_paths_and_table_exports():
    import pose_pipeline
    import pose_pipeline.wrappers.hand_bbox as hb
    import pose_pipeline.wrappers.hand_estimation as he
    import posepipeline_amd.wrappers.hand_bbox as hb2
    import posepipeline_amd.wrappers.hand_estimation as he2
    assert hb is hb2 and he is he2
    from pose_pipeline import (HandBbox, HandBboxMethod, HandBboxMethodLookup, HandPoseEstimation, HandPoseEstimationMethod,  # noqa: F401
                               HandPoseEstimationMethodLookup)
    assert HandBbox is pl.HandBbox and HandPoseEstimation is pl.HandPoseEstimation
    for n in ("HandBboxMethodLookup", "HandBboxMethod", "HandBbox", "HandPoseEstimationMethodLookup", "HandPoseEstimationMethod",
              "HandPoseEstimation"):
        assert n in pose_pipeline.__all__
    assert pl.HandBboxMethodLookup().fetch(as_dict=True) == [{"detection_method": 0, "detection_method_name": "RTMDet"},
                                                             {"detection_method": 1, "detection_method_name": "TopDown"}]
    rows = {r["estimation_method"]: r["estimation_method_name"] for r in pl.HandPoseEstimationMethodLookup().fetch(as_dict=True)}
    assert rows == {-1: "Halpe", 0: "RTMPoseHand5", 1: "RTMPoseCOCO", 2: "freihand", 3: "HRNet_dark", 4: "HRNet_udp"}
    assert pl.HandBbox.primary_key == ["video_project", "filename", "detection_method"]
    assert pl.HandBbox.heading[-2:] == ["num_boxes", "bboxes"]
    assert pl.HandPoseEstimation.primary_key == pl.HandBbox.primary_key + ["estimation_method"]
    assert pl.HandPoseEstimation.heading[-1] == "keypoints_2d"
    names = (pl.HandPoseEstimationMethodLookup & {"estimation_method": 4}).joint_names()
    assert len(names) == 42 and names[0] == "wrist_r" and names[21] == "wrist_l" and names[41] == "tip5_l"
    assert (pl.HandPoseEstimationMethodLookup & {"estimation_method": -1}).joint_names() == names
    rhd = (pl.HandPoseEstimationMethodLookup & {"estimation_method": 3}).joint_names()
    assert len(rhd) == 21 and rhd[:5] == ["Wrist", "TIP1", "IP1", "MCP1", "CMC1"]


def _halpe_rows(vkey):
    """a Halpe track stored as the 2D stage stores it, next to a COCO track of the same person (top_down_method 0)"""
    kp = np.load(GOLDEN)["kp_a"]
    pkey = {**vkey, "tracking_method": 5, "video_subject_id": 0}
    pl.TopDownPerson().insert1({**pkey, "top_down_method": 0, "keypoints": np.zeros((len(kp), 17, 3))})
    pl.TopDownPerson().insert1({**pkey, "top_down_method": 2, "keypoints": kp})
    return kp


def test_populate_hand_tables_halpe():
    import datetime
    vkey = {"video_project": "p", "filename": "f"}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 5, 1)})
    kp = _halpe_rows(vkey)
    # the HandBbox key carries detection_method, which TopDownPerson lacks; it lacks tracking_method / video_subject_id
    bkey = {**vkey, "detection_method": 1}
    assert (pl.TopDownPerson & bkey & "top_down_method=2").fetch1("keypoints").shape == (len(kp), 136, 3)
    pl.HandBboxMethod().insert1(bkey)
    pl.HandBbox().populate(bkey)
    num_boxes, bboxes = (pl.HandBbox & bkey).fetch1("num_boxes", "bboxes")
    assert num_boxes == 2 and (np.array(bboxes) == np.load(GOLDEN)["boxes_a"]).all()
    ekey = {**bkey, "estimation_method": -1}
    pl.HandPoseEstimationMethod().insert1(ekey)
    pl.HandPoseEstimation().populate(ekey)
    k2 = (pl.HandPoseEstimation & ekey).fetch1("keypoints_2d")
    assert k2.shape == (len(kp), 42, 3)
    assert np.array_equal(k2[:, :21], kp[:, 115:136]) and np.array_equal(k2[:, 21:], kp[:, 94:115])     # right 21, then left 21


def test_unbuilt_methods_raise():
    import datetime
    from posepipeline_amd.wrappers import hand_bbox, hand_estimation
    vkey = {"video_project": "p", "filename": "f"}
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 5, 1)})
    _halpe_rows(vkey)
    with pytest.raises(NotImplementedError, match="RTMDet"):
        hand_bbox.mmpose_hand_det(vkey, "RTMDet")
    pl.HandBboxMethod().insert1({**vkey, "detection_method": 0})
    with pytest.raises(NotImplementedError, match="RTMDet"):
        pl.HandBbox().populate({**vkey, "detection_method": 0})
    bkey = {**vkey, "detection_method": 1}
    pl.HandBboxMethod().insert1(bkey)
    pl.HandBbox().populate(bkey)
    for mid, name in ((0, "RTMPoseHand5"), (1, "RTMPoseCOCO"), (2, "freihand")):
        with pytest.raises(NotImplementedError, match=name):
            hand_estimation.mmpose_HPE(bkey, name)
        pl.HandPoseEstimationMethod().insert1({**bkey, "estimation_method": mid})
        with pytest.raises(Exception, match="Method not implemented"):
            pl.HandPoseEstimation().populate({**bkey, "estimation_method": mid})
    assert len(pl.HandPoseEstimation()) == 0
    # without the Halpe track the box stage says so, as the reference does
    djshim.reset()
    pl.Video().insert1({**vkey, "video": "unused.ppvid", "start_time": datetime.datetime(2024, 5, 1)})
    pl.HandBboxMethod().insert1(bkey)
    with pytest.raises(Exception, match="does not have the required keypoints"):
        pl.HandBbox().populate(bkey)


def test_hand_settings_and_checkpoint_paths(monkeypatch, tmp_path):
    from posepipeline_amd import weights
    from posepipeline_amd.wrappers import hand_estimation as he
    d, u = he.topdown_settings("HRNet_dark"), he.topdown_settings("HRNet_udp")
    for s in (d, u):
        assert s["num_joints"] == 21 and np.array_equal(s["flip_perm"], np.arange(21)) and s["blur_kernel"] == 11
        assert s["chan_map"] == (2, 1, 0)          # one BGR -> RGB swap
    assert (d["post"], d["shift_heatmap"]) == ("unbiased", True) and (u["post"], u["shift_heatmap"]) == ("udp", False)
    assert np.array_equal(he.boxes_to_tlwh([[10.0, 20.0, 110.0, 70.0]]), [[10.0, 20.0, 100.0, 50.0]])
    assert os.path.basename(he._METHODS["HRNet_dark"][1]) == "hrnetv2_w18_rhd2d_256x256_dark-4df3a347_20210330.pth"
    assert os.path.basename(he._METHODS["HRNet_udp"][1]) == "hrnetv2_w18_onehand10k_256x256_udp-0d1b515d_20210330.pth"
    # a missing checkpoint raises with the expected path (nothing is ever fetched)
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    monkeypatch.delenv("POSEPIPE_SYNTHETIC_WEIGHTS", raising=False)
    spec = hrnetv2.hrnetv2_w18_256x256()
    with pytest.raises(FileNotFoundError) as e:
        weights.get_state_dict(he._METHODS["HRNet_dark"][1], hrnetv2.hrnetv2_param_shapes(spec), seed=1)
    assert os.path.join(str(tmp_path), "mmpose/checkpoints/hrnetv2_w18_rhd2d_256x256_dark-4df3a347_20210330.pth") in str(e.value)


# ---- 3. the float32 bilinear restatement vs torch in float64 ------------------------------------------------------------------
@pytest.mark.parametrize("u", [1, 2, 3])
@pytest.mark.parametrize("hw", [(3, 5), (1, 7), (6, 1)])
def test_bilinear_restatement_vs_torch_float64(u, hw):
    """value = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11) with exact (dyadic) weights: a tap's
    contribution w_ij * a_ij passes through at most FOUR float32 roundings (its product, the inner sum, the product with
    the row weight, the outer sum), each of relative size <= eps = 2^-24.  So
        |float32 value - exact value| <= ((1 + eps)^4 - 1) * sum_ij w_ij |a_ij|,
    i.e. 4 eps (two ulp) of the value itself where the four taps have one sign.  The float64 evaluation of torch is exact to
    2^-53 of the same sum, which the factor 4.001 absorbs."""
    h, w = hw
    rng = np.random.default_rng(10 * u + h)
    x = (rng.standard_normal((2, h, w, 4)) * rng.choice([1e-3, 1.0, 1e3], (2, 1, 1, 4))).astype(np.float32)
    got = hand_ref.bilinear_up(x, u)
    assert got.dtype == np.float32 and got.shape == (2, h << u, w << u, 4)
    t = torch.from_numpy(np.transpose(x, (0, 3, 1, 2)).astype(np.float64))
    ref = F.interpolate(t, scale_factor=2 ** u, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    mag = F.interpolate(t.abs(), scale_factor=2 ** u, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= 4.001 * 2.0 ** -24 * mag).all(), (err / mag).max() / 2.0 ** -24
    assert err.max() > 0 or u == 0                  # (the comparison is not vacuous: float32 did round somewhere)
    # the output-size form gives the same map
    ref2 = F.interpolate(t, size=(h << u, w << u), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(ref, ref2)


def test_bilinear_add_order_and_identity():
    rng = np.random.default_rng(3)
    r = rng.standard_normal((1, 8, 8, 4)).astype(np.float32)
    a, b = rng.standard_normal((1, 4, 4, 4)).astype(np.float32), rng.standard_normal((1, 2, 2, 4)).astype(np.float32)
    want = np.maximum((r + hand_ref.bilinear_up(a, 1)) + hand_ref.bilinear_up(b, 2), 0)
    assert np.array_equal(hand_ref.bilinear_add([(a, 1), (b, 2)], res1=r, relu_last=True), want)
    assert np.array_equal(hand_ref.bilinear_up(r, 0), r)          # a resize to the same size is the identity


# ---- 4. / 5. parameter inventory and program ------------------------------------------------------------------------------
def test_hrnetv2_param_shapes():
    spec = hrnetv2.hrnetv2_w18_256x256()
    sh = hrnetv2.hrnetv2_param_shapes(spec)
    assert spec.channels == (18, 36, 72, 144) and spec.concat_channels == 270
    H = "keypoint_head.final_layer."
    assert sh[H + "0.weight"] == (270, 270, 1, 1) and sh[H + "0.bias"] == (270,)
    assert all(sh[H + "1." + s] == (270,) for s in ("weight", "bias", "running_mean", "running_var"))
    assert sh[H + "3.weight"] == (21, 270, 1, 1) and sh[H + "3.bias"] == (21,)
    assert "keypoint_head.final_layer.weight" not in sh
    # multiscale_output: every module -- the last one too -- has a fuse layer for every (i, j), i != j
    for stage, (n_mod, n_br) in zip((2, 3, 4), spec.stages):
        for m in range(n_mod):
            for i in range(n_br):
                for j in range(n_br):
                    pre = f"backbone.stage{stage}.{m}.fuse_layers.{i}.{j}."
                    keys = [k for k in sh if k.startswith(pre)]
                    assert bool(keys) == (i != j), pre
                    if j > i:
                        assert sh[pre + "0.weight"] == (spec.channels[i], spec.channels[j], 1, 1)
                    elif j < i:
                        assert sh[f"{pre}{i - j - 1}.0.weight"] == (spec.channels[i], spec.channels[j], 3, 3)
    # the pose HRNet of the same widths has only fuse output 0 in its last module
    pose = hrnet.hrnet_param_shapes(hrnet.HRNetSpec(18, 21, 256, 256))
    assert not any(k.startswith("backbone.stage4.2.fuse_layers.1.") for k in pose)
    assert set(pose) - set(sh) == {"keypoint_head.final_layer.weight", "keypoint_head.final_layer.bias"}


@pytest.fixture(scope="module")
def v2_program():
    spec = hrnetv2.hrnetv2_w18_256x256()
    sd = synth.synth_state_dict(hrnetv2.hrnetv2_param_shapes(spec), seed=2)
    return spec, sd, hrnetv2.build_hrnetv2_program(spec, sd)


def test_hrnetv2_program(v2_program):
    spec, sd, prog = v2_program
    assert prog.bufs[prog.named["input"]] == (256, 256, 4) and prog.bufs[prog.named["output"]] == (64, 64, 21)
    last = prog.ops[-1]
    assert last.type == L.PP_OP_CONV and last.out == prog.named["output"] and last.out_nchw == 1 and (last.cin, last.cout) == (272, 21)
    bil = [op for op in prog.ops if op.type == L.PP_OP_BILINEAR_ADD]
    # from the stage table: one pass per fuse output that has a coarser branch (n_br - 1 per module), three resizes for the head
    want = sum(n_mod * (n_br - 1) for n_mod, n_br in ((1, 2), (4, 3), (3, 4))) + 3
    assert want == 21 == hrnetv2.bilinear_op_count(spec) == len(bil)
    assert not any(op.type == L.PP_OP_UPSAMPLE_ADD for op in prog.ops)
    # the concatenation: one 64x64x272 buffer, written in four channel slices (20 + 36 + 72 + 144), read by the head
    cat = [op for op in bil if prog.bufs[op.out][2] != op.cout]
    assert len({op.out for op in cat}) == 1 and prog.bufs[cat[0].out] == (64, 64, 272)
    assert sorted((op.out_c_off, op.cout) for op in cat) == [(0, 20), (20, 36), (56, 72), (128, 144)]
    assert sorted(op.up_log2 for op in cat[1:]) == [1, 2, 3] and all(op.in2 < 0 and op.res1 < 0 for op in cat[1:])
    head0 = prog.ops[-2]
    assert head0.type == L.PP_OP_CONV and head0.in_ == cat[0].out and (head0.cin, head0.cout, head0.relu) == (272, 272, L.PP_RELU_LAST)
    assert ctypes_sizeof_op() == 120
    with pytest.raises(KeyError):
        hrnetv2.build_hrnetv2_program(spec, {k: v for k, v in sd.items() if k != "keypoint_head.final_layer.0.bias"})
    bad = dict(sd)
    bad["keypoint_head.final_layer.3.weight"] = np.zeros((21, 18, 1, 1), np.float32)
    with pytest.raises(ValueError):
        hrnetv2.build_hrnetv2_program(spec, bad)


def ctypes_sizeof_op():
    import ctypes
    return ctypes.sizeof(L.pp_op)


# ---- 6. the CPU restatement vs an independently assembled torch float64 model ----------------------------------------------
class TorchHRNetV2:
    """mmpose 0.x HRNet (multiscale_output, bilinear fuse upsampling) + resize_concat head written against torch ops only,
    in float64, BatchNorm unfolded."""

    def __init__(self, sd, width):
        self.sd = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in sd.items()}
        self.ch = [width * 2 ** i for i in range(4)]

    def bn(self, y, bn):
        sd = self.sd
        return F.batch_norm(y, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.1, 1e-5)

    def cb(self, x, conv, bn, stride=1, pad=1):
        return self.bn(F.conv2d(x, self.sd[conv + ".weight"], None, stride, pad), bn)

    def forward(self, x):
        B = "backbone."
        x = F.relu(self.cb(x, B + "conv1", B + "bn1", 2))
        x = F.relu(self.cb(x, B + "conv2", B + "bn2", 2))
        for i in range(4):
            p = f"{B}layer1.{i}."
            idn = self.cb(x, p + "downsample.0", p + "downsample.1", 1, 0) if i == 0 else x
            y = F.relu(self.cb(x, p + "conv1", p + "bn1", 1, 0))
            y = F.relu(self.cb(y, p + "conv2", p + "bn2", 1, 1))
            x = F.relu(self.cb(y, p + "conv3", p + "bn3", 1, 0) + idn)
        ys, pre = [x], [256]
        for si, (n_mod, n_br) in enumerate(((1, 2), (4, 3), (3, 4))):
            cur = self.ch[:n_br]
            t = f"{B}transition{si + 1}."
            xs = []
            for i in range(n_br):
                if i < len(pre):
                    xs.append(F.relu(self.cb(ys[i], f"{t}{i}.0", f"{t}{i}.1")) if pre[i] != cur[i] else ys[i])
                else:
                    y = ys[-1]
                    for j in range(i + 1 - len(pre)):
                        y = F.relu(self.cb(y, f"{t}{i}.{j}.0", f"{t}{i}.{j}.1", 2))
                    xs.append(y)
            for m in range(n_mod):
                mp = f"{B}stage{si + 2}.{m}."
                for b in range(n_br):
                    for k in range(4):
                        p = f"{mp}branches.{b}.{k}."
                        y = F.relu(self.cb(xs[b], p + "conv1", p + "bn1"))
                        xs[b] = F.relu(self.cb(y, p + "conv2", p + "bn2") + xs[b])
                outs = []
                for i in range(n_br):
                    y = 0
                    for j in range(n_br):
                        f = f"{mp}fuse_layers.{i}.{j}."
                        if i == j:
                            y = y + xs[j]
                        elif j > i:
                            y = y + F.interpolate(self.cb(xs[j], f + "0", f + "1", 1, 0), scale_factor=2 ** (j - i), mode="bilinear",
                                                  align_corners=False)
                        else:
                            z = xs[j]
                            for k in range(i - j):
                                z = self.cb(z, f"{f}{k}.0", f"{f}{k}.1", 2)
                                if k != i - j - 1:
                                    z = F.relu(z)
                            y = y + z
                    outs.append(F.relu(y))
                xs = outs
            ys, pre = xs, cur
        size = ys[0].shape[2:]
        cat = torch.cat([F.interpolate(y, size=size, mode="bilinear", align_corners=False) for y in ys], dim=1)
        H = "keypoint_head.final_layer."
        y = F.relu(self.bn(F.conv2d(cat, self.sd[H + "0.weight"], self.sd[H + "0.bias"]), H + "1"))
        return F.conv2d(y, self.sd[H + "3.weight"], self.sd[H + "3.bias"])


def test_hrnetv2_ref_vs_torch_float64():
    """tests/test_oracle_nets.py holds the float32 oracle of the pose HRNet to 2e-4 of the output range against a float32 torch
    model (two float32 evaluations in different orders).  Against a float64 model only ONE float32 evaluation's rounding is in
    the gap, of a network of the same depth, so the same bar holds with room."""
    spec = hrnetv2.HRNetV2Spec(18, 21, 64, 96)
    sd = synth.synth_state_dict(hrnetv2.hrnetv2_param_shapes(spec), seed=4)
    x = np.random.default_rng(1).standard_normal((2, 3, 64, 96)).astype(np.float32)
    with torch.no_grad():
        ref = TorchHRNetV2(sd, 18).forward(torch.from_numpy(x).double()).numpy()
    got = hand_ref.HRNetV2Ref(sd, 18).forward(x)
    assert got.shape == ref.shape == (2, 21, 16, 24) and got.dtype == np.float32
    scale = np.abs(ref).max()
    assert scale > 1e-3
    assert np.abs(got - ref).max() <= 2e-4 * scale, np.abs(got - ref).max() / scale


# ---- 7. the pose HRNet programs did not change ------------------------------------------------------------------------------
def program_digest(prog):
    h = hashlib.sha256()
    for op in prog.ops:
        h.update(bytes(op))
    h.update(np.asarray(prog.bufs, np.int32).tobytes())
    h.update(np.asarray(prog.buf_pad or [0] * len(prog.bufs), np.int32).tobytes())
    h.update(np.ascontiguousarray(prog.blob, np.float32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("spec,digest", [
    (hrnet.HRNetSpec(32, 17, 256, 192), "a02a7890b8a5a28491c8585d4310a079a4b54859ef88db1afb04269ea6150865"),
    (hrnet.HRNetSpec(48, 136, 384, 288), "2d072533c56fb6d37d208d6af8ce6f705ea4d0bc7a7ef115019b97ad8f2d5277"),
])
def test_pose_hrnet_programs_unchanged(spec, digest, monkeypatch):
    """sha256 over every pp_op record, the buffer table and the weight blob of the program built from seeded parameters,
    recorded on the commit before models/hrnet.py gained its HRNetv2 hooks: the defaults reproduce it byte for byte."""
    monkeypatch.delenv("POSEPIPE_CONV_HALO", raising=False)
    assert hrnet.FUSE_MODE == "onepass"
    sd = synth.synth_state_dict(hrnet.hrnet_param_shapes(spec), seed=7)
    assert program_digest(hrnet.build_hrnet_program(spec, sd)) == digest
