"""FairMOT stage on the CPU: table row, tracker against the loop-by-loop reference, assignment against enumeration, geometry,
transform_preds, parameter inventory, the program's buffers and the float64 network reference's internal consistency.
(The kernels are held to tests/fairmot_ref.py by tests/test_gpu_fairmot.py.)"""
import datetime
import sys
import types

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.models import dla
from posepipeline_amd.tracking import JDETracker, lapjv_assign
from tests import fairmot_ref as R


# ---- table row and import ---------------------------------------------------------------------------------------------------------
def test_tracking_row_2_populates_through_the_wrapper(monkeypatch, tmp_path):
    """fails on the parent commit: row 2 raised Exception("Unsupported tracking method")"""
    from posepipeline_amd import djshim, pipeline as pl, video
    import posepipeline_amd.wrappers as W
    djshim.reset()
    try:
        assert (pl.TrackingBboxMethodLookup & {"tracking_method": 2}).fetch1("tracking_method_name") == "FairMOT"
        path = str(tmp_path / "v.ppvid")
        video.write_ppvid(path, np.zeros((5, 48, 64, 3), np.uint8), 30.0)
        vkey = {"video_project": "p", "filename": "f"}
        pl.Video().insert1({**vkey, "video": path, "start_time": datetime.datetime(2024, 5, 1)})
        calls = []

        def fake(file_path):
            calls.append(file_path)
            box = lambda i: {"track_id": i, "tlbr": np.array([1.0, 2, 11, 22]), "tlhw": np.array([1.0, 2, 10, 20]), "confidence": 0.9}
            return [[box(1)], [box(1), box(2)], [], [box(4)], [box(1)]]
        fake_mod = types.ModuleType("posepipeline_amd.wrappers.fairmot")
        fake_mod.fairmot_bounding_boxes = fake
        monkeypatch.setitem(sys.modules, "posepipeline_amd.wrappers.fairmot", fake_mod)
        monkeypatch.setattr(W, "fairmot", fake_mod, raising=False)
        tkey = {**vkey, "tracking_method": 2}
        pl.TrackingBboxMethod().insert1(tkey)
        pl.TrackingBbox().populate()
        assert calls == [path]
        assert (pl.TrackingBbox & tkey).fetch1("num_tracks") == 3
        assert len((pl.TrackingBbox & tkey).fetch1("tracks")) == 5
    finally:
        djshim.reset()


def test_reference_module_path_imports():
    from pose_pipeline.wrappers.fairmot import fairmot_bounding_boxes
    from posepipeline_amd.wrappers import fairmot as w
    assert fairmot_bounding_boxes is w.fairmot_bounding_boxes
    for word in ("1920 x 1080", "608 x 1088", "min_box_area", "BaseTrack._count", "K = 500", "conf_thres = 0.2", "track_buffer = 30"):
        assert word in w.__doc__, word


# ---- tracker ----------------------------------------------------------------------------------------------------------------------
def _unit(k, d=8, mix=None):
    v = np.zeros(d)
    v[k] = 1.0
    if mix is not None:
        v[mix] = 0.05
    return v


def _scenario(n_frames):
    """frame -> (dets [n][5], feats [n][8]).  A: present except frame 5 (where a far look-alike E appears: gated), re-activated by
    appearance in frame 6.  B: frames 1-3, away 4-6, back in 7 (re-activated).  C: new in frame 2 (unconfirmed), confirmed in 3, matched
    by IoU alone in 4 (its embedding changes).  D: frame 2 only (dropped).  F: frame 5, on top of lost B with another embedding
    (duplicate of a longer-lived lost track).  G: frames 1-2, then never again (expires)."""
    frames = []
    for f in range(1, n_frames + 1):
        d, e = [], []

        def add(x, y, w, h, s, feat):
            d.append([x, y, x + w, y + h, s])
            e.append(feat)
        if f != 5:
            add(100 + 2 * f, 100 + f, 60, 160, 0.9, _unit(0, mix=3))
        else:
            add(900, 500, 60, 160, 0.8, _unit(0, mix=4))                     # E: A's look-alike, far away
        if f <= 3 or f >= 7:
            add(400 + f, 120, 50, 150, 0.85, _unit(1))
        if f >= 2:
            add(650 - f, 300 + f, 70, 170, 0.7, _unit(2) if f != 4 else _unit(5))
        if f == 2:
            add(1200, 200, 40, 100, 0.5, _unit(6))                           # D
        if f == 5:
            add(403, 120, 50, 150, 0.6, _unit(7))                            # F: where lost B waits
        if f <= 2:
            add(1500, 700, 80, 200, 0.75, _unit(4))                          # G
        frames.append((np.array(d, np.float64).reshape(-1, 5), np.array(e, np.float64).reshape(len(d), 8)))
    return frames


@pytest.mark.parametrize("fps", [30, 15])
def test_tracker_scenario_against_the_loop_by_loop_reference(fps):
    """ids and scores are equal; boxes agree to 1e-9 relative: the product runs the C++ Kalman filter (pp_kalman_*), the reference
    a numpy one, both float64, so the last bits of a Cholesky solve may differ"""
    trk, ref = JDETracker(frame_rate=fps), R.JDETrackerRef(frame_rate=fps)
    assert trk.max_time_lost == ref.max_time_lost == fps
    for f, (dets, feats) in enumerate(_scenario(40), 1):
        got, want = trk.step(dets, feats), ref.step(dets, feats)
        assert [g[0] for g in got] == [w[0] for w in want], f
        assert [g[2] for g in got] == [w[2] for w in want], f
        for g, w in zip(got, want):
            np.testing.assert_allclose(g[1], w[1], rtol=1e-9, atol=1e-9)
        if f == 1:
            assert sorted(g[0] for g in got) == [1, 2, 3]                  # frame-1 activation, ids from 1
    kinds = {e[0] for e in ref.events}
    assert {"activate", "update", "re_activate", "lost", "confirmed", "dropped", "gated", "iou", "duplicate", "expired"} <= kinds, kinds
    ev = ref.events
    a_id = 1
    assert ("gated", 5, a_id, 0) in ev and ("lost", 5, a_id) in ev and ("re_activate", 6, a_id) in ev       # A never takes its far look-alike
    assert ("re_activate", 7, 2) in ev                                                                      # B, by appearance
    c_id = next(e[2] for e in ev if e[0] == "activate" and e[1] == 2)
    assert ("confirmed", 3, c_id) in ev and ("iou", 4, c_id) in ev
    assert any(e[0] == "dropped" and e[1] == 3 for e in ev)                                                # D
    assert any(e[0] == "duplicate" and e[1] == 5 and e[3] == 2 for e in ev)                                # F over lost B
    # G (id 3) was last matched in frame 2: it expires in the first frame with frame - 2 > max_time_lost
    assert [e for e in ev if e[0] == "expired" and e[2] == 3][0][1] == 2 + fps + 1


def test_a_second_tracker_starts_ids_at_one_again():
    dets, feats = _scenario(1)[0]
    assert sorted(t[0] for t in JDETracker().step(dets, feats)) == sorted(t[0] for t in JDETracker().step(dets, feats)) == [1, 2, 3]


def test_extended_matrix_assignment_against_enumeration():
    rng = np.random.default_rng(5)
    n_inf = 0
    for trial in range(200):
        n, m = rng.integers(1, 6, 2)
        cost = rng.uniform(0, 1, (n, m))
        if trial % 2:
            cost[rng.uniform(size=(n, m)) < 0.3] = np.inf
        n_inf += int(np.isinf(cost).sum())
        thresh = float(rng.choice([0.4, 0.5, 0.7]))
        matches, ur, uc = lapjv_assign(cost, thresh)
        want, best = R.assign_brute_force(cost, thresh)
        assert set(matches) == want, (cost, thresh, matches, want)
        assert all(cost[i, j] <= thresh for i, j in matches)
        assert sorted(ur + [i for i, _ in matches]) == list(range(n)) and sorted(uc + [j for _, j in matches]) == list(range(m))
    assert n_inf > 100
    assert lapjv_assign(np.zeros((0, 3)), 0.4) == ([], [], [0, 1, 2]) and lapjv_assign(np.zeros((2, 0)), 0.4) == ([], [0, 1], [])


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def test_letterbox_geometry_both_orientations():
    from posepipeline_amd import ops
    g = R.letterbox_geometry(1080, 1920)
    assert (g["hp"], g["wp"], g["nw"], g["nh"], g["left"], g["right"], g["top"], g["bottom"]) == (608, 1088, 1081, 608, 3, 4, 0, 0)
    p = R.letterbox_geometry(1920, 1080)
    assert (p["hp"], p["wp"], p["nw"], p["nh"], p["left"], p["right"], p["top"], p["bottom"]) == (1088, 608, 608, 342, 0, 0, 373, 373)
    for hw in ((1080, 1920), (48, 64), (90, 50), (1920, 1080), (300, 300)):
        r = R.letterbox_geometry(*hw)
        assert ops.fairmot_input_size(*hw) == (r["hp"], r["wp"], r["nh"], r["nw"], r["top"], r["left"]), hw


def test_transform_preds_against_the_explicit_inverse_map():
    """CenterNet builds the matrix from float32 triangles: the scale s (1932.6 landscape, 1920 portrait) and s / 2 are rounded to
    float32, so against the float64 map the factor is off by at most 2^-23 relative and a mapped coordinate by at most
    2^-23 * s = 2.3e-4 px; stored as float32 a coordinate below 2048 adds half an ulp, 2^-14 = 6.1e-5 px"""
    from posepipeline_amd.wrappers import fairmot as w
    rng = np.random.default_rng(1)
    for hp, wp in ((608, 1088), (1088, 608)):
        s = max(wp / hp * 1080, 1920)
        tol = s * 2.0 ** -23
        m, m64 = w.transform_matrix(hp, wp), R.transform_matrix_f64(hp, wp)
        np.testing.assert_allclose(m[:, :2], m64[:, :2], rtol=0, atol=m64[0, 0] * 2.0 ** -23)
        np.testing.assert_allclose(m[:, 2], m64[:, 2], rtol=0, atol=tol)
        pts = rng.uniform(0, [wp // 4, hp // 4], (50, 2)).astype(np.float32)
        want = np.concatenate([pts.astype(np.float64), np.ones((50, 1))], 1) @ m64.T
        np.testing.assert_allclose(w.transform_preds(pts, m), want, rtol=0, atol=tol)
        dets = np.concatenate([pts, pts + 3, rng.uniform(0, 1, (50, 1)).astype(np.float32)], 1).astype(np.float32)
        got = w.post_process(dets, hp, wp)
        ref, keep = R.post_process(dets, hp, wp)
        assert got.shape == dets.shape and keep.sum() == len(ref)
        np.testing.assert_allclose(got[keep][:, :4], ref[:, :4], rtol=0, atol=tol + 2.0 ** -13)
        assert np.array_equal(got[:, 4], dets[:, 4])
    # landscape: the heat-map centre is the frame centre and a cell is s / 272 pixels
    m = w.transform_matrix(608, 1088)
    s = 1088 / 608 * 1080
    np.testing.assert_allclose(w.transform_preds(np.array([[136.0, 76.0], [137.0, 76.0]], np.float32), m),
                               [[960.0, 540.0], [960.0 + s / 272, 540.0]], atol=s * 2.0 ** -23)


# ---- parameters -------------------------------------------------------------------------------------------------------------------
def _independent_count():
    bn = lambda c: 4 * c
    block = lambda ci, co: co * ci * 9 + bn(co) + co * co * 9 + bn(co)

    def tree1(ci, co, extra):
        return (co * ci + bn(co) if ci != co else 0) + block(ci, co) + block(co, co) + co * (2 * co + extra) + bn(co)
    deform = lambda ci, co: bn(co) + co * ci * 9 + co + 27 * ci * 9 + 27
    step = lambda ci, o, f: deform(ci, o) + deform(o, o) + o * 4 * f * f
    n = 16 * 3 * 49 + bn(16) + 16 * 16 * 9 + bn(16) + 32 * 16 * 9 + bn(32)
    n += tree1(32, 64, 0)
    n += tree1(64, 128, 0) + tree1(128, 128, 64 + 128)
    n += tree1(128, 256, 0) + tree1(256, 256, 128 + 256)
    n += tree1(256, 512, 256)
    n += step(512, 256, 2) + 2 * step(256, 128, 2) + 3 * step(128, 64, 2)          # dla_up: ida_0, ida_1, ida_2
    n += step(128, 64, 2) + step(256, 64, 4)                                       # ida_up
    n += sum(256 * 64 * 9 + 256 + c * 256 + c for c in (1, 4, 128, 2))
    return n


def test_parameter_inventory_and_checkpoint_checks():
    shapes = dla.dla34_param_shapes()
    assert dla.dla34_param_count() == _independent_count() == sum(int(np.prod(s)) for s in shapes.values())
    assert shapes["dla_up.ida_0.proj_1.conv.conv_offset_mask.weight"] == (27, 512, 3, 3)
    assert shapes["ida_up.up_2.weight"] == (64, 1, 8, 8) and shapes["base.level3.tree2.root.conv.weight"] == (128, 448, 1, 1)
    assert sum(k.endswith("conv_offset_mask.weight") for k in shapes) == 16
    sd = {k: np.zeros(s, np.float32) for k, s in shapes.items()}
    ok = dla.check_state_dict({"module." + k: v for k, v in sd.items()})            # a DataParallel checkpoint
    assert set(ok) == set(shapes)
    ok = dla.check_state_dict({**sd, "base.fc.weight": np.zeros((1000, 512, 1, 1), np.float32)})      # extra keys are ignored
    assert set(ok) == set(shapes)
    bad = dict(sd)
    del bad["hm.2.bias"]
    with pytest.raises(KeyError, match="hm.2.bias"):
        dla.check_state_dict(bad)
    bad = dict(sd)
    bad["id.2.weight"] = np.zeros((64, 256, 1, 1), np.float32)
    with pytest.raises(ValueError, match="id.2.weight"):
        dla.check_state_dict(bad)


def test_synthetic_weights_need_the_switch(monkeypatch, tmp_path):
    monkeypatch.setenv("PIPELINE_3RDPARTY", str(tmp_path))
    monkeypatch.delenv("POSEPIPE_SYNTHETIC_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError):
        dla.get_state_dict()
    monkeypatch.setenv("POSEPIPE_SYNTHETIC_WEIGHTS", "1")
    sd = dla.get_state_dict()
    assert set(sd) == set(dla.dla34_param_shapes()) and float(sd["hm.2.bias"][0]) < -1.0


# ---- program ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    return dla.synth_dla34_state_dict(dla.dla34_param_shapes(), 11)


@pytest.mark.parametrize("hp,wp", [(608, 1088), (1088, 608)])
def test_program_builds_with_the_right_buffers(seeded, hp, wp):
    prog = dla.build_dla34_program(seeded, hp, wp)
    out_dims = {name: prog.bufs[op.out] for name, op in zip(prog.op_names, prog.ops)}
    want = {"base.base_layer.0": (1, 16), "base.level0.0": (1, 16), "base.level1.0": (2, 32), "base.level2.root.conv": (4, 64),
            "base.level3.tree2.root.conv": (8, 128), "base.level4.tree2.root.conv": (16, 256), "base.level5.root.conv": (32, 512),
            "dla_up.ida_0.node_1.conv": (16, 256), "dla_up.ida_1.node_2.conv": (8, 128), "dla_up.ida_2.node_3.conv": (4, 64),
            "ida_up.node_1.conv": (4, 64), "ida_up.node_2.conv": (4, 64), "ida_up.up_2": (4, 64), "dla_up.ida_0.up_1": (16, 256)}
    for name, (s, c) in want.items():
        assert out_dims[name] == (hp // s, wp // s, c), (name, out_dims[name])
    for head, c in dla.HEADS:
        assert prog.bufs[prog.named[head]] == (hp // 4, wp // 4, c)
    assert prog.bufs[prog.named["input"]] == (hp, wp, 4)
    types_ = [op.type for op in prog.ops]
    assert types_.count(L.PP_OP_DCN3X3) == 16 and types_.count(L.PP_OP_DWDECONV) == 8
    for op in prog.ops:
        if op.type == L.PP_OP_DCN3X3:
            assert prog.bufs[op.in2][2] == 27 and prog.bufs[op.in2][:2] == prog.bufs[op.in_][:2] == prog.bufs[op.out][:2]
        if op.type == L.PP_OP_DWDECONV:
            assert op.res1 >= 0 and prog.bufs[op.res1] == prog.bufs[op.out]
    # the Root of level3.tree2 reads one 448-channel buffer: x2 | x1 | bottom | tree1's output
    root = prog.ops[prog.op_names.index("base.level3.tree2.root.conv")]
    assert prog.bufs[root.in_] == (hp // 8, wp // 8, 448)
    assert 0.2e9 < dla.activation_bytes_per_frame(prog) < 0.5e9


# ---- float64 network reference: internal consistency ------------------------------------------------------------------------------
def test_reference_dcn_with_zero_offsets_is_a_convolution():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((7, 9, 8))
    w = rng.standard_normal((5, 8, 3, 3))
    b = rng.standard_normal(5)
    om = np.zeros((7, 9, 27))
    om[..., 18:] = np.inf
    np.testing.assert_allclose(R.dcn3x3(x, om, w, b), R.conv2d(x, w, b, 1, 1), rtol=0, atol=1e-12)
    # integer offsets move the taps: every tap one pixel to the right = the convolution of the image shifted left (but for
    # output column 0, whose left tap now reads column 0 where the shifted image has its zero padding)
    om[..., 1:18:2] = 1.0
    xs = np.zeros_like(x)
    xs[:, :-1] = x[:, 1:]
    np.testing.assert_allclose(R.dcn3x3(x, om, w, b)[:, 1:], R.conv2d(xs, w, b, 1, 1)[:, 1:], rtol=0, atol=1e-12)
    # logits of -inf switch every tap off
    om[..., 18:] = -np.inf
    np.testing.assert_allclose(R.dcn3x3(x, om, w, b), np.broadcast_to(b, (7, 9, 5)), rtol=0, atol=0)


@pytest.mark.parametrize("s", [2, 4, 8])
def test_reference_dwdeconv_with_bilinear_weights_is_bilinear_upsampling(s):
    rng = np.random.default_rng(3)
    h, w, c = 5, 6, 3
    x = rng.standard_normal((h, w, c))
    k, f = 2 * s, s
    cc = (2 * f - 1 - f % 2) / (2.0 * f)
    w1 = 1 - np.abs(np.arange(k) / f - cc)                                   # upstream fill_up_weights
    wt = np.broadcast_to(np.outer(w1, w1), (c, 1, k, k))
    y = R.dwdeconv(x, wt, s)
    assert y.shape == (h * s, w * s, c)
    oy, ox = np.mgrid[s:(h - 1) * s, s:(w - 1) * s]                         # interior
    sy, sx = (oy + 0.5) / s - 0.5, (ox + 0.5) / s - 0.5
    y0, x0 = np.floor(sy).astype(int), np.floor(sx).astype(int)
    ly, lx = (sy - y0)[..., None], (sx - x0)[..., None]
    want = (1 - ly) * ((1 - lx) * x[y0, x0] + lx * x[y0, x0 + 1]) + ly * ((1 - lx) * x[y0 + 1, x0] + lx * x[y0 + 1, x0 + 1])
    np.testing.assert_allclose(y[oy, ox], want, rtol=0, atol=1e-12)


def test_reference_network_shapes_and_float32_deviation(seeded):
    x = np.zeros((32, 64, 4), np.float32)
    x[..., :3] = np.random.default_rng(4).uniform(0, 1, (32, 64, 3))
    h64 = R.Dla34Ref(seeded, np.float64).forward(x)
    h32 = R.Dla34Ref(seeded, np.float32).forward(x)
    for head, c in dla.HEADS:
        assert h64[head].shape == (8, 16, c) and h64[head].dtype == np.float64 and h32[head].dtype == np.float32
        dev = np.abs(h32[head] - h64[head]).max() / np.abs(h64[head]).max()
        assert 0 < dev < 1e-4, (head, dev)


def test_reference_preprocess_and_decode_basics():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    out = R.preprocess(img)
    assert out.shape == (608, 1088, 4) and out.dtype == np.float32 and not out[..., 3].any()
    assert (out[:, :3, :3] == np.float32(128) / np.float32(255)).all() and (out[:, -4:, :3] == np.float32(128) / np.float32(255)).all()
    flat = np.full((90, 50, 3), 77, np.uint8)                                # a constant image stays constant through both resizes
    p = R.preprocess(flat)
    assert p.shape == (1088, 608, 4) and (p[373:373 + 342, :, :3] == np.float32(77) / np.float32(255)).all()
    assert (p[:373, :, :3] == np.float32(128) / np.float32(255)).all()
    big = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    assert np.array_equal(R.resize_linear_u8(big, 1920, 1080), big)           # the identity first step
    # decode: two equal peaks rank by index, a plateau keeps its members, the rest are -1
    hm = np.full((6, 7, 1), -5.0, np.float32)
    hm[1, 1] = hm[4, 5] = 2.0
    hm[3, 2] = hm[3, 3] = 1.0
    wh, reg, idm = np.ones((6, 7, 4), np.float32), np.zeros((6, 7, 2), np.float32), rng.standard_normal((6, 7, 8)).astype(np.float32)
    dets, feats, inds = R.decode(hm, wh, reg, idm, 8)
    assert inds[:4].tolist() == [8, 33, 23, 24] and dets[0, :4].tolist() == [0.0, 0.0, 2.0, 2.0]
    assert len(set(inds[4:].tolist()) - {-1}) == 4 or (inds[4:] >= 0).all()    # the flat -5 background is one big plateau
    np.testing.assert_allclose(np.linalg.norm(feats[:4], axis=1), 1.0, atol=1e-12)
