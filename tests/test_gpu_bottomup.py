"""The bottom-up stage on the GPU: the three post-processing kernels alone on maps the test builds, the HigherHRNet program
against the oracle's HRNet + a torch float64 head, and `mmpose_bottom_up` through the tables against the reference chain
(tests/bottomup_ref.py) fed the GPU's own four maps.

Bounds: the project's convention, FACTOR x the deviation of the SAME reference run in float32 from its float64 run.  What must be
exact (candidate indices, comparison bits, refine positions, the grouping) is made robust by construction: the seeds below were
chosen on the CPU, from the float64 reference alone, so that every decision the chain takes has a margin of more than
10 x that float32 deviation (`assert_gaps`, asserted in the test)."""
import datetime

import numpy as np
import pytest

from tests import bottomup_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 4
K = 17


# ---- synthetic low-resolution maps ---------------------------------------------------------------------------------------------
def synth_maps(seed, f, h0, w0, n_person=3):
    """s0 [2f][34][h0][w0], s1 [2f][17][2 h0][2 w0] as the network would give them for f frames and their mirror images: Gaussian
    peaks for n_person persons (some joints weak -- below the detection threshold, for the refine step -- some absent), per-person
    tag planes 3 apart, noise on everything.  The heat-map noise sits below zero, so that the positive local maxima are the peaks
    (a noise floor around zero has hundreds of maxima per plane, and some pair of them is always closer than any margin); the
    last joint of every frame carries 40 extra sub-threshold spikes of distinct heights, which puts the rank-30 cut to work."""
    rng = np.random.default_rng(seed)
    fi = np.asarray(ref.FLIP_INDEX)
    h1, w1 = 2 * h0, 2 * w0
    s0 = np.zeros((2 * f, 2 * K, h0, w0))
    s1 = np.zeros((2 * f, K, h1, w1))
    for fr in range(f):
        pos = rng.uniform(0.12, 0.88, (n_person, K, 2))                      # (y, x) in units of the map
        amp = rng.uniform(0.6, 0.95, (n_person, K))
        kind = rng.uniform(0, 1, (n_person, K))
        amp = np.where(kind < 0.15, 0.07, np.where(kind < 0.25, 0.0, amp))   # weak / absent joints
        amp[:, 0] = np.maximum(amp[:, 0], 0.6)                               # every person has a nose: three groups open at once
        amp[:, K - 1] = 0.0                                                  # the last joint belongs to the spikes below
        tagval = 3.0 * np.arange(n_person)

        def heat(h, w, sigma):
            yy, xx = np.mgrid[0:h, 0:w]
            m = np.zeros((K, h, w))
            for p in range(n_person):
                for j in range(K):
                    cy, cx = pos[p, j, 0] * (h - 1), pos[p, j, 1] * (w - 1)
                    m[j] += amp[p, j] * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma ** 2))
            return m
        yy, xx = np.mgrid[0:h0, 0:w0]
        tag = np.zeros((K, h0, w0))
        for j in range(K):
            d = np.stack([(yy - pos[p, j, 0] * (h0 - 1)) ** 2 + (xx - pos[p, j, 1] * (w0 - 1)) ** 2 for p in range(n_person)])
            tag[j] = tagval[np.argmin(d, axis=0)]
        c0, c1 = heat(h0, w0, 0.8), heat(h1, w1, 1.6)
        mirror = lambda m: m[fi][..., ::-1]          # noqa: E731  what the network gives for the mirrored frame
        s0[fr, :K] = c0 + rng.normal(-0.02, 0.01, c0.shape)
        s0[fr, K:] = tag + rng.normal(0, 0.02, tag.shape)
        s1[fr] = c1 + rng.normal(-0.02, 0.01, c1.shape)
        s0[f + fr, :K] = mirror(c0) + rng.normal(-0.02, 0.01, c0.shape)
        s0[f + fr, K:] = mirror(tag) + rng.normal(0, 0.02, tag.shape)
        s1[f + fr] = mirror(c1) + rng.normal(-0.02, 0.01, c1.shape)
        sy, sx = np.meshgrid(np.arange(1, h1, 3), np.arange(1, w1, 3), indexing="ij")
        spikes = np.stack([sy.ravel(), sx.ravel()], 1)[:40]
        height = 0.15 + 0.002 * rng.permutation(len(spikes))
        for dy, dx, g in ((0, 0, 1.0), (0, 1, 0.5), (0, -1, 0.5), (1, 0, 0.5), (-1, 0, 0.5)):      # small tents: they survive any resize
            s1[fr, K - 1, spikes[:, 0] + dy, spikes[:, 1] + dx] += g * height
            s1[f + fr, fi[K - 1], spikes[:, 0] + dy, w1 - 1 - (spikes[:, 1] + dx)] += g * height
    return s0.astype(np.float32), s1.astype(np.float32)


def neighbour_max(v):
    """max over the 5x5 neighbourhood WITHOUT the centre, clipped to the map; v [..][H][W]"""
    h, w = v.shape[-2:]
    pad = np.full(v.shape[:-2] + (h + 4, w + 4), -np.inf)
    pad[..., 2:-2, 2:-2] = v
    out = np.full(v.shape, -np.inf)
    for dy in range(5):
        for dx in range(5):
            if (dy, dx) != (2, 2):
                out = np.maximum(out, pad[..., dy:dy + h, dx:dx + w])
    return out


def assert_gaps(trace, margin_h, margin_t):
    """every decision of the float64 chain has a margin: margin_h on heat-map values, margin_t on tag distances.  Returns the
    largest number of positive survivors in one plane."""
    hm = trace["hm"]
    f, k, h, w = hm.shape
    most = 0
    for fr in range(f):
        rec = trace["frames"][fr]
        top = rec["top"]
        for c in range(k):
            v = hm[fr, c]
            nm = neighbour_max(v)
            surv = np.sort(v[(v >= nm) & (v > 0)])[::-1]
            lead = surv[:ref.MAX_PEOPLE + 1]
            most = max(most, len(surv))
            assert (np.abs(np.diff(lead)) > margin_h).all(), "ranked candidates (the 30th / 31st cut included) too close"
            assert (np.abs(lead - ref.DET_THR) > margin_h).all() and (lead > margin_h).all(), "a candidate at a threshold"
            cut = lead[ref.MAX_PEOPLE] if len(lead) > ref.MAX_PEOPLE else 0.0
            near = v > cut - margin_h
            assert (np.abs(v - nm)[near] > margin_h).all(), "a pixel that is a local maximum by less than the margin"
            for m in range(ref.MAX_PEOPLE):
                if top["val"][c, m] > 0:
                    y, x = top["y"][c, m], top["x"][c, m]
                    assert abs(v[min(h - 1, y + 1), x] - v[max(0, y - 1), x]) > margin_h
                    assert abs(v[y, min(w - 1, x + 1)] - v[y, max(0, x - 1)]) > margin_h
        for d in rec["dists"]:
            assert (np.abs(d - np.floor(d) - 0.5) > margin_t).all() and (np.abs(d - ref.TAG_THR) > margin_t).all(), "a tag distance at a rounding step"
        for s in rec["scans"]:
            y, x, d, m = s["y"], s["x"], s["d"], s["hm"]
            if m.max() < -margin_h:          # no positive pixel: whichever wins, its value is not > 0 and nothing is filled
                continue
            best_low = m[y, x] - margin_h - np.round(d[y, x] + margin_t)
            others = m + margin_h - np.round(d - margin_t)
            others[y, x] = -np.inf
            assert best_low > others.max(), "the refine arg-max is not robust"
            assert abs(m[y, x]) > margin_h
            assert abs(m[min(h - 1, y + 1), x] - m[max(0, y - 1), x]) > margin_h and abs(m[y, min(w - 1, x + 1)] - m[y, max(0, x - 1)]) > margin_h
        sc = np.sort(np.asarray(rec["scores"], np.float64))
        assert len(sc) < 2 or (np.diff(sc) > margin_h).all()
    return most


def reference_runs(s0, s1, hr, wr, center, scale, align):
    """the chain in float64 and in float32 -> (results64, trace64, float32 deviation of the heat-maps, of the tags)"""
    t64, t32 = {}, {}
    out64 = ref.chain(s0, s1, hr, wr, center, scale, align, np.float64, trace=t64)
    ref.chain(s0, s1, hr, wr, center, scale, align, np.float32, trace=t32)
    dev_h = float(np.abs(t32["hm"].astype(np.float64) - t64["hm"]).max())
    dev_t = float(np.abs(t32["tags"].astype(np.float64) - t64["tags"]).max())
    return out64, t64, dev_h, dev_t


# (frames, (h0, w0), (hr, wr), seed): 8x12 and 16x24 maps projected to 32x48 (x4 / x2), and to the odd 40x56 (x5 / x2.5 and
# x4.67 / x2.33: no output pixel but the corners falls on a source pixel with align_corners, none without)
KERNEL_CASES = [(2, (8, 12), (32, 48), 3), (1, (8, 12), (40, 56), 3)]


@pytest.mark.parametrize("align", [True, False], ids=["align_corners", "half_pixel"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "f%d_%dx%d_to_%dx%d" % (c[0], c[1][0], c[1][1], c[2][0], c[2][1]))
def test_kernels_alone(ctx, case, align):
    from posepipeline_amd import bottomup as bu
    f, (h0, w0), (hr, wr), seed = case
    s0, s1 = synth_maps(seed, f, h0, w0)
    center, scale = np.array([wr * 0.8, hr * 0.9]), np.array([wr * 1.5 / 200.0, hr * 1.5 / 200.0])
    want, t64, dev_h, dev_t = reference_runs(s0, s1, hr, wr, center, scale, align)
    assert 0 < dev_h < 1e-5 and 0 < dev_t < 1e-4
    most = assert_gaps(t64, 10 * dev_h, 10 * 4 * dev_t)     # a distance moves by < 4 x what its tags move by (two points, two dims)
    assert most > ref.MAX_PEOPLE                            # the rank-30 cut drops something
    n_filled = sum(fr["filled"] for fr in t64["frames"])
    assert all(len(fr["persons"]) >= 3 for fr in t64["frames"]) and n_filled >= 1
    maps = bu.MapSet(ctx, s0, s1, f, K, (h0, w0), (2 * h0, 2 * w0), hr, wr, np.asarray(ref.FLIP_INDEX), align)
    try:
        maps.aggregate()
        hm = maps.heatmaps()
        err_h = float(np.abs(hm.astype(np.float64) - t64["hm"]).max())
        cand = maps.candidates(30)
        assert np.array_equal(cand, maps.candidates(30))                    # run-to-run
        err_t = err_v = 0.0
        for fr in range(f):
            top = t64["frames"][fr]["top"]
            on = top["val"] > 0
            assert on.any() and np.array_equal(cand[fr, :, :, 0] > 0, on)
            assert np.array_equal(cand[fr, :, :, 7][on], top["ind"][on]) and np.array_equal(cand[fr, :, :, 1][on], top["x"][on])
            assert np.array_equal(cand[fr, :, :, 2][on], top["y"][on])
            assert np.array_equal(cand[fr, :, :, 5][on] > 0, top["by"][on]) and np.array_equal(cand[fr, :, :, 6][on] > 0, top["bx"][on])
            assert np.array_equal(cand[fr][~on], np.broadcast_to(np.array([0, -1, -1, 0, 0, 0, 0, -1], np.float32), cand[fr][~on].shape))
            err_v = max(err_v, float(np.abs(cand[fr, :, :, 0][on] - top["val"][on]).max()))
            err_t = max(err_t, float(np.abs(cand[fr, :, :, 3:5][on] - top["tag"][on]).max()))
        trace = {}
        got = bu.parse_chunk(maps, center, scale, trace=trace)
    finally:
        maps.close()
    print(f"[{hr}x{wr} align={align}] float32 reference vs float64: heat-maps {dev_h:.3e}, tags {dev_t:.3e}; GPU vs float64: heat-maps "
          f"{err_h:.3e}, candidate values {err_v:.3e}, candidate tags {err_t:.3e}; refined joints {n_filled}")
    assert err_h <= FACTOR * dev_h and err_v <= FACTOR * dev_h and err_t <= FACTOR * dev_t
    assert trace["refined"] == n_filled
    for fr in range(f):
        r64 = t64["frames"][fr]
        assert np.array_equal(trace["persons"][fr][:, :, [1, 2]], r64["persons"][:, :, :2])          # the groups, in order
        assert np.array_equal(trace["kpts"][fr][:, :, :2], r64["refined"][:, :, :2])                 # adjusted + refined positions
        assert got[fr].shape == want[fr].shape and got[fr].dtype == np.float32
        assert np.array_equal(got[fr][:, :, :2], want[fr][:, :, :2])                                # exact positions map to equal pixels
        assert np.abs(got[fr][:, :, 2] - want[fr][:, :, 2]).max() <= FACTOR * dev_h


def test_plateau_ties_go_to_the_lower_index(ctx):
    """Equal maxima: two in one 5x5 window (both survive: neither is larger) and a run of equal peaks across the rank-30 cut.  The
    heat-maps are written directly, so the values are exactly equal; ties rank by the lower flat index, every run the same."""
    from posepipeline_amd import bottomup as bu
    hr, wr, h0, w0 = 40, 56, 8, 12
    rng = np.random.default_rng(4)
    s0, s1 = synth_maps(3, 1, h0, w0)
    hm = (rng.uniform(-0.2, -0.1, (1, K, hr, wr))).astype(np.float32)
    # joint 0: 40 isolated peaks, 35 of them with the SAME value 0.5 (ranks 3 .. 37: the cut at 30 falls inside the run), a pair of
    # equal maxima 0.75 two pixels apart, and 3 distinct larger ones
    ys, xs = np.meshgrid(np.arange(2, hr, 6), np.arange(2, wr, 6), indexing="ij")
    pts = np.stack([ys.ravel(), xs.ravel()], 1)
    rng.shuffle(pts)
    for i, (y, x) in enumerate(pts[:40]):
        hm[0, 0, y, x] = [0.9, 0.8, 0.7][i] if i < 3 else (0.5 if i < 38 else 0.3)
    py, px = pts[40]
    hm[0, 0, py, px] = hm[0, 0, py, px + 2] = 0.75
    # joint 1: a flat positive map: every pixel is a survivor, the first 30 indices win
    hm[0, 1] = 0.25
    maps = bu.MapSet(ctx, s0, s1, 1, K, (h0, w0), (2 * h0, 2 * w0), hr, wr, np.asarray(ref.FLIP_INDEX), True)
    try:
        maps.ctx.h2d(maps.hm, hm)
        cand = maps.candidates(30)
        again = maps.candidates(30)
    finally:
        maps.close()
    assert np.array_equal(cand, again)
    _, tags = ref.aggregate(s0, s1, hr, wr, True, np.float64)
    top = ref.top_k(hm[0].astype(np.float64), tags[0])
    for c in (0, 1):
        assert np.array_equal(cand[0, c, :, 7], top["ind"][c]) and np.array_equal(cand[0, c, :, 0], top["val"][c].astype(np.float32))
        assert np.array_equal(cand[0, c, :, 5] > 0, top["by"][c]) and np.array_equal(cand[0, c, :, 6] > 0, top["bx"][c])
    assert np.array_equal(cand[0, 1, :, 7], np.arange(30))
    v0, i0 = cand[0, 0, :, 0], cand[0, 0, :, 7]
    assert list(v0[:5]) == [np.float32(0.9), np.float32(0.8), np.float32(0.75), np.float32(0.75), np.float32(0.7)]
    assert i0[3] == i0[2] + 2 and (v0[5:] == 0.5).all()                  # the pair, lower index first; then 25 of the 35 equal peaks
    want = np.sort([y * wr + x for y, x in pts[3:38]])[:25]
    assert np.array_equal(i0[5:], want)
    assert (cand[0, 2:, :, 0] == 0).all() and (cand[0, 2:, :, 7] == -1).all()      # negative maps: no candidate


# ---- 2. the network ------------------------------------------------------------------------------------------------------------
SMALL = dict(image_size=128, width=48)        # the W48 widths at a quarter of the size


def backbone_features(sd, x_nchw, width=48):
    """branch 0 of the oracle's HRNet (oracle/nets.py, bit-equal to the float32-MFMA kernels): its head is a 1x1 convolution, an
    identity matrix there hands the features out unchanged (1 * x + 0 * ... is exact)"""
    from oracle import nets as onets
    sd2 = dict(sd)
    sd2["keypoint_head.final_layer.weight"] = np.eye(width, dtype=np.float32).reshape(width, width, 1, 1)
    sd2["keypoint_head.final_layer.bias"] = np.zeros(width, np.float32)
    return onets.HRNetRef(sd2, width, width).forward(x_nchw)


def torch_head(sd, feats, dtype):
    """BottomUpHigherResolutionHead on the backbone features with torch ops only, BatchNorm unfolded: (y0, y1) as numpy"""
    import torch
    import torch.nn.functional as F
    p = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd.items() if k.startswith("keypoint_head.")}
    H = "keypoint_head."

    def bn(y, n):
        return F.batch_norm(y, p[n + ".running_mean"], p[n + ".running_var"], p[n + ".weight"], p[n + ".bias"], False, 0.1, 1e-5)
    with torch.no_grad():
        x = torch.from_numpy(feats).to(dtype)
        y0 = F.conv2d(x, p[H + "final_layers.0.weight"], p[H + "final_layers.0.bias"])
        x = torch.cat([x, y0], 1)
        x = F.relu(bn(F.conv_transpose2d(x, p[H + "deconv_layers.0.0.0.weight"], None, 2, 1), H + "deconv_layers.0.0.1"))
        for i in range(4):
            b = f"{H}deconv_layers.0.1.{i}."
            y = F.relu(bn(F.conv2d(x, p[b + "conv1.weight"], None, 1, 1), b + "bn1"))
            x = F.relu(bn(F.conv2d(y, p[b + "conv2.weight"], None, 1, 1), b + "bn2") + x)
        y1 = F.conv2d(x, p[H + "final_layers.1.weight"], p[H + "final_layers.1.bias"])
    return y0.numpy(), y1.numpy()


def test_network_vs_oracle_backbone_and_torch_float64_head(ctx):
    import torch
    from posepipeline_amd.models import higherhrnet as hh
    from posepipeline_amd.models import synth
    from posepipeline_amd.program import Net
    spec = hh.HigherHRNetSpec(**SMALL)
    sd = synth.synth_state_dict(hh.higherhrnet_param_shapes(spec), seed=3)
    hp, wp = 64, 128
    prog = hh.build_higherhrnet_program(spec, sd, hp, wp)
    x = np.random.default_rng(0).standard_normal((2, 3, hp, wp)).astype(np.float32)
    xin = np.zeros((2, hp, wp, 4), np.float32)
    xin[..., :3] = np.transpose(x, (0, 2, 3, 1))
    feats = backbone_features(sd, x)
    r64 = torch_head(sd, feats, torch.float64)
    r32 = torch_head(sd, feats, torch.float32)
    dev = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32, r64)]
    got = {}
    for numerics in ("exact", "split"):
        net = Net(ctx, prog, max_batch=2, numerics=numerics)
        assert net.numerics == numerics
        ctx.h2d(net.buffer("input")[0], xin)
        net.run(2)
        ctx.synchronize()
        got[numerics] = (net.read("output0", 2).reshape(2, 34, hp // 4, wp // 4), net.read("output1", 2).reshape(2, 17, hp // 2, wp // 2))
        net.close()
    err = {m: [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got[m], r64)] for m in got}
    rng_ = [float(np.abs(b).max()) for b in r64]
    print(f"HigherHRNet-W48 {hp}x{wp}, output range {rng_[0]:.3e} / {rng_[1]:.3e}: torch float32 head vs float64 {dev[0]:.3e} / {dev[1]:.3e}; "
          f"GPU exact vs float64 {err['exact'][0]:.3e} / {err['exact'][1]:.3e}; GPU default numerics {err['split'][0]:.3e} / {err['split'][1]:.3e}")
    assert all(d > 0 for d in dev) and all(np.isfinite(a).all() for a in got["exact"])
    assert err["exact"][0] <= FACTOR * dev[0] and err["exact"][1] <= FACTOR * dev[1]


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------
def clip_frames():
    """3 frames of 60 x 100 (-> a 128 x 256 input): blocks of colour + noise"""
    rng = np.random.default_rng(21)
    coarse = rng.integers(0, 256, (3, 6, 10, 3)).astype(np.float64)
    frames = np.repeat(np.repeat(coarse, 10, axis=1), 10, axis=2) + rng.normal(0, 12, (3, 60, 100, 3))
    return np.clip(frames, 0, 255).astype(np.uint8)


# Seeded heads give maps of no use to the parser (values in the hundreds, everywhere).  The final 1x1 layers are scaled and biased,
# per channel, so that the AVERAGED heat-maps have a standard deviation near 1 around -2.8: a handful of peaks per frame are
# positive, most of those above detection_threshold, and the tags spread by about 0.3, so that candidates group into a few
# persons whose missing joints the refine step can fill.  The figures were measured once on the CPU (oracle backbone + torch head)
# on the clip below; what they are meant to achieve is asserted from the reference's trace.
HEAD_GAIN = (0.0658, 0.00953, 0.0524)            # final_layers.0 heat-map rows, final_layers.0 tag rows, final_layers.1
HEAD_BIAS0 = [-6.943, -1.685, 1.973, -4.061, 0.223, -8.142, 7.811, 8.482, -3.826, 11.726, -4.409, -2.82, -4.396, 3.637, -1.432, 11.114,
              -17.969, 0.181, -1.371, 0.153, -0.801, -1.159, -0.329, -0.503, 0.396, 1.594, -1.013, 0.753, -1.445, 0.472, -0.927, 1.854,
              -0.624, -0.077]
HEAD_BIAS1 = [-4.054, -7.973, 0.679, -2.42, -5.418, -0.126, -3.308, -7.481, -2.801, -5.245, -0.618, -2.756, -1.173, 2.335, 0.059, -6.219,
              1.856]


def tame_heads(sd):
    H = "keypoint_head."
    sd = dict(sd)
    w = sd[H + "final_layers.0.weight"].copy()
    w[:K] *= np.float32(HEAD_GAIN[0])
    w[K:] *= np.float32(HEAD_GAIN[1])
    sd[H + "final_layers.0.weight"] = w
    sd[H + "final_layers.0.bias"] = np.asarray(HEAD_BIAS0, np.float32)
    sd[H + "final_layers.1.weight"] = sd[H + "final_layers.1.weight"] * np.float32(HEAD_GAIN[2])
    sd[H + "final_layers.1.bias"] = np.asarray(HEAD_BIAS1, np.float32)
    return sd


def matched_person(box, persons, iou_thr=0.25, vis_thr=0.1, min_joints=5):
    """The reference's rule for a track's (x, y, w, h) box (utils/keypoint_matching.py): each person's box spans its joints
    with score > 0.1, and is empty when fewer than 5 are; the first person of largest IoU is taken if that IoU exceeds
    0.25.  Returns its index or None; float64"""
    best, best_iou = None, 0.0
    bx0, by0, bx1, by1 = box[0], box[1], box[0] + box[2], box[1] + box[3]
    for j, p in enumerate(np.asarray(persons, np.float64)):
        vis = p[p[:, 2] > vis_thr, :2]
        if len(vis) < min_joints:
            continue
        x0, y0, x1, y1 = vis[:, 0].min(), vis[:, 1].min(), vis[:, 0].max(), vis[:, 1].max()
        iw, ih = min(bx1, x1) - max(bx0, x0), min(by1, y1) - max(by0, y0)
        if iw <= 0 or ih <= 0:
            continue
        iou = iw * ih / ((bx1 - bx0) * (by1 - by0) + (x1 - x0) * (y1 - y0) - iw * ih + 1e-8)
        if iou > best_iou:
            best, best_iou = j, iou
    return best if best_iou > iou_thr else None


def test_end_to_end_through_the_tables(ctx, monkeypatch, tmp_path):
    from posepipeline_amd import bottomup as bu
    from posepipeline_amd import djshim, video
    from posepipeline_amd import pipeline as pl
    from posepipeline_amd.models import higherhrnet as hh
    from posepipeline_amd.models import synth
    from posepipeline_amd.wrappers import mmpose as mp
    frames = clip_frames()
    path = str(tmp_path / "clip.ppvid")
    video.write_ppvid(path, frames, fps=30.0)
    spec = hh.HigherHRNetSpec(**SMALL)
    sd = tame_heads(synth.synth_state_dict(hh.higherhrnet_param_shapes(spec), seed=1))
    stage = bu.BottomUpStage(spec=spec, ctx=ctx, state_dict=sd)
    monkeypatch.setitem(mp._bottom_up_cache, 0, stage)
    djshim.reset()
    try:
        vkey = {"video_project": "test", "filename": "bottomup"}
        pl.Video().insert1({**vkey, "video": path, "start_time": datetime.datetime(2024, 1, 1)})
        mkey = {**vkey, "bottom_up_method_name": "MMPose"}
        pl.BottomUpMethod().insert1(mkey)
        pl.BottomUpPeople().populate(mkey)
        kps = (pl.BottomUpPeople & mkey).fetch1("keypoints")
        assert len(kps) == 3 and all(k.dtype == np.float32 and k.shape[1:] == (17, 3) for k in kps)
        for stage_name in ("preprocess", "network", "aggregate", "candidates", "group", "refine", "nms", "total"):
            assert mp.last_timing[stage_name] >= 0
        assert mp.last_timing["frames"] == 3
        again = mp.mmpose_bottom_up(mkey)
        assert all(np.array_equal(a, b) for a, b in zip(kps, again))
        # the reference chain on the GPU's own four maps (the clip is one chunk: the net still holds them)
        wr, hr, center, scale = ref.input_size(60, 100, 128)
        assert (wr, hr) == (256, 128) and list(stage.nets) == [(128, 256)]
        net = stage.nets[(128, 256)]
        s0 = net.read("output0", 6).reshape(6, 34, 32, 64)
        s1 = net.read("output1", 6).reshape(6, 17, 64, 128)
        want, t64, dev_h, dev_t = reference_runs(s0, s1, hr, wr, center, scale, True)
        assert_gaps(t64, 10 * dev_h, 10 * 4 * dev_t)
        n_cand = sum(int((fr["top"]["val"] > ref.DET_THR).sum()) for fr in t64["frames"])
        n_filled = sum(fr["filled"] for fr in t64["frames"])
        n_dropped = sum(len(fr["persons"]) - len(fr["keep"]) for fr in t64["frames"])
        print(f"end to end: {n_cand} candidates above the threshold, {[len(fr['persons']) for fr in t64['frames']]} persons, {n_filled} joints "
              f"refined, {n_dropped} persons dropped by oks_nms; float32 deviation {dev_h:.3e} (heat-maps) {dev_t:.3e} (tags)")
        assert 3 <= n_cand <= 60 and n_filled >= 1 and all(len(w) >= 1 for w in want)
        for got, exp in zip(kps, want):
            assert got.shape == exp.shape                                            # same persons ...
            assert np.abs(got[:, :, :2] - exp[:, :, :2]).max() <= FACTOR * dev_h      # ... in the same order, at the same place
            assert np.abs(got[:, :, 2] - exp[:, :, 2]).max() <= FACTOR * dev_h
        # BottomUpPerson: a track that follows the first person of each frame.  What the table must hold is what the reference's
        # matching rule (restated in matched_person) gives for these boxes; a person of the scaled seeded heads may have too few
        # visible joints to be matched at all, and then its frame is a (17, 3) row of zeros
        boxes = []
        for k in kps:
            p = k[0]
            boxes.append([p[:, 0].min(), p[:, 1].min(), p[:, 0].max() - p[:, 0].min(), p[:, 1].max() - p[:, 1].min()])
        boxes = np.array(boxes, np.float64)
        pkey = {**vkey, "tracking_method": 0, "video_subject_id": 0}
        pl.PersonBbox().insert1({**pkey, "bbox": boxes, "present": np.ones(3, bool)})
        pl.BottomUpPerson().populate(pkey)
        person = (pl.BottomUpPerson & {**pkey, **mkey}).fetch1("keypoints")
        picks = [matched_person(boxes[i], kps[i]) for i in range(3)]
        print(f"BottomUpPerson: the track's boxes match persons {picks} (None: no person with 5 visible joints and IoU > 0.25)")
        assert isinstance(person, np.ndarray) and person.dtype != object and person.shape == (3, 17, 3)
        for i, j in enumerate(picks):
            assert np.array_equal(person[i], np.zeros((17, 3)) if j is None else kps[i][j])
    finally:
        djshim.reset()
        stage.close()


# ---- 4. the resize-align warp ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(60, 100), (100, 60), (64, 64)])
def test_resize_align_warp_bit_exact(ctx, hw):
    """pp_warp_affine_normalize against the oracle's cv2.warpAffine on BottomUpResizeAlign's transform: the u8 warp, the normalised
    tensor and its mirrored copy, for a landscape, a portrait and a square frame"""
    from posepipeline_amd import bottomup as bu
    h, w = hw
    frames = np.random.default_rng(h).integers(0, 256, (2, h, w, 3)).astype(np.uint8)
    wr, hr, center, scale = bu.input_size(h, w, 128)
    out, u8 = bu.warp_affine_normalize(ctx, frames, center, scale, (wr, hr), want_u8=True)
    assert out.shape == (4, hr, wr, 4) and u8.shape == (2, hr, wr, 3)
    for i in range(2):
        x, ref_u8 = ref.network_input(frames[i], 128)
        assert ref_u8.shape == (hr, wr, 3) and np.array_equal(u8[i], ref_u8)
        assert np.array_equal(out[i, :, :, :3], np.transpose(x, (1, 2, 0))) and not out[i, :, :, 3].any()
        assert np.array_equal(out[2 + i], out[i][:, ::-1])
    assert len(np.unique(u8)) > 100
