"""Inputs and references for tests/test_gpu_roi_align.py: RoIAlign on CHOSEN RoIs (roi_align_kernel, the exact numerics, and
roi_align_sep_kernel, the default; csrc/det_post.hip).  TEST INFRASTRUCTURE ONLY: numpy and the oracle, no device code, so that
tests/test_roi_align_cases.py can check every property stated below on a machine without a GPU.

Geometry: source frames of 153 x 272 become 612 x 1088 inside 640 x 1088 (the benchmarked geometry) with scale factors of exactly
4.0, so every RoI corner below (input pixels = 4 x source pixels) is exact in the float32 product pp_detector_regress forms.  The FPN
maps are 160 x 272, 80 x 136, 40 x 68 and 20 x 34 at strides 4 / 8 / 16 / 32, 256 channels.

Every builder is cached and hands out read-only arrays: one input and one reference per process, shared by the tests."""
import functools

import numpy as np

from oracle import detector as odet

f32, f64 = np.float32, np.float64
SRC_H, SRC_W = 153, 272
INPUT_SIZE = (612, 1088, 640, 1088)          # detector_input_size(153, 272): resized h, w inside padded h, w
SF = 4.0
IMG_H, IMG_W = 640, 1088
STRIDES = (4, 8, 16, 32)
MAP_HW = ((160, 272), (80, 136), (40, 68), (20, 34))
C = 256
N_FRAMES = 2


def _ro(a):
    a.setflags(write=False)
    return a


# ---- feature maps -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def feature_maps(frame):
    """the four FPN maps [h][w][256] of one frame: seeded noise, every channel with its own scale (1 .. 7) and offset (0.01 c), so
    that a lane serving another lane's channels shows; frame 1 has another seed, so the frame offset inside pp_detector_regress shows"""
    rng = np.random.default_rng(1000 + 17 * frame)
    c = np.arange(C)
    scale, offset = (1 + c % 7).astype(f32), (0.01 * c).astype(f32)
    return tuple(_ro((rng.standard_normal((h, w, C), dtype=f32) * scale + offset).astype(f32)) for h, w in MAP_HW)


def ramp_coefficients():
    """a_c, b_c, d_c (float64, dyadic): ramp map of level l is a_c x + b_c y + d_c at pixel (y, x), exact in float32"""
    c = np.arange(C)
    return ((c % 5) - 2) / 8.0, ((c % 3) - 1) / 4.0, c / 16.0


@functools.lru_cache(maxsize=None)
def ramp_maps():
    a, b, d = ramp_coefficients()
    out = []
    for h, w in MAP_HW:
        y, x = np.mgrid[0:h, 0:w]
        m = a[None, None, :] * x[:, :, None] + b[None, None, :] * y[:, :, None] + d[None, None, :]
        assert np.array_equal(m.astype(f32).astype(f64), m)
        out.append(_ro(m.astype(f32)))
    return tuple(out)


# RoIs inside the map whose sample positions are exact in float32 (dyadic corners, bin sizes and sample steps), one per level and a
# non-square one: the average over a bin of a linear function is the function at the bin's centre
RAMP_ROIS = np.array([(100, 60, 184, 144),            # level 0: bins of 3 px, 3 x 3 samples
                      (64, 64, 176, 176),             # level 1: bins of 2 px, 2 x 2 samples
                      (160, 96, 384, 320),            # level 2
                      (320, 96, 768, 544),            # level 3
                      (50.5, 30.25, 85.5, 86.25)],    # level 0, 35 x 56: bins of 1.25 x 2 px, 2 x 2 samples
                     f32)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def _axis(v, n, dtype):
    """one coordinate of a sample on an axis of n pixels, mmcv's bilinear_interpolate: None outside [-1, n], else (low, high, weight
    of high, weight of low).  The position, the validity test and the clamping are float32 (the op's decisions); the weights dtype."""
    if v < -1.0 or v > n:
        return None
    v = f32(max(v, f32(0)))
    low = int(v)
    if low >= n - 1:
        high = low = n - 1
        v = f32(low)
    else:
        high = low + 1
    l_ = dtype(dtype(v) - dtype(low))
    return low, high, l_, dtype(dtype(1) - l_)


def roi_align_ref(feat, roi, spatial_scale, dtype, info=None):
    """oracle.detector.roi_align's sample loop (mmcv RoIAlign 7 x 7, aligned, adaptive sampling, avg) for one roi on an [H][W][C]
    map -> [7][7][C] of `dtype`.  Sample positions, the validity test, the clamping, gh / gw / count stay in the oracle's float32
    arithmetic; the bilinear weights, the products and the sums are taken in `dtype` (float32: the oracle's bits; float64: what the
    GPU is measured against).  info (a dict, optional) receives gh, gw, the numbers of samples and of valid samples and the range of
    map columns and rows the valid samples read."""
    out = 7
    h, w, _ = feat.shape
    ss = f32(spatial_scale)
    x1, y1 = f32(f32(roi[0] * ss) - f32(0.5)), f32(f32(roi[1] * ss) - f32(0.5))
    x2, y2 = f32(f32(roi[2] * ss) - f32(0.5)), f32(f32(roi[3] * ss) - f32(0.5))
    rw, rh = f32(x2 - x1), f32(y2 - y1)
    bw, bh = f32(rw / f32(out)), f32(rh / f32(out))
    gh = int(np.ceil(f32(rh / f32(out))))
    gw = int(np.ceil(f32(rw / f32(out))))
    count = dtype(f32(max(gh * gw, 1)))
    res = np.zeros((out, out, feat.shape[2]), dtype)
    cols, rows, n_valid = [w, -1], [h, -1], 0
    for ph in range(out):
        for pw in range(out):
            acc = np.zeros(feat.shape[2], dtype)
            for iy in range(gh):
                y = f32(f32(y1 + f32(f32(ph) * bh)) + f32(f32(f32(iy) + f32(0.5)) * bh) / f32(gh))
                ay = _axis(y, h, dtype)
                if ay is None:
                    continue
                yl, yh, ly, hy = ay
                for ix in range(gw):
                    x = f32(f32(x1 + f32(f32(pw) * bw)) + f32(f32(f32(ix) + f32(0.5)) * bw) / f32(gw))
                    ax = _axis(x, w, dtype)
                    if ax is None:
                        continue
                    xl, xh, lx, hx = ax
                    w1, w2, w3, w4 = dtype(hy * hx), dtype(hy * lx), dtype(ly * hx), dtype(ly * lx)
                    v = w1 * feat[yl, xl].astype(dtype)
                    v = v + w2 * feat[yl, xh].astype(dtype)
                    v = v + w3 * feat[yh, xl].astype(dtype)
                    v = v + w4 * feat[yh, xh].astype(dtype)
                    acc = acc + v
                    n_valid += 1
                    cols[0], cols[1] = min(cols[0], xl), max(cols[1], xh)
                    rows[0], rows[1] = min(rows[0], yl), max(rows[1], yh)
            res[ph, pw] = acc / count
    if info is not None:
        info.update(gh=gh, gw=gw, n_samples=49 * max(gh, 0) * max(gw, 0), n_valid=n_valid, cols=tuple(cols), rows=tuple(rows))
    return res


def level_without_epsilon(rois):
    """map_roi_levels without its 1e-6 term (what the term decides is the difference to odet.map_roi_levels)"""
    scale = np.sqrt(((rois[:, 2] - rois[:, 0]).astype(f32) * (rois[:, 3] - rois[:, 1]).astype(f32)).astype(f32)).astype(f32)
    return np.clip(np.floor(np.log2((scale / f32(56)).astype(f32))), 0, 3).astype(np.int64)


# ---- RoI families, input pixels (x1, y1, x2, y2); each is one pp_detector_regress call per frame ----------------------------------------
def _square(x, y, side):
    return (x, y, f32(x) + f32(side), f32(y) + f32(side))


# the largest side below 112 that both 200 + side and 100 + side can hold in float32: 312 is followed downwards by 312 - 2^-15
SIDE_BELOW_112 = f32(np.nextafter(f32(312), f32(0))) - f32(200)
LEVEL_SIDES = (111.5, SIDE_BELOW_112, 112, 223.5, 224, 447.5, 448)
LEVELS_CLEAN = {111.5: 0, 112: 1, 223.5: 1, 224: 2, 447.5: 2, 448: 3}
WINDOW_K = (1, 2, 3, 5, 8, 13, 21, 34, 55, 67, 89, 130, 200, 258)
# edges: (roi, number of the 49 bins that are not zero)
EDGES_STATED = [((-4, 100, 24, 128), 49),           # first x sample at exactly -1.0: valid, reads column 0
                ((-4.5, 100, 23.5, 128), 42),       # first column of bins samples nothing
                ((1088, 100, 1116, 128), 7),        # x sample at exactly W: valid
                ((1088.5, 100, 1116.5, 128), 0),
                ((100, -4, 128, 24), 49),           # the same in y
                ((100, -4.5, 128, 23.5), 42),
                ((100, 640, 128, 668), 7),
                ((100, 640.5, 128, 668.5), 0)]
# one straddler per side (left, right, top, bottom) on each of levels 1 - 3
EDGES_STRADDLE = [(-60.25, 200, 99.75, 360), (1000.5, 200.5, 1160.5, 360.5), (400, -70.75, 560, 89.25), (400.25, 560, 560.25, 720),
                  (-120.5, 150, 179.5, 450), (950, 150.25, 1250, 450.25), (400, -130.5, 700, 169.5), (400.75, 500, 700.75, 800),
                  (-200, 60.5, 300, 560.5), (800.25, 60, 1300.25, 560), (300, -250.25, 800, 249.75), (300.5, 400.5, 800.5, 900.5)]
EDGES_STRADDLE_LEVELS = [1] * 4 + [2] * 4 + [3] * 4
DEGENERATE = [(300, 200, 300, 260),       # zero width
              (300, 200, 360, 200),       # zero height
              (300, 200, 300, 200),       # both
              (360, 260, 300, 200),       # inverted in both axes: the area is positive, the level defined
              (360, 200, 300, 260),       # inverted in x only: the level is the square root of a negative number
              (300, 260, 360, 200)]       # inverted in y only: likewise
DEGENERATE_NO_LEVEL = (4, 5)


def _generic():
    """24 seeded RoIs with fractional corners: six per level (sqrt(area) = 56 * 2^level * [1.1, 1.8], aspect 0.4 .. 2.5), of which the
    first leaves the image on the left or right and the second at the top or bottom"""
    rng = np.random.default_rng(24)
    out = []
    for level in range(4):
        for i in range(6):
            s = 56.0 * 2 ** level * rng.uniform(1.1, 1.8) if level else rng.uniform(20.0, 100.0)
            a = rng.uniform(0.4, 2.5)
            w, h = s * np.sqrt(a), s / np.sqrt(a)
            cx, cy = rng.uniform(0.5 * w, max(IMG_W - 0.5 * w, 0.5 * w + 1)), rng.uniform(0.5 * h, max(IMG_H - 0.5 * h, 0.5 * h + 1))
            if i == 0:
                cx = rng.uniform(-0.3, 0.3) * w + (IMG_W if level % 2 else 0)
            if i == 1:
                cy = rng.uniform(-0.3, 0.3) * h + (0 if level % 2 else IMG_H)
            out.append((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h))
    return out


@functools.lru_cache(maxsize=None)
def families():
    """name -> [n][4] float32.  `levels` has 9 RoIs (1 mod 4: the last workgroup of the separable kernel serves one RoI); `pair` is the
    first two RoIs of `generic` on their own, so that a workgroup has two idle waves"""
    fam = {
        "levels": [_square(200, 100, s) for s in LEVEL_SIDES] + [(544 - 1500, 320 - 1500, 544 + 1500, 320 + 1500), (300, 200, 300.5, 200.5)],
        "window": [(40, 300, 40 + 4 * k, 308) for k in WINDOW_K] + [(0, 200, 1088, 208), (500, 0, 508, 640)],
        "edges": [r for r, _ in EDGES_STATED] + EDGES_STRADDLE,
        "outside": [(-300, 100, -100, 200), (1200, 100, 1400, 200), (100, -200, 128, -100), (100, 700, 128, 800), (-300, -300, -100, -100)],
        "huge": [(-1500, -900, 2600, 1500), (-4000, -100, 5000, 700)],
        "degenerate": DEGENERATE,
        "generic": _generic(),
    }
    fam = {k: _ro(np.array(v, f32)) for k, v in fam.items()}
    fam["pair"] = _ro(fam["generic"][:2].copy())
    assert len(fam["levels"]) % 4 == 1
    return fam


FAMILY_NAMES = ("levels", "window", "edges", "outside", "huge", "degenerate", "generic", "pair")
ZERO_FAMILIES = ("outside", "degenerate")       # every row is exact zeros


def source_boxes(rois):
    """what pp_detector_regress is given: source pixels, rois / 4 (exact), which it multiplies by the scale factors (4.0, exact)"""
    b = (rois / f32(SF)).astype(f32)
    assert np.array_equal(b * f32(SF), rois)
    return b


def defined(name):
    """indices of the family's RoIs whose level is defined (all but the two half-inverted ones)"""
    n = len(families()[name])
    return [i for i in range(n) if not (name == "degenerate" and i in DEGENERATE_NO_LEVEL)]


@functools.lru_cache(maxsize=None)
def reference(frame, name):
    """dict(levels [n] (-1: not defined), ref32 [n][7][7][C] = odet.roi_align (the bits roi_align_kernel must give), ref64 = roi_align_ref
    in float64, info = per RoI what roi_align_ref reports).  RoIs without a defined level are not computed: their rows are zeros on any
    level, because gw < 1 or gh < 1."""
    rois = families()[name]
    maps = feature_maps(frame)
    n = len(rois)
    ok = defined(name)
    levels = np.full(n, -1, np.int64)
    levels[ok] = odet.map_roi_levels(rois[ok])
    ref32, ref64, infos = np.zeros((n, 7, 7, C), f32), np.zeros((n, 7, 7, C), f64), [None] * n
    for i in ok:
        lv = int(levels[i])
        ref32[i] = odet.roi_align(maps[lv], rois[i], 1.0 / STRIDES[lv])
        infos[i] = {}
        ref64[i] = roi_align_ref(maps[lv], rois[i], 1.0 / STRIDES[lv], f64, infos[i])
    return dict(levels=_ro(levels), ref32=_ro(ref32), ref64=_ro(ref64), info=infos)
