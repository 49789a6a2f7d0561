"""Inputs for tests/test_gpu_selection_wide.py: maps at which the two-level selections (per-workgroup partial results, then a
merge or rank pass) take more than one workgroup.  TEST INFRASTRUCTURE ONLY: numpy and the references (tests/bottomup_ref.py,
tests/fairmot_ref.py, tests/trades_ref.py), no device code, so that tests/test_selection_cases.py can check every property below
on a machine without a GPU.  Each `check_*` asserts, from the reference alone, that an input is what its builder says; the GPU tests
call the same functions before they compare.

The kernels' constants are not exported; the shapes here follow them and must follow them again if they change:
    BU_TILE 4096        pixels per workgroup of pp_bottomup_candidates (csrc/bottomup.hip)
    REFINE_SPAN 8192    pp_bottomup_refine splits a plane into clamp(npix / 8192, 1, 64) spans of ceil(npix / n_split) pixels
    RANK_CHUNK 256      keys per LDS chunk of fm_rank_of and per workgroup of the rank kernels (csrc/fairmot.hip)

Every builder is cached and hands out read-only arrays: one input and one reference per process, shared by the tests."""
import functools

import numpy as np

from tests import bottomup_ref as ref
from tests import fairmot_ref as FR
from tests import trades_ref as TR

f32 = np.float32
BU_TILE, REFINE_SPAN, REFINE_MAX_SPLIT, RANK_CHUNK = 4096, 8192, 64, 256
K = 17
NONE_ROW = np.array([0, -1, -1, 0, 0, 0, 0, -1], f32)      # a candidate slot with nothing in it


def n_tiles(npix):
    return -(-npix // BU_TILE)


def n_split(npix):
    return max(1, min(REFINE_MAX_SPLIT, npix // REFINE_SPAN))


def span_len(npix):
    return -(-npix // n_split(npix))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _sources(rng, f, h0, w0):
    """s0 [2f][2K][h0][w0], s1 [2f][K][2 h0][2 w0]: seeded noise (the tests below write the heat-maps directly; the tag planes of s0
    are what the candidate records and the refine scan interpolate)"""
    return rng.standard_normal((2 * f, 2 * K, h0, w0)).astype(f32), rng.standard_normal((2 * f, K, 2 * h0, 2 * w0)).astype(f32)


# ---- A. pp_bottomup_candidates: 96 x 100 = 9600 pixels = three tiles, the last of 1408 pixels ----------------------------------------
CAND = dict(f=2, h0=8, w0=12, hr=96, wr=100)
CAND_MAX_PEOPLE = (1, 30, 64)
# plane 5 of frame 0: (y, x, value).  4096 = (40, 96) and 8192 = (81, 92): both tile boundaries fall mid-row
PAIRS = [(40, 95, 0.6), (40, 97, 0.8),        # either side of 4096, unequal: the larger (in tile 1) suppresses the one in tile 0
         (81, 91, 0.7), (81, 93, 0.7),        # either side of 8192, equal: both survive, the lower index first
         (39, 50, 0.9), (41, 50, 0.5),        # 2 rows apart across the row that holds 4096, unequal: the one in tile 0 wins
         (80, 30, 0.65), (82, 30, 0.65)]      # 2 rows apart across the row that holds 8192, equal: both survive
PAIRS_WANT = [39 * 100 + 50, 40 * 100 + 97, 81 * 100 + 91, 81 * 100 + 93, 80 * 100 + 30, 82 * 100 + 30]


@functools.lru_cache(maxsize=None)
def candidates_case():
    """dict(s0, s1, hm [2][17][96][100] float32, tags64 / tags32 [2][17][96][100][2], dev_t): background in (-0.2, -0.1), isolated
    peaks on a lattice of pitch 5 (no peak inside another's 5x5 window); frame 1 = the planes of frame 0 in reverse order"""
    f, h0, w0, hr, wr = (CAND[k] for k in ("f", "h0", "w0", "hr", "wr"))
    rng = np.random.default_rng(20)
    s0, s1 = _sources(rng, f, h0, w0)
    hm0 = rng.uniform(-0.2, -0.1, (K, hr, wr)).astype(f32)
    ys, xs = np.meshgrid(np.arange(2, hr, 5), np.arange(2, wr, 5), indexing="ij")
    lattice = (ys * wr + xs).ravel()
    by_tile = [lattice[lattice // BU_TILE == t] for t in range(3)]

    def pick(counts):
        return [rng.permutation(by_tile[t])[:n] for t, n in enumerate(counts)]

    def put(c, idx, val):
        hm0[c].reshape(-1)[np.asarray(idx)] = np.asarray(val, f32)
    # plane 0: 35 distinct peaks per tile, the heights dealt at random over the three tiles
    put(0, np.concatenate(pick((35, 35, 35))), 0.15 + 0.005 * rng.permutation(105))
    # plane 1: the 32 largest in the ragged last tile, 32 smaller ones in each of the others
    lo0, lo1, hi = pick((32, 32, 32))
    put(1, hi, 0.6 + 0.01 * rng.permutation(32))
    put(1, np.concatenate([lo0, lo1]), 0.1 + 0.004 * rng.permutation(64))
    # plane 2: 5 distinct peaks above a run of 40 equal ones over all three tiles (ranks 5 .. 44: the cut at 30 falls inside)
    p0, p1, p2 = pick((16, 14, 15))
    put(2, np.concatenate([p0[:2], p1[:1], p2[:2]]), [0.9, 0.8, 0.85, 0.7, 0.75])
    put(2, np.concatenate([p0[2:], p1[1:], p2[2:]]), 0.5)
    # plane 3: flat and positive: every pixel survives, every tile offers its first max_people pixels
    hm0[3] = 0.25
    # plane 4: seven survivors, all in tile 1
    put(4, pick((0, 7, 0))[1], 0.3 + 0.05 * rng.permutation(7))
    # plane 5: pairs across the tile boundaries
    for y, x, v in PAIRS:
        hm0[5, y, x] = v
    hm = np.stack([hm0, hm0[::-1]])
    _, tags64 = ref.aggregate(s0, s1, hr, wr, True, np.float64)
    _, tags32 = ref.aggregate(s0, s1, hr, wr, True, f32)
    dev_t = float(np.abs(tags32.astype(np.float64) - tags64).max())
    return _freeze(dict(s0=s0, s1=s1, hm=np.ascontiguousarray(hm), tags64=tags64, tags32=tags32, dev_t=dev_t, **CAND))


@functools.lru_cache(maxsize=None)
def candidates_expected(max_people):
    """ref.top_k of both frames in float64"""
    case = candidates_case()
    return [ref.top_k(case["hm"][fr].astype(np.float64), case["tags64"][fr], max_people) for fr in range(case["f"])]


def _survivors(plane):
    """(flat indices, values) of the positive 5x5 maxima of one float64 plane, by descending value then ascending index"""
    v = (plane * ref.nms_mask(plane)).reshape(-1)
    idx = np.flatnonzero(v > 0)
    idx = idx[np.lexsort((idx, -v[idx]))]
    return idx, v[idx]


def check_candidates_case(case):
    hr, wr = case["hr"], case["wr"]
    npix = hr * wr
    assert n_tiles(npix) == 3 and npix - 2 * BU_TILE == 1408 and BU_TILE % wr and (2 * BU_TILE) % wr
    assert 0 < case["dev_t"] < 1e-4
    hm = case["hm"].astype(np.float64)
    assert np.array_equal(hm[1], hm[0][::-1]) and ((hm > 0) | ((hm >= f32(-0.2)) & (hm <= f32(-0.1)))).all()
    top = candidates_expected(30)
    tile = lambda i: np.asarray(i) // BU_TILE      # noqa: E731
    # plane 0
    idx, val = _survivors(hm[0, 0])
    assert len(np.unique(val)) == len(val) and all((tile(idx) == t).sum() >= 31 for t in range(3))
    assert set(tile(top[0]["ind"][0])) == {0, 1, 2} and np.array_equal(top[0]["ind"][0], idx[:30])
    # plane 1
    idx, val = _survivors(hm[0, 1])
    assert (tile(idx[:30]) == 2).all() and all((tile(idx) == t).sum() >= 30 for t in (0, 1))
    assert np.array_equal(top[0]["ind"][1], idx[:30])
    # plane 2
    idx, val = _survivors(hm[0, 2])
    run = np.sort(idx[val == f32(0.5)])
    assert len(idx) == 45 and len(run) == 40 and len(np.unique(val[:5])) == 5 and val[4] > 0.5
    assert all((tile(run) == t).sum() >= 2 for t in range(3))
    assert np.array_equal(top[0]["ind"][2][5:], run[:25]) and set(tile(run[:25])) == {0, 1} and (tile(run[25:]) >= 1).all()
    # plane 3
    assert np.array_equal(top[0]["ind"][3], np.arange(30)) and (top[0]["val"][3] == f32(0.25)).all()
    # plane 4
    idx, val = _survivors(hm[0, 4])
    assert len(idx) == 7 and (tile(idx) == 1).all() and (top[0]["val"][4] > 0).sum() == 7
    # plane 5
    idx, val = _survivors(hm[0, 5])
    assert idx.tolist() == PAIRS_WANT
    assert [int(t) for t in tile(PAIRS_WANT)] == [0, 1, 1, 2, 1, 2]
    # the others, and frame 1
    assert (hm[0, 6:] < 0).all() and not (top[0]["val"][6:] > 0).any()
    for key in ("val", "ind"):
        on = top[0]["val"] > 0
        assert np.array_equal(np.where(on, top[0][key], -1)[::-1], np.where(top[1]["val"] > 0, top[1][key], -1))


# ---- B. pp_bottomup_refine: 2 spans of 8256 pixels, 3 spans of 8235 (the last one short) ---------------------------------------------
REFINE_SHAPES = ((128, 129), (128, 193))
REFINE_FRAMES = (0, 1, 0)       # person_frame
# what the planes of frame 0 hold in the exact variant, by joint (frame 1: the same list rotated by one)
EXACT_KINDS = ("first", "middle", "last", "last_pixel", "tie", "negative") * 2 + ("middle", "last", "tie", "negative", "last_pixel")


def refine_rule(hm, tags, mean_tag, dt=np.float64):
    """HeatmapParser.refine's scan of one plane (tests/bottomup_ref.py::refine_person) for a GIVEN mean tag: hm [H][W],
    tags [H][W][2], in dtype dt -> (flat index of the winner, distances [H][W], scores [H][W])"""
    hm, tags, prev = hm.astype(dt), tags.astype(dt), np.asarray(mean_tag, dt)
    d = (((tags - prev[None, None, :]) ** 2).sum(axis=2) ** 0.5).astype(dt)
    norm = (hm - np.round(d)).astype(dt)
    return int(np.argmax(norm)), d, norm


def refine_row(plane, p):
    """the record pp_bottomup_refine returns for the winner p of a plane: (x, y, value, bit 0: below > above | bit 1: right > left)"""
    h, w = plane.shape
    y, x = divmod(int(p), w)
    by = plane[min(h - 1, y + 1), x] > plane[max(0, y - 1), x]
    bx = plane[y, min(w - 1, x + 1)] > plane[y, max(0, x - 1)]
    return np.array([x, y, plane[y, x], int(by) | 2 * int(bx)], f32)


def _row_in_span(rng, s, npix, wr):
    """a row that lies in span s entirely"""
    span = span_len(npix)
    lo, hi = -(-s * span // wr), min((s + 1) * span, npix) // wr
    assert lo < hi
    return int(rng.integers(lo, hi))


@functools.lru_cache(maxsize=None)
def refine_exact_case(hw):
    """All tag planes zero: with mean tag (0, 0) every distance is exactly 0 and the score is the heat-map value; with (3, 4) it is
    exactly 5 everywhere.  dict(s0, s1, hm [2][17][H][W] float32 in (-1, -0.1) but for what `kinds` says, kinds [2][17], calls):
    calls = two (person_frame, mean_tag [P][2], need [P][17]) triples, the second one smaller."""
    hr, wr = hw
    npix, ns = hr * wr, n_split(hr * wr)
    rng = np.random.default_rng(hr * wr)
    s0, s1 = _sources(rng, 2, 8, 12)
    s0[:, K:] = 0
    hm = rng.uniform(-1.0, -0.1, (2, K, hr, wr)).astype(f32)
    kinds = [list(EXACT_KINDS), list(EXACT_KINDS[1:] + EXACT_KINDS[:1])]
    for fr in range(2):
        for c, kind in enumerate(kinds[fr]):
            m = hm[fr, c]
            x = int(rng.integers(0, wr))
            if kind in ("first", "middle", "last"):
                m[_row_in_span(rng, {"first": 0, "middle": ns // 2, "last": ns - 1}[kind], npix, wr), x] = rng.uniform(0.3, 0.9)
            elif kind == "last_pixel":
                m[hr - 1, wr - 1] = 0.6
            elif kind == "tie":                       # the later one first in x, so that "lower index" is not "lower x"
                m[_row_in_span(rng, ns - 1, npix, wr), wr // 4] = m[_row_in_span(rng, ns - 2, npix, wr), wr // 2] = 0.7
            else:                                     # all negative: the winner clears the rest by 0.05
                m[_row_in_span(rng, ns - 1, npix, wr), x] = -0.05
    need0 = np.array([[(c + p) % 3 != 0 for c in range(K)] for p in range(3)], np.int32)
    need1 = np.array([[c % 2 == 0 for c in range(K)]], np.int32)
    calls = ((np.array(REFINE_FRAMES, np.int32), np.zeros((3, 2), f32), need0), (np.array([1], np.int32), np.array([[3, 4]], f32), need1))
    return _freeze(dict(s0=s0, s1=s1, hm=hm, hr=hr, wr=wr)) | dict(kinds=kinds, calls=calls)


def refine_exact_expected(case, call):
    """[P][17][4] float32: np.argmax of the plane (the lowest index among equal maxima), zero rows where need == 0"""
    frames, _, need = call
    out = np.zeros((len(frames), K, 4), f32)
    for p, fr in enumerate(frames):
        for c in range(K):
            if need[p, c]:
                out[p, c] = refine_row(case["hm"][fr, c], np.argmax(case["hm"][fr, c].astype(np.float64)))
    return out


def check_refine_exact_case(case):
    hr, wr = case["hr"], case["wr"]
    npix, ns, span = hr * wr, n_split(hr * wr), span_len(hr * wr)
    assert ns == {16512: 2, 24704: 3}[npix] and span == {16512: 8256, 24704: 8235}[npix] and (ns * span > npix) == (npix == 24704)
    hm = case["hm"].astype(np.float64)
    tags = np.zeros((hr, wr, 2))
    seen = set()
    for fr in range(2):
        for c, kind in enumerate(case["kinds"][fr]):
            m = hm[fr, c]
            p = int(np.argmax(m))
            best = np.flatnonzero(m.reshape(-1) == m.max())
            assert np.sort(m.reshape(-1))[-1 - len(best)] < m.max() - 0.04          # a margin float32 rounding of (hm - 5) cannot close
            for mean in ((0, 0), (3, 4)):             # the rule itself: distance 0 / 5, the same winner
                q, d, _ = refine_rule(m, tags, mean)
                assert q == p and (d == np.hypot(*mean)).all()
            assert len(best) == (2 if kind == "tie" else 1) and (m.max() < 0) == (kind == "negative")
            if kind == "tie":
                assert best[0] // span != best[1] // span and best[0] % wr > best[1] % wr
            if kind == "last_pixel":
                assert p == npix - 1
            if kind in ("first", "middle", "last"):
                assert p // span == {"first": 0, "middle": ns // 2, "last": ns - 1}[kind]
            seen.add(p // span)
    assert seen == set(range(ns))
    (fr0, mt0, need0), (fr1, mt1, need1) = case["calls"]
    assert fr0.tolist() == list(REFINE_FRAMES) and len(fr1) < len(fr0) and not np.array_equal(need0[:1], need1) and not np.array_equal(mt0[:1], mt1)
    for need in (need0, need1):
        assert all(0 < row.sum() < K and (np.diff(row) != 0).sum() >= 5 for row in need)      # zeros interleaved with ones


REFINE_TAG_SEEDS = {(128, 129): 12, (128, 193): 1}      # chosen on the CPU: check_refine_tag_case holds (tests/test_selection_cases.py)


@functools.lru_cache(maxsize=None)
def refine_tag_case(hw, seed=None):
    """Tag planes with two regions, the left columns near 0 and the right ones near 3 (noise 0.02; the bilinear transition lies in
    the middle columns, every peak keeps clear of it).  Plane (frame, joint) is meant for a person of the region `(joint + frame) % 2`
    (0: left): the plane's maximum 0.9 lies in the OTHER region, in span 0, where the distance rounds to 4; the winner 0.6 lies in a
    later span of the right region, a decoy 0.4 in its span 0.  Persons: frames (0, 1, 0), mean tags (0, 0), (3, 3), (3, 3)."""
    hr, wr = hw
    npix, ns = hr * wr, n_split(hr * wr)
    rng = np.random.default_rng(REFINE_TAG_SEEDS[hw] if seed is None else seed)
    h0, w0 = 8, 12
    s0, s1 = _sources(rng, 2, h0, w0)
    region = np.where(np.arange(w0) < w0 // 2, 0.0, 3.0)[None, None, None, :]
    s0[:2, K:] = region + rng.normal(0, 0.02, (2, K, h0, w0))
    s0[2:, K:] = region[..., ::-1] + rng.normal(0, 0.02, (2, K, h0, w0))      # the mirrored samples: un-mirrored, the same two regions
    hm = rng.uniform(-0.2, -0.1, (2, K, hr, wr)).astype(f32)
    cols = (np.arange(2, int(0.35 * wr)), np.arange(int(0.65 * wr) + 1, wr - 2))
    for fr in range(2):
        for c in range(K):
            side = (c + fr) % 2
            hm[fr, c, _row_in_span(rng, 0, npix, wr), rng.choice(cols[1 - side])] = 0.9
            hm[fr, c, _row_in_span(rng, 0, npix, wr), rng.choice(cols[side])] = 0.4
            hm[fr, c, _row_in_span(rng, 1 + (c // 2) % (ns - 1), npix, wr), rng.choice(cols[side])] = 0.6
    frames = np.array(REFINE_FRAMES, np.int32)
    mean_tag = np.array([[0, 0], [3, 3], [3, 3]], f32)
    need = np.array([[(c + fr) % 2 == (mt[0] > 1) for c in range(K)] for fr, mt in zip(frames, mean_tag)], np.int32)
    _, tags64 = ref.aggregate(s0, s1, hr, wr, True, np.float64)
    _, tags32 = ref.aggregate(s0, s1, hr, wr, True, f32)
    dev_t = float(np.abs(tags32.astype(np.float64) - tags64).max())
    return _freeze(dict(s0=s0, s1=s1, hm=hm, tags64=tags64, tags32=tags32, frames=frames, mean_tag=mean_tag, need=need, dev_t=dev_t, hr=hr, wr=wr))


def refine_tag_scans(case):
    """per needed (person, joint): (person, joint, winner, distances, scores) of the float64 rule, and dev_h = the largest deviation
    of the float32 rule's scores from them (the heat-maps are written directly, so that is the rounding of the score alone)"""
    scans, dev_h = [], 0.0
    for p, fr in enumerate(case["frames"]):
        for c in np.flatnonzero(case["need"][p]):
            q, d, norm = refine_rule(case["hm"][fr, c], case["tags64"][fr, c], case["mean_tag"][p])
            _, _, norm32 = refine_rule(case["hm"][fr, c], case["tags32"][fr, c], case["mean_tag"][p], f32)
            dev_h = max(dev_h, float(np.abs(norm32.astype(np.float64) - norm).max()))
            scans.append((p, int(c), q, d, norm))
    return scans, dev_h


def refine_tag_expected(case, scans):
    out = np.zeros((len(case["frames"]), K, 4), f32)
    for p, c, q, _, _ in scans:
        out[p, c] = refine_row(case["hm"][case["frames"][p], c], q)
    return out


def check_refine_tag_case(case, scans, dev_h):
    """the margins, from the float64 reference alone: no distance within 10 x 4 x dev_t of a rounding step (a distance moves by less
    than 4 x what its tags move by: two points, two dimensions), the winner ahead by more than 10 x dev_h"""
    hr, wr = case["hr"], case["wr"]
    ns, span = n_split(hr * wr), span_len(hr * wr)
    assert ns >= 2 and 0 < case["dev_t"] < 1e-4 and 0 < dev_h < 1e-5
    margin_t, margin_h = 10 * 4 * case["dev_t"], 10 * dev_h
    spans = set()
    for p, c, q, d, norm in scans:
        assert (np.abs(d - np.floor(d) - 0.5) > margin_t).all(), "a tag distance at a rounding step"
        s = np.sort(norm.reshape(-1))
        assert s[-1] - s[-2] > margin_h, "the refine arg-max is not robust"
        m = case["hm"][case["frames"][p], c].astype(np.float64)
        top = int(np.argmax(m))
        assert top != q and top // span == 0 and np.round(d.reshape(-1)[top]) >= 1        # the heat-map maximum: wrong region, span 0
        assert q // span >= 1 and np.round(d.reshape(-1)[q]) == 0 and m.reshape(-1)[q] == f32(0.6)
        spans.add(q // span)
    assert spans == set(range(1, ns)) and len(scans) == int(case["need"].sum()) >= K
    assert {tuple(t) for t in case["mean_tag"].tolist()} == {(0.0, 0.0), (3.0, 3.0)} and 0 < case["need"].sum(1).min()


# ---- C. pp_fairmot_decode / pp_trades_decode: more than 256 peaks per frame ------------------------------------------------------
DECODE_HW = (40, 56)
DECODE_KS = (1, 255, 256, 257, 500, 560, 600)
DECODE_FRAMES = ("lattice", "random", "flat", "saturated")
TIED = f32(1.25)


@functools.lru_cache(maxsize=None)
def decode_maps():
    """dict(hm [4][40][56][1], fairmot = (wh, reg, id), trades = (reg, ltrb, tracking)), all [4][40][56][c] float32; the side maps as
    the decode tests of tests/test_gpu_fairmot.py and tests/test_gpu_trades.py draw them"""
    h, w = DECODE_HW
    rng = np.random.default_rng(7)
    lattice = rng.uniform(-6, -3, (h, w)).astype(f32)
    lattice[::2, ::2] = rng.uniform(-2, 3, (h // 2, w // 2))
    ly, lx = np.meshgrid(np.arange(0, h, 2), np.arange(0, w, 2), indexing="ij")
    cells = rng.permutation(ly.size)
    lattice[ly.ravel()[cells[:60]], lx.ravel()[cells[:60]]] = TIED
    saturated = lattice.copy()
    saturated[ly.ravel()[cells[60:360]], lx.ravel()[cells[60:360]]] = 40.0
    hm = np.stack([lattice, rng.uniform(-6, 1, (h, w)).astype(f32), np.full((h, w), 0.5, f32), saturated])[..., None]
    n = len(hm)
    fairmot = (rng.uniform(0.5, 6, (n, h, w, 4)).astype(f32), rng.uniform(0, 1, (n, h, w, 2)).astype(f32),
               rng.standard_normal((n, h, w, 128)).astype(f32))
    trades = (rng.uniform(0, 1, (n, h, w, 2)).astype(f32), (rng.uniform(0.5, 6, (n, h, w, 4)) * [-1, -1, 1, 1]).astype(f32),
              rng.uniform(-3, 3, (n, h, w, 2)).astype(f32))
    for a in fairmot + trades:
        a.setflags(write=False)
    return _freeze(dict(hm=np.ascontiguousarray(hm))) | dict(fairmot=fairmot, trades=trades)


@functools.lru_cache(maxsize=None)
def fairmot_expected(frame, k, feat_dtype=np.float64):
    m = decode_maps()
    return FR.decode(m["hm"][frame], *(a[frame] for a in m["fairmot"]), k, feat_dtype)


@functools.lru_cache(maxsize=None)
def trades_expected(frame, k):
    m = decode_maps()
    return TR.decode(m["hm"][frame], *(a[frame] for a in m["trades"]), k)


def check_decode_maps(maps):
    """peak counts, chunk counts and tie structure, from fairmot_ref.decode alone.  Returns the peak count of every frame."""
    h, w = DECODE_HW
    hm = maps["hm"]
    counts = []
    for frame, kind in enumerate(DECODE_FRAMES):
        dets, _, inds = fairmot_expected(frame, h * w)
        dets_t, inds_t = trades_expected(frame, h * w)
        assert np.array_equal(inds, inds_t) and np.array_equal(dets[:, 4], dets_t[:, 8])      # one selection rule, two references
        peaks = inds[inds >= 0]
        score = dets[:len(peaks), 4]
        counts.append(len(peaks))
        assert -(-len(peaks) // RANK_CHUNK) >= 2, kind           # more than one chunk of fm_rank_of, more than one rank workgroup
        assert (np.diff(score) <= 0).all() and (np.diff(peaks)[np.diff(score) == 0] > 0).all()
        flat = hm[frame].reshape(-1)
        if kind == "lattice":
            assert len(peaks) == 560 and len(np.unique(score)) == 501
            tied = peaks[flat[peaks] == TIED]
            assert len(tied) == 60 and (np.diff(tied) > 0).all() and tied.max() - tied.min() > RANK_CHUNK
        if kind == "random":
            assert len(peaks) > RANK_CHUNK and len(np.unique(score)) == len(peaks)
        if kind == "flat":
            assert np.array_equal(inds, np.arange(h * w))
        if kind == "saturated":
            one = peaks[score == f32(1.0)]
            assert len(peaks) == 560 and len(one) == 300 > RANK_CHUNK and np.array_equal(one, np.sort(np.flatnonzero(flat == f32(40.0))))
            assert np.array_equal(peaks[:300], one)
    assert counts[0] == 560 and max(DECODE_KS) == 600 and 560 in DECODE_KS
    return counts
