"""tracking.TracktorTracker on the CPU: a scripted scenario through stub `regress` / `embed` callables, with the expected ids per
frame written out by hand AND compared (ids, boxes, scores) with the loop-by-loop transcription tests/tracktor_ref.TracktorRef,
whose trace shows that every branch of the flow was taken.  Plus the float64 ECC reference on its own inputs.

The scene: persons stand on "lanes"; lane k is the box [100 k + 30, 20, 100 k + 70, 100].  The regress stub returns each box as
it came with the lane's scripted score (a frame's script may move a box or change a score); the embed stub returns 3 * e_a for
appearance a (by default the lane), so different appearances are 3 sqrt(2) > 2.0 apart and equal ones 0."""
import numpy as np
import pytest

from posepipeline_amd.tracking import TracktorTracker
from tests import tracktor_ref as R

f32 = np.float32
LANE_SCORE = {0: 0.9, 1: 0.8, 2: 0.7, 3: 0.85, 6: 0.6}


def lane_box(k, dx=0.0):
    return np.array([100 * k + 30 + dx, 20, 100 * k + 70 + dx, 100], f32)


def lane_of(box):
    return int(round(((box[0] + box[2]) / 2 - 50) / 100))


def det(k, score):
    return np.concatenate([lane_box(k), [score]]).astype(f32)


IDENT = np.array([[1.0, 0, 0], [0, 1.0, 0]])
TH = 0.01
SMALL = np.array([[np.cos(TH), -np.sin(TH), 3.0], [np.sin(TH), np.cos(TH), -2.0]])

# per frame: (frame_id, detections, regress score overrides by lane, lane whose box regresses ONTO another lane's (+2 px),
#             appearance overrides by lane, warp, expected ids)
SCRIPT = [
    (0, [det(0, .9), det(1, .8), det(2, .7), det(5, .4)], {}, None, {}, None, [0, 1, 2]),          # start; a detection <= .5 is ignored
    (1, [det(0, .9), det(1, .8), det(2, .7), det(3, .95)], {}, None, {}, IDENT, [0, 1, 2, 3]),     # propagation; 3 detections suppressed (IoU .3)
    (2, [], {1: 0.3}, None, {}, IDENT, [0, 3, 2]),                                                  # track 1 killed by score; output by score
    (3, [det(1, .9)], {}, (3, 2), {}, SMALL, [0, 3, 1]),                                            # track 2 killed by the .6 NMS; 1 re-identified
    (4, [det(6, .9)], {}, None, {6: 2}, IDENT, [0, 1, 3, 4]),                                       # looks like lost track 2, IoU 0: refused
] + [(f, [], {}, None, {}, IDENT, [0, 1, 3, 4]) for f in range(5, 13)] + [                          # track 2 (last seen in 2) dropped at 12
    (0, [det(0, .9), det(1, .8)], {}, None, {}, None, [0, 1]),                                      # frame_id 0: restart from empty
]


def stubs(score_over, onto, app_over):
    def regress(boxes):
        boxes = np.asarray(boxes, f32).reshape(-1, 4)
        lanes = [lane_of(b) for b in boxes]
        out = boxes.copy()
        scores = np.array([score_over.get(k, LANE_SCORE[k]) for k in lanes], f32)
        if onto is not None:
            src, dst = onto
            out[lanes.index(src)] = boxes[lanes.index(dst)] + np.array([2, 0, 2, 0], f32)
            scores[lanes.index(src)] = LANE_SCORE[src]
        return out, scores

    def embed(boxes):
        e = np.zeros((len(boxes), 8), f32)
        for r, b in enumerate(np.asarray(boxes, f32).reshape(-1, 4)):
            k = lane_of(b)
            e[r, app_over.get(k, k)] = 3.0
        return e
    return regress, embed


def test_scripted_scenario_takes_every_branch():
    trk = TracktorTracker()
    ref = R.TracktorRef()
    dropped_at = None
    for step, (fid, dets, score_over, onto, app_over, warp, expect) in enumerate(SCRIPT):
        regress, embed = stubs(score_over, onto, app_over)
        dets = np.array(dets, f32).reshape(-1, 5)
        rows = trk.step(fid, dets, regress, embed, warp)
        want = ref.step(fid, dets, regress, embed, warp)
        assert [int(r[0]) for r in rows] == expect, (step, rows)
        assert rows.dtype == np.float32 and np.array_equal(rows, want), (step, rows, want)
        assert trk.live_ids() == set(ref.tracks), step
        if ref.trace[-1]["dropped"]:
            dropped_at = (step, ref.trace[-1]["dropped"])
    t = ref.trace
    assert t[1]["propagated"] == [0, 1, 2] and t[1]["suppressed"] == 3 and t[1]["new"] == [3]
    assert t[2]["killed_score"] == [1] and t[2]["propagated"] == [0, 3, 2]
    assert t[3]["killed_nms"] == [2] and t[3]["reid"] == [1] and t[3]["propagated"] == [0, 3]
    assert t[4]["gated"] == [2] and t[4]["reid"] == [] and t[4]["new"] == [4]
    assert dropped_at == (12, [2])
    assert t[13]["new"] == [0, 1] and t[13]["propagated"] == []


def test_warp_is_applied_to_every_track_in_float32():
    trk = TracktorTracker()
    regress, embed = stubs({}, None, {})
    trk.step(0, np.array([det(0, .9), det(2, .7)], f32), regress, embed, None)
    trk.step(1, np.zeros((0, 5), f32), lambda b: (b, np.zeros(len(b), f32)), embed, IDENT)      # both tracks lost in frame 1
    trk.step(2, np.zeros((0, 5), f32), regress, embed, SMALL)                                   # nothing regressed: last != frame - 1
    m = SMALL.astype(f32)
    for i, k in ((0, 0), (1, 2)):
        b = lane_box(k)
        want = np.array([(m[0, 0] * b[0] + m[0, 1] * b[1]) + m[0, 2], (m[1, 0] * b[0] + m[1, 1] * b[1]) + m[1, 2],
                         (m[0, 0] * b[2] + m[0, 1] * b[3]) + m[0, 2], (m[1, 0] * b[2] + m[1, 1] * b[3]) + m[1, 2]], f32)
        assert np.array_equal(trk.tracks[i]["box"], want) and trk.tracks[i]["last"] == 0


@pytest.mark.parametrize("shape", R.ECC_SHAPES, ids=lambda s: "%dx%d" % s)
def test_reference_ecc_recovers_the_known_motions(shape):
    """the float64 reference itself on the inputs of tests/test_gpu_tracktor.py, at the configured rule (100, 1e-5): 4 - 7
    iterations, and the truth within 0.01 px / 1e-4 rad -- half of what the GPU test allows the kernel (0.02 px, 2e-4 rad).
    Observed here: 4 - 6 iterations, at worst 8.8e-3 px and 7.5e-5 rad (50 x 70); 96 x 128 alone stays below 4e-3 px.  The
    stopping rule ends the loop while successive iterates still move by ~1e-3 px on the small image."""
    for (tmpl, img), motion in zip(R.ecc_test_pairs(*shape), R.ECC_MOTIONS):
        M, rho, it, status = R.ecc_euclidean(tmpl, img, 100, 1e-5)
        assert status == R.ECC_OK and 4 <= it <= 7 and rho > 0.99, (motion, it, rho)
        assert abs(np.arcsin(M[1, 0]) - motion[0]) <= 1e-4 and np.abs(M[:, 2] - motion[1:]).max() <= 0.01, (motion, M)


def test_reference_ecc_degenerate_inputs():
    img = R.sinusoid_image(50, 70, 3)
    M, rho, it, status = R.ecc_euclidean(img, img, 100, 1e-5)
    assert status == R.ECC_OK and it == 2 and np.abs(M - IDENT).max() <= 1e-12 and abs(rho - 1) < 1e-12
    assert R.ecc_euclidean(img, np.full((50, 70), 0.3), 100, 1e-5)[3] == R.ECC_NAN


def test_qdtrack_still_raises_and_unknown_names_too():
    from posepipeline_amd.wrappers import mmtrack as wmt
    with pytest.raises(NotImplementedError, match="qdtrack"):
        wmt.mmtrack_bounding_boxes("no_such_file", "qdtrack")
    with pytest.raises(Exception, match="Unknown config file"):
        wmt.mmtrack_bounding_boxes("no_such_file", "tracktor2")
    assert wmt.mmtrack_bounding_boxes.__defaults__ == ("tracktor",) and (wmt.ECC_ITERS, wmt.ECC_EPS) == (100, 1e-5)
