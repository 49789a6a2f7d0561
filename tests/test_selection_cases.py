"""The inputs of tests/test_gpu_selection_wide.py are what their builders say (tests/selection_cases.py), from the references alone:
tile, span and chunk counts above 1, top-30 membership across tiles, peak counts above 256, and the margins the exact comparisons
of the refine scan rest on.  No GPU."""
import numpy as np
import pytest

from tests import bottomup_ref as ref
from tests import selection_cases as S


def test_candidate_planes_span_three_tiles():
    case = S.candidates_case()
    assert S.n_tiles(case["hr"] * case["wr"]) == 3
    S.check_candidates_case(case)
    for m in S.CAND_MAX_PEOPLE:                     # a smaller max_people is a prefix of a larger one's result
        top, top64 = S.candidates_expected(m), S.candidates_expected(64)
        for fr in range(case["f"]):
            on = top[fr]["val"] > 0
            assert np.array_equal(top[fr]["ind"][on], top64[fr]["ind"][:, :m][on])
    print(f"candidates: float32 reference tags vs float64 {case['dev_t']:.3e}")


@pytest.mark.parametrize("hw", S.REFINE_SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_refine_exact_planes_put_winners_in_every_span(hw):
    case = S.refine_exact_case(hw)
    assert S.n_split(hw[0] * hw[1]) > 1
    S.check_refine_exact_case(case)
    want = S.refine_exact_expected(case, case["calls"][0])
    need = case["calls"][0][2]
    assert not want[need == 0].any() and (want[need != 0][:, 2] != 0).all()


@pytest.mark.parametrize("hw", S.REFINE_SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_refine_tag_planes_have_their_margins(hw):
    case = S.refine_tag_case(hw)
    scans, dev_h = S.refine_tag_scans(case)
    S.check_refine_tag_case(case, scans, dev_h)
    print(f"refine {hw}: float32 reference vs float64: tags {case['dev_t']:.3e}, scores {dev_h:.3e}")


def test_refine_rule_is_the_references_scan():
    """`refine_rule` takes the mean tag as an argument; ref.refine_person derives it from the person's detected joints.  Given that
    mean, both pick the same pixel on every plane they scan."""
    case = S.refine_tag_case(S.REFINE_SHAPES[0])
    hm, tags = case["hm"][0].astype(np.float64), case["tags64"][0]
    person = np.zeros((S.K, 5), np.float32)
    person[0, :3] = (10, 20, 0.5)                   # one detected joint, in the left region
    trace = []
    ref.refine_person(hm, tags, person, np.float64, trace=trace)
    prev = tags[0, 20, 10]
    assert len(trace) == S.K - 1 and np.abs(prev).max() < 0.2
    for rec in trace:
        q, d, _ = S.refine_rule(hm[rec["joint"]], tags[rec["joint"]], prev)
        assert divmod(q, case["wr"]) == (rec["y"], rec["x"]) and np.array_equal(d, rec["d"])


def test_decode_frames_have_more_than_one_rank_chunk():
    counts = S.check_decode_maps(S.decode_maps())
    assert all(-(-c // S.RANK_CHUNK) > 1 for c in counts)
    print("decode: peaks per frame", dict(zip(S.DECODE_FRAMES, counts)))
    for frame in range(len(S.DECODE_FRAMES)):       # K = 600 on 560 peaks: 40 empty slots; the flat frame has none
        dets, feats, inds = S.fairmot_expected(frame, 600)
        empty = inds < 0
        assert empty.sum() == max(0, 600 - counts[frame]) and not dets[empty].any() and not feats[empty].any()
