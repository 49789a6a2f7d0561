"""Inputs with tied, saturated, empty and capped data for the selection kernels (nms.hip, det_post.hip), and the oracle-side
statements of what each one exercises.  Shared by tests/test_detect_post_scenarios.py (no GPU: the inputs and their edges) and
the GPU tests that feed them to the kernels (tests/test_gpu_detect_post.py, tests/test_gpu_pipeline.py)."""
import numpy as np

from oracle import boxes as obox
from oracle import detector as odet
from posepipeline_amd.models import faster_rcnn as fr
from posepipeline_amd.models import synth

f32 = np.float32
SRC_H, SRC_W = 135, 240
RPN_CLS_W, RPN_CLS_B = "detector.rpn_head.rpn_cls.weight", "detector.rpn_head.rpn_cls.bias"
RPN_REG_W, RPN_REG_B = "detector.rpn_head.rpn_reg.weight", "detector.rpn_head.rpn_reg.bias"
FC_CLS_W, FC_CLS_B = "detector.roi_head.bbox_head.fc_cls.weight", "detector.roi_head.bbox_head.fc_cls.bias"
FC_REG_W = "detector.roi_head.bbox_head.fc_reg.weight"
HEAD_KEYS = (RPN_CLS_W, RPN_CLS_B, RPN_REG_W, RPN_REG_B, FC_CLS_W, FC_CLS_B, FC_REG_W)


# ---- standalone NMS under mass ties -----------------------------------------------------------------------------------------
NMS_SIZES = (1, 2, 15, 63, 64, 65, 128, 129, 4096, 8192)     # both sides of the 64-box mask tile and of the sort's power-of-two padding


def tie_box_sets(n):
    """-> [(name, x1y1x2y2 float64 [n][4], scores float64 [n])]: every score equal on a regular grid of overlapping boxes (the kept
    set then depends on the tie order alone) and on identical boxes; three (n < 4096) or four score levels on random boxes."""
    cols = max(1, int(np.ceil(np.sqrt(n))))
    while n > 1 and ((n - 1) % cols + (n - 1) // cols) % 2 == 0:
        cols += 1                           # the greedy pass keeps a checkerboard: put the last box on the other colour than the first
    i = np.arange(n)
    x, y = (i % cols) * 6.0, (i // cols) * 6.0
    grid = np.stack([x, y, x + 10.0, y + 10.0], 1)                 # neighbours overlap by 4 of 10 px (IoU .25 / .43 with the +1 areas)
    same = np.tile([[20.0, 30.0, 60.0, 110.0]], (n, 1))
    rng = np.random.default_rng(n)
    ctr = rng.uniform(0, 400, (n, 2))
    wh = rng.uniform(8, 40, (n, 2))
    rnd = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).round()
    levels = np.array([0.9, 0.7, 0.5, 0.3] if n >= 4096 else [0.8, 0.6, 0.4])
    return [("grid", grid, np.full(n, 0.75)), ("identical", same, np.full(n, 0.75)),
            ("levels", rnd, levels[rng.integers(0, len(levels), n)])]


def to_convention(boxes_xyxy, scores, convention):
    """the same boxes in the layout of a convention: 0 float32 x1y1x2y2, 1 float64 tlwh, 2 float32 y1x1y2x2"""
    b = np.asarray(boxes_xyxy, np.float64)
    if convention == 0:
        return b.astype(f32), scores.astype(f32)
    if convention == 1:
        return np.concatenate([b[:, :2], b[:, 2:] - b[:, :2]], 1), scores.astype(np.float64)
    return b[:, [1, 0, 3, 2]].astype(f32), scores.astype(f32)


def tf_nms_all(boxes_yxyx, scores, iou_thr):
    """oracle.yolo.tf_nms with max_output_size = n, vectorised over the candidates (same float32 operations, same order: descending
    score, ties lower index first); pinned to tf_nms at small n by tests/test_detect_post_scenarios.py"""
    b = np.asarray(boxes_yxyx, f32)
    s = np.asarray(scores, f32)
    order = np.argsort(-s, kind="stable")
    y1, y2 = np.minimum(b[:, 0], b[:, 2])[order], np.maximum(b[:, 0], b[:, 2])[order]
    x1, x2 = np.minimum(b[:, 1], b[:, 3])[order], np.maximum(b[:, 1], b[:, 3])[order]
    area = ((y2 - y1) * (x2 - x1)).astype(f32)
    thr = f32(iou_thr)
    suppressed = np.zeros(len(b), bool)
    keep = []
    for i in range(len(b)):
        if suppressed[i]:
            continue
        keep.append(int(order[i]))
        if area[i] <= 0:
            continue
        r = slice(i + 1, len(b))
        ih = np.maximum((np.minimum(y2[i], y2[r]) - np.maximum(y1[i], y1[r])).astype(f32), f32(0))
        iw = np.maximum((np.minimum(x2[i], x2[r]) - np.maximum(x1[i], x1[r])).astype(f32), f32(0))
        inter = (ih * iw).astype(f32)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = (inter / ((area[i] + area[r]).astype(f32) - inter).astype(f32)).astype(f32)
        suppressed[r] |= (area[r] > 0) & (iou > thr)
    return keep


def nms_reference(boxes, scores, thr, convention):
    """the kept list each convention promises (nms.hip header), in the layout of `to_convention`"""
    if convention == 0:
        return obox.nms_mmcv(boxes, scores, thr)
    if convention == 1:
        return obox.nms_deepsort_stable(boxes, thr, scores)
    return tf_nms_all(boxes, scores, thr)


# ---- the detector's head tensors ----------------------------------------------------------------------------------------
def tamed_state_dict():
    """tests/test_gpu_detector.py's weights: He-normal heads scaled so that every selection sees a spread of values"""
    sd = synth.synth_state_dict(fr.faster_rcnn_param_shapes(), seed=2)
    for k, g in ((RPN_CLS_W, 0.5), (RPN_REG_W, 0.1), (FC_REG_W, 0.2)):
        sd[k] = (sd[k] * g).astype(f32)
    return sd


def threshold_biases():
    """fc_cls biases (fg, bg) whose softmax_fg is exactly float32(0.05), the score threshold ("eq": the strict > drops every RoI)
    and exactly the next float32 up ("up": every RoI passes), found on the float32 grid of the background bias"""
    thr = f32(0.05)
    want = {"eq": thr, "up": np.nextafter(thr, f32(1))}
    fg = f32(np.log(0.05 / 0.95))
    found = {}
    for k in range(-4096, 4097):
        bg = f32(k * 2.0 ** -28)
        s = odet.softmax_fg(np.array([[fg, bg]], f32))[0]
        for name, v in want.items():
            if s == v and name not in found:
                found[name] = np.array([fg, bg], f32)
    return found


DX_EMPTY = 1e12        # * anchor width: the centre lands where one float32 ulp exceeds the box -> x1 == x2, dropped by rpn_compact
DX_OFF = 128.0         # * anchor width: past the right edge of the padded input for every anchor and dw -> RoIAlign samples nothing


def scenarios():
    """name -> (state dict, edge).  Each changes only the 1x1 head tensors of the tamed weights (the backbone stays the one
    tests/test_gpu_detector.py pins against the oracle bit for bit); `edge` names what the GPU test asserts on the oracle side"""
    base = tamed_state_dict()

    def variant(**upd):
        sd = dict(base)                     # the backbone arrays are shared, not copied
        sd.update({k: np.ascontiguousarray(v, f32) for k, v in upd.items()})
        return sd

    reg_b = base[RPN_REG_B].copy()
    one_type = reg_b.copy()
    one_type[4] = DX_EMPTY                  # anchor type 1 (ratio 1): dx of every level
    all_types = reg_b.copy()
    all_types[0::4] = DX_EMPTY
    off = reg_b.copy()
    off[0::4] = DX_OFF
    tb = threshold_biases()
    return {
        "saturated_rpn": (variant(**{RPN_CLS_W: base[RPN_CLS_W] * 400}), "rpn_cut_in_tie"),
        "constant_rpn": (variant(**{RPN_CLS_W: np.zeros_like(base[RPN_CLS_W]), RPN_CLS_B: [0.25, 1.5, -0.75]}), "rpn_all_tied"),
        "empty_one_type": (variant(**{RPN_REG_B: one_type}), "some_dropped"),
        "empty_all_types": (variant(**{RPN_REG_B: all_types}), "no_proposals"),
        "off_image": (variant(**{RPN_REG_B: off}), "rois_sample_nothing"),
        "threshold_eq": (variant(**{FC_CLS_W: np.zeros_like(base[FC_CLS_W]), FC_CLS_B: tb["eq"]}), "all_at_threshold"),
        "threshold_up": (variant(**{FC_CLS_W: np.zeros_like(base[FC_CLS_W]), FC_CLS_B: tb["up"]}), "det_cut_in_tie"),
        "saturated_roi": (variant(**{FC_CLS_W: base[FC_CLS_W] * 4000}), "det_cut_in_tie"),
    }


# ---- frames ----------------------------------------------------------------------------------------------------------------
def synth_frame(rng, h, w):
    base = rng.integers(0, 256, (h // 6 + 1, w // 6 + 1, 3)).astype(np.uint8)
    img = np.repeat(np.repeat(base, 6, axis=0), 6, axis=1)[:h, :w].astype(np.int64)
    img[h // 4: 3 * h // 4, w // 3: w // 2] = rng.integers(100, 255, (3 * h // 4 - h // 4, w // 2 - w // 3, 3))
    return np.clip(img + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)


def frames_with_bars():
    """[5][135][240][3] u8 BGR: black, uniform grey, a 4:3 picture pillarboxed into the 16:9 frame, a letterboxed picture, and the
    synthetic frame of tests/test_gpu_detector.py"""
    rng = np.random.default_rng(2)
    pic = synth_frame(np.random.default_rng(7), SRC_H, SRC_W)
    pillar = np.zeros((SRC_H, SRC_W, 3), np.uint8)
    pw = SRC_H * 4 // 3                                                    # 180 of 240 columns
    pillar[:, (SRC_W - pw) // 2: (SRC_W + pw) // 2] = pic[:, :pw]
    letter = np.zeros((SRC_H, SRC_W, 3), np.uint8)
    lh = SRC_W * 9 // 21                                                   # a 21:9 picture: 102 of 135 rows
    letter[(SRC_H - lh) // 2: (SRC_H + lh) // 2] = pic[:lh]
    return np.stack([np.zeros((SRC_H, SRC_W, 3), np.uint8), np.full((SRC_H, SRC_W, 3), 128, np.uint8), pillar, letter,
                     synth_frame(rng, SRC_H, SRC_W)])


FRAME_NAMES = ("black", "grey", "pillarbox", "letterbox", "synthetic")


# ---- oracle-side views of the GPU's own intermediates --------------------------------------------------------------------------
def level_scores(cls_map):
    return odet.sigmoid_f32(np.asarray(cls_map).reshape(-1))


def rpn_candidates(cls_maps, reg_maps):
    """the first half of odet.rpn_proposals: per level the selected scores and decoded boxes, before the empty-box filter"""
    scores_l, boxes_l = [], []
    for lvl, (c, r) in enumerate(zip(cls_maps, reg_maps)):
        h, w, _ = c.shape
        scores = level_scores(c)
        deltas = r.reshape(-1, 4)
        anchors = odet.grid_anchors(h, w, odet.STRIDES[lvl])
        if scores.shape[0] > 1000:
            order = np.argsort(-scores, kind="stable")[:1000]
            scores, deltas, anchors = scores[order], deltas[order], anchors[order]
        scores_l.append(scores)
        boxes_l.append(odet.delta2bbox(anchors, deltas))
    return scores_l, boxes_l


def cut_in_tie(scores, k):
    """True when the k-th largest score has more equal members than the top k take (the cut falls inside a run of equal scores)"""
    s = np.sort(np.asarray(scores))[::-1]
    if len(s) <= k:
        return False
    v = s[k - 1]
    return int((s == v).sum()) > int((s[:k] == v).sum())


def scale_factor(det):
    return np.array([det.nw / SRC_W, det.nh / SRC_H, det.nw / SRC_W, det.nh / SRC_H], f32)
