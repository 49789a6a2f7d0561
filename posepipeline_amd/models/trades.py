"""TraDeS (TrackingBboxMethodLookup row 4): CenterTrack's DLA-34 with the DCN up-sampling neck, a cost volume between the embeddings
of consecutive frames (CVA) and a deformable warp of the previous frame's features along the resulting offset (MFW), as two layer
programs with one kernel between them.

The network behind pose_pipeline/wrappers/trades.py (upstream `Detector` of TRADES_PATH, which is not vendored): an UNPINNED
restatement of the published model (INTEGRATION.md lists what to check first with a real trades/crowdhuman.pth).

Layers (state-dict keys are upstream's; trunk = models/dla.dla34_trunk, the same layers as FairMOT's):
  base, dla_up, ida_up     DLA-34, DLAUp, IDAUp with 16 DCN layers -> feat, 64 channels at stride 4
  embedconv.{0,2,4}        3x3 64 -> 64 + ReLU, 3x3 64 -> 64 + ReLU, 1x1 64 -> 128, all with bias; then MaxPool2d(2, 2) -> emb'
                           [hp / 8][wp / 8][128]                                                              (program A, batched)
  CVA                      pp_trades_cva(emb'_cur, emb'_prev): row / column maxima of the cost volume, two softmaxes at temperature 5,
                           offsets in units of stride-4 cells (the x 2 is in the templates), nearest x 2 -> tracking_offset
                           [hp / 4][wp / 4][2], channel 0 = w, 1 = h
  pre_hm                   pp_trades_render_prehm of the tracker's boxes, already AvgPool2d(4, 4)-ed: [hp / 4][wp / 4][1]
  conv_offset_w / _h       3x3 65 -> 9 with bias on cat[tracking_offset[0:1] resp. [1:2], feat_cur - feat_prev]          (program B)
  dcn1_1                   DCNv2 3x3 64 -> 64 (bias, no BN, no activation) of pre_hm * feat_prev with offsets channel 2k = dy =
                           off_h9[k], 2k + 1 = dx = off_w9[k] and mask = 1 -> prop
  attention_cur / _prev    3x3 64 -> 1 with bias on feat_cur / prop; a = softmax over the pair; enhanced = a0 feat_cur + a1 prop
  hm 1, reg 2, wh 2, ltrb_amodal 4     3x3 64 -> 256 + ReLU, 1x1 -> c, both with bias, on `enhanced`

Program B in ops: PP_OP_SUB_CAT writes cat[tracking_offset, 0, 0, feat_cur - feat_prev] (68 channels) once; ONE 3x3 convolution 68 -> 27
then produces the offset / mask tensor of PP_OP_DCN3X3 directly: the channel interleave of off_h9 / off_w9 is the order of the rows of
its weight (row 2k = conv_offset_h[k] reading channel 1 and the difference, row 2k + 1 = conv_offset_w[k] reading channel 0 and the
difference), and its rows 18 .. 26 are zero weights with bias MASK_LOGIT = 32: PP_OP_DCN3X3 applies a sigmoid to the mask logit, and
1 / (1 + exp(-32)) evaluated in double and rounded to float32 is exactly 1.0f, which is upstream's mask of ones.  Then PP_OP_BCAST_MUL,
PP_OP_DCN3X3, the two attention convolutions, PP_OP_BLEND2 and the heads: 15 launches per frame.
"""
from __future__ import annotations

import math

import numpy as np

from .. import _lib as L
from ..program import Program, ProgramBuilder
from . import dla

# the reference wrapper's `params` that matter at inference, restated (pose_pipeline/wrappers/trades.py:93-112)
K = 100
OUT_THRESH = NEW_THRESH = PRE_THRESH = TRACK_THRESH = 0.5
DOWN_RATIO = 4
HEAD_CONV = 256
HEADS = (("hm", 1), ("reg", 2), ("wh", 2), ("ltrb_amodal", 4))
EMBED_DIM = 128
TEMPERATURE = 5.0
MEAN = (0.408, 0.447, 0.470)
STD = (0.289, 0.274, 0.278)
CHECKPOINT = "trades/crowdhuman.pth"
HM_BIAS = -21.95          # synthetic weights only (synth_trades_state_dict)
MASK_LOGIT = 32.0          # float32(1 / (1 + exp(-32))) == 1.0f: the unit mask of dcn1_1 through PP_OP_DCN3X3's sigmoid


def input_size(src_h: int, src_w: int):
    """network input (hp, wp): 480 x 864, or 864 x 480 when the source has height > width (:114-121)"""
    return (864, 480) if src_h > src_w else (480, 864)


def trades_param_shapes() -> dict:
    """{upstream state-dict key: shape} of every parameter the inference pass reads"""
    s = dla.dla34_trunk_param_shapes()
    for i, (co, ci, k) in ((0, (64, 64, 3)), (2, (64, 64, 3)), (4, (EMBED_DIM, 64, 1))):
        s[f"embedconv.{i}.weight"] = (co, ci, k, k)
        s[f"embedconv.{i}.bias"] = (co,)
    for name in ("attention_cur", "attention_prev"):
        s[name + ".weight"] = (1, 64, 3, 3)
        s[name + ".bias"] = (1,)
    for name in ("conv_offset_w", "conv_offset_h"):
        s[name + ".weight"] = (9, 65, 3, 3)
        s[name + ".bias"] = (9,)
    s["dcn1_1.weight"] = (64, 64, 3, 3)
    s["dcn1_1.bias"] = (64,)
    for head, c in HEADS:
        s[f"{head}.0.weight"] = (HEAD_CONV, 64, 3, 3)
        s[f"{head}.0.bias"] = (HEAD_CONV,)
        s[f"{head}.2.weight"] = (c, HEAD_CONV, 1, 1)
        s[f"{head}.2.bias"] = (c,)
    return s


def trades_param_count() -> int:
    return int(sum(int(np.prod(v)) for v in trades_param_shapes().values()))


def check_state_dict(sd: dict) -> dict:
    """keys and shapes of a checkpoint dict (`checkpoint["state_dict"]` or the dict itself; a `module.` prefix is dropped) against the
    inventory; returns the float32 dict of the inventory's keys.  KeyError names missing parameters, ValueError a wrong shape.  Keys
    outside the inventory (base.pre_img_layer.*, base.pre_hm_layer.*, base.fc, num_batches_tracked) are ignored, never required."""
    if isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    shapes = trades_param_shapes()
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise KeyError(f"TraDeS checkpoint: missing parameters {missing[:5]}{'...' if len(missing) > 5 else ''}")
    for k, shp in shapes.items():
        if tuple(np.shape(sd[k])) != tuple(shp):
            raise ValueError(f"TraDeS checkpoint: {k} has shape {tuple(np.shape(sd[k]))}, expected {tuple(shp)}")
    return {k: np.asarray(sd[k], np.float32) for k in shapes}


def synth_trades_state_dict(shapes: dict, seed: int) -> dict:
    """Seeded parameters: models/dla.synth_dla34_state_dict (fractional DCN offsets, perturbed bilinear up-sampling, the `hm` head
    amplified and biased), then conv_offset_w / _h scaled so that the warp moves taps by fractions of a cell, a large amodal box
    around every peak (the seeded embeddings of neighbouring cells are almost parallel -- mean cosine 0.99 -- so
    the cost volume's offsets are tens of cells long and carry no motion: only a large box lets CenterTrack's size gates accept a
    match), and the `hm` head re-biased: measured at 480 x 864 on seeded clips, the raw map of this network (before the gain of 100)
    has mean 0.153 and standard deviation 0.010 with one group of outliers, the ~115 cells of the last column at 0.215 .. 0.223;
    logit = 100 raw + HM_BIAS puts 0.5 at raw = 0.2195, which a handful of them pass"""
    sd = dla.synth_dla34_state_dict(shapes, seed)
    for name in ("conv_offset_w", "conv_offset_h"):
        sd[name + ".weight"] = (sd[name + ".weight"] * np.float32(0.25)).astype(np.float32)
    sd["wh.2.bias"] = np.full_like(sd["wh.2.bias"], 6.0)
    sd["ltrb_amodal.2.bias"] = np.array([-100.0, -120.0, 100.0, 120.0], np.float32)
    sd["hm.2.bias"] = np.full_like(sd["hm.2.bias"], HM_BIAS)
    return sd


def get_state_dict(seed: int = 11) -> dict:
    """trades/crowdhuman.pth under MODEL_DATA_DIR, keys and shapes checked; POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded
    parameters when the file is absent.  Nothing is fetched."""
    import os
    from .. import weights
    path = os.path.join(weights.model_data_dir(), CHECKPOINT)
    if os.path.exists(path):
        return check_state_dict(weights.load_state_dict(path))
    return weights.get_state_dict(CHECKPOINT, trades_param_shapes(), seed=seed, synth=synth_trades_state_dict)


# ---- the two programs -----------------------------------------------------------------------------------------------------------------
def build_program_a(sd: dict, hp: int, wp: int) -> Program:
    """input [hp][wp][4] (pp_warp_affine_normalize_each) -> "feat" [hp / 4][wp / 4][64] and "emb" [hp / 8][wp / 8][128]; batched over frames"""
    pb = ProgramBuilder()
    feat = dla.dla34_trunk(pb, sd, hp, wp)
    pb.mark_output(feat, "feat")
    e = pb.conv(feat, sd["embedconv.0.weight"], sd["embedconv.0.bias"], pad=1, relu=L.PP_RELU_LAST, name="embedconv.0")
    e = pb.conv(e, sd["embedconv.2.weight"], sd["embedconv.2.bias"], pad=1, relu=L.PP_RELU_LAST, name="embedconv.2")
    e = pb.conv(e, sd["embedconv.4.weight"], sd["embedconv.4.bias"], name="embedconv.4")
    pb.mark_output(pb.maxpool(e, 2, 2, 0, name="maxpool_stride2"), "emb")
    return pb.build()


def offset_mask_conv(sd: dict):
    """the 68 -> 27 convolution that writes PP_OP_DCN3X3's offset / mask tensor from PP_OP_SUB_CAT's output (module docstring)"""
    ww, wh = sd["conv_offset_w.weight"], sd["conv_offset_h.weight"]
    w = np.zeros((27, 68, 3, 3), np.float32)
    b = np.zeros(27, np.float32)
    w[0:18:2, 1] = wh[:, 0]            # dy = off_h9: the h channel of tracking_offset ...
    w[0:18:2, 4:] = wh[:, 1:]          # ... and the difference
    w[1:18:2, 0] = ww[:, 0]            # dx = off_w9
    w[1:18:2, 4:] = ww[:, 1:]
    b[0:18:2] = sd["conv_offset_h.bias"]
    b[1:18:2] = sd["conv_offset_w.bias"]
    b[18:] = MASK_LOGIT
    return w, b


def build_program_b(sd: dict, h: int, w: int) -> Program:
    """inputs "feat_cur", "feat_prev" [h][w][64], "tracking_offset" [h][w][2], "pre_hm" [h][w][1] -> "enhanced" and the head maps
    "hm", "reg", "wh", "ltrb_amodal"; "diff_cat", "offset_mask", "gated" and "prop" keep buffers of their own too (tests; 0.6 MB at 120 x 216)"""
    pb = ProgramBuilder()
    cur = pb.buf(h, w, 64, name="feat_cur")
    prev = pb.buf(h, w, 64, name="feat_prev")
    trk = pb.buf(h, w, 2, name="tracking_offset")
    pre_hm = pb.buf(h, w, 1, name="pre_hm")
    cat = pb.mark_output(pb.sub_cat(cur, prev, trk, name="diff_cat"), "diff_cat")
    wom, bom = offset_mask_conv(sd)
    om = pb.mark_output(pb.conv(cat, wom, bom, pad=1, name="conv_offset_hw"), "offset_mask")
    gated = pb.mark_output(pb.bcast_mul(prev, pre_hm, name="pre_hm_gate"), "gated")
    prop = pb.mark_output(pb.dcn3x3(gated, om, sd["dcn1_1.weight"], sd["dcn1_1.bias"], name="dcn1_1"), "prop")
    a_cur = pb.conv(cur, sd["attention_cur.weight"], sd["attention_cur.bias"], pad=1, name="attention_cur")
    a_prev = pb.conv(prop, sd["attention_prev.weight"], sd["attention_prev.bias"], pad=1, name="attention_prev")
    enh = pb.mark_output(pb.blend2(cur, prop, a_cur, a_prev, name="attention_blend"), "enhanced")
    for head, c in HEADS:
        t = pb.conv(enh, sd[f"{head}.0.weight"], sd[f"{head}.0.bias"], pad=1, relu=L.PP_RELU_LAST, name=f"{head}.0")
        o = pb.buf(h, w, c, name=head)
        pb.conv(t, sd[f"{head}.2.weight"], sd[f"{head}.2.bias"], out=o, name=f"{head}.2")
    return pb.build()


# ---- host geometry (CenterTrack's utils/image.py, restated) ------------------------------------------------------------------------------
def _third_point(a, b):
    d = a - b
    return b + np.array([-d[1], d[0]], np.float32)


def affine_matrix(src_h: int, src_w: int, out_w: int, out_h: int, inv: bool = False) -> np.ndarray:
    """get_affine_transform(c, s, 0, (out_w, out_h), inv) with pre_process' fix_res centre and scale: c = (w / 2, h / 2), s = max(h, w)
    -> 2 x 3 float64.  Triangles in float32, the third point by rotation, cv2.getAffineTransform = a float64 6 x 6 solve.  inv=False
    maps source pixels to the (out_w, out_h) image, inv=True back."""
    c = np.array([src_w / 2.0, src_h / 2.0], np.float32)
    s = max(src_h, src_w) * 1.0
    scale = np.array([s, s], np.float32)
    src_dir = np.array([0.0, scale[0] * -0.5])
    dst_dir = np.array([0, out_w * -0.5], np.float32)
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0] = c
    src[1] = c + src_dir
    dst[0] = [out_w * 0.5, out_h * 0.5]
    dst[1] = np.array([out_w * 0.5, out_h * 0.5], np.float32) + dst_dir
    src[2] = _third_point(src[0], src[1])
    dst[2] = _third_point(dst[0], dst[1])
    p, q = (dst, src) if inv else (src, dst)
    a = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        a[2 * i, 0:3] = [p[i, 0], p[i, 1], 1.0]
        a[2 * i + 1, 3:6] = [p[i, 0], p[i, 1], 1.0]
        b[2 * i], b[2 * i + 1] = q[i, 0], q[i, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def affine_transform(pt, t) -> np.ndarray:
    """CenterTrack affine_transform: float32 point, float64 matrix -> float64 [2]"""
    return t @ np.array([pt[0], pt[1], 1.0], np.float32).astype(np.float64)


def gaussian_radius(height, width, min_overlap=0.7) -> float:
    a1 = 1
    b1 = height + width
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + np.sqrt(b1 ** 2 - 4 * a1 * c1)) / 2
    a2 = 4
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + np.sqrt(b2 ** 2 - 4 * a2 * c2)) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + np.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def prehm_boxes(boxes_src, trans_input, hp: int, wp: int) -> np.ndarray:
    """CenterTrack `_get_additional_inputs` up to the rendering: source-pixel boxes [m][4] (the tracks with score >= pre_thresh) -> int32
    [m'][3] = (cx, cy, radius) in network-input pixels for pp_trades_render_prehm.  Per box: both corners through the forward matrix
    (float32 results), clipped to the input (`_trans_bbox`); skipped unless height and width are positive; radius = max(0,
    int(gaussian_radius((ceil(h), ceil(w))))); centre = the float32 centre truncated."""
    out = []
    for box in np.asarray(boxes_src, np.float32).reshape(-1, 4):
        b = np.empty(4, np.float32)
        b[:2] = affine_transform(box[:2], trans_input)
        b[2:] = affine_transform(box[2:], trans_input)
        b[[0, 2]] = np.clip(b[[0, 2]], 0, wp - 1)
        b[[1, 3]] = np.clip(b[[1, 3]], 0, hp - 1)
        h, w = b[3] - b[1], b[2] - b[0]
        if h > 0 and w > 0:
            radius = max(0, int(gaussian_radius(math.ceil(h), math.ceil(w))))
            ct = np.array([(b[0] + b[2]) / 2, (b[1] + b[3]) / 2], np.float32).astype(np.int32)
            out.append((int(ct[0]), int(ct[1]), radius))
    return np.array(out, np.int32).reshape(-1, 3)


def post_process(dets, trans_inv, out_thresh=OUT_THRESH):
    """pp_trades_decode's rows [K][9] of one frame (heat-map cells) -> the detections of generic_post_process in source pixels: ct,
    both box corners and ct + tracking go through the inverse matrix, `tracking` is the difference of the transformed points, and the
    list stops at the first score below out_thresh.  float32 values, as upstream stores them."""
    out = []
    for d in np.asarray(dets, np.float32):
        if d[8] < out_thresh:
            break
        ct = affine_transform(d[0:2], trans_inv).astype(np.float32)
        moved = affine_transform(d[0:2] + d[6:8], trans_inv).astype(np.float32)
        bbox = np.r_[affine_transform(d[2:4], trans_inv), affine_transform(d[4:6], trans_inv)].astype(np.float32)
        out.append({"score": float(d[8]), "class": 1, "ct": ct, "tracking": moved - ct, "bbox": bbox})
    return out
