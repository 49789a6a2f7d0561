"""Drop-in for pose_pipeline/wrappers/trades.py:93-155 `trades_bounding_boxes`.

Same signature and the same return structure: one list per decoded frame of
    {"track_id": int, "tlbr": ndarray(4,) x1y1x2y2, "tlhw": ndarray(4,) [x, y, w, h], "confidence": float}
(`parse_result`, :147-155: tlbr is the detection's `bbox`, tlhw = [x1, y1, x2 - x1, y2 - y1] -- the key really is spelled `tlhw` and
holds x, y, w, h --, confidence = `score`, track_id = `tracking_id`).  The reference imports upstream's `Detector` from TRADES_PATH and
calls `detector.run(frame)` once per frame; upstream needs the CUDA-only DCNv2 extension.  Here the clip is streamed to the device
in chunks (streaming.FrameStreamer); pre-processing and program A (DLA-34 trunk, embedding) run batched over a chunk, the cost-volume
association (pp_trades_cva) runs batched over the chunk's frame pairs, and the part that depends on the tracker's state -- the
pre-heat-map, program B (warp, attention blend, heads), the decode and the association (tracking.TradesTracker) -- runs frame by frame.

Reference behaviour kept (TraDeS / CenterTrack are not vendored: everything below is restated and UNPINNED):
  * THE CHANNELS ARE SWAPPED: the wrapper applies cv2.cvtColor(frame, COLOR_RGB2BGR) to what cv2 decoded (BGR), and the detector
    normalises with mean (0.408, 0.447, 0.470) / std (0.289, 0.274, 0.278) in its own BGR order.  The network therefore sees R where its
    statistics expect B.  Kept: tensor channel c = (frame[2 - c] / 255 - mean[c]) / std[c].
  * Network input 864 x 480 (w x h), or 480 x 864 when the source has height > width (:114-121); `fix_res` pre-processing: c = (w / 2,
    h / 2), s = max(h, w), get_affine_transform(c, s, 0, (inp_w, inp_h)), cv2.warpAffine(INTER_LINEAR), border 0
    (pp_warp_affine_normalize_each: one matrix, a LUT and the channel map).
  * Settings: K = 100, out_thresh = new_thresh = pre_thresh = track_thresh = 0.5, down_ratio = 4, clip_len = 2 (one previous frame),
    max_age = -1, hungarian = False, public_det = False, embedding = False, head_conv = 256, head_kernel = 3, heads hm 1 / reg 2 / wh 2
    / ltrb_amodal 4, deform_kernel_size = 3.  The box is ltrb_amodal's, about the integer peak (it overrides `wh`'s).
  * Frame 0's previous frame is itself (upstream initialises pre_images and inference_feats with the current frame) and its
    pre-heat-map is empty; ids start at 1 in every call.

UNPINNED -- check these first with a real trades/crowdhuman.pth at hand: the state-dict key names of the added modules
(embedconv.{0,2,4}, attention_cur, attention_prev, conv_offset_w, conv_offset_h, dcn1_1, the head names); that the x 2 is in the offset
templates; the (w, h) channel order of tracking_offset; which of off_h9 / off_w9 feeds dy and which dx; that temperature 5 multiplies
before the softmax; that base.pre_img_layer.* / base.pre_hm_layer.* may be present and are not read on this path (ignored like
base.fc, never required); AvgPool2d(4) of pre_hm; frame 0's previous features being its own.

Checkpoint: trades/crowdhuman.pth under MODEL_DATA_DIR (`checkpoint["state_dict"]` or the dict itself, a `module.` prefix dropped, keys
and shapes checked); POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded parameters (models/trades.synth_trades_state_dict).
"""
from __future__ import annotations

import time

import numpy as np

from .. import _lib, ops
from ..models import trades as T
from ..program import Net
from ..tracking import TradesTracker
from ..video import open_video

BATCH = 4                              # frames per pass of program A (the arena of the 480 x 864 trunk is 0.2 GB per frame)
CHAN_MAP = (2, 1, 0)                   # see "THE CHANNELS ARE SWAPPED"
_cache: dict = {}
last_timing: dict = {}                 # total wall milliseconds and frames of the most recent call; with STAGE_TIMING also per stage
STAGE_TIMING = False                   # True (tools/trades_timing.py): a stream synchronisation after every stage, so that the stages add up
STAGES = ("pre", "program_a", "cva", "render", "program_b", "decode", "tracker")


def parse_result(result) -> dict:
    """one detection of the tracker's output -> the wrapper's dict (:147-155)"""
    bbox = np.asarray(result["bbox"])
    return {"track_id": int(result["tracking_id"]), "tlbr": bbox,
            "tlhw": np.array([bbox[0], bbox[1], bbox[2] - bbox[0], bbox[3] - bbox[1]]), "confidence": float(result["score"])}


class TradesDetector:
    """pre-processing -> program A -> CVA for chunks of frames, then pre-heat-map -> program B -> decode per frame, for one source size"""

    def __init__(self, ctx, sd, src_h, src_w, max_frames=BATCH, numerics=None):
        self.ctx, self.src = ctx, (int(src_h), int(src_w))
        self.hp, self.wp = T.input_size(src_h, src_w)
        self.h, self.w = self.hp // T.DOWN_RATIO, self.wp // T.DOWN_RATIO
        self.net_a = Net(ctx, T.build_program_a(sd, self.hp, self.wp), max_batch=max_frames, numerics=numerics)
        self.net_b = Net(ctx, T.build_program_b(sd, self.h, self.w), max_batch=1, numerics=numerics)
        self.max_frames = max_frames
        self.trans_input = T.affine_matrix(src_h, src_w, self.wp, self.hp)
        self.trans_inv = T.affine_matrix(src_h, src_w, self.w, self.h, inv=True)
        self.lut = ops.normalize_lut(T.MEAN, T.STD)
        self.feat_bytes = self.h * self.w * 64 * 4
        self.emb_bytes = (self.h // 2) * (self.w // 2) * T.EMBED_DIM * 4
        self.trk_bytes = self.h * self.w * 2 * 4
        # slot 0: the frame before the chunk (the previous chunk's last frame; frame 0: itself); slots 1 .. n: the chunk
        self.feats = ctx.malloc((max_frames + 1) * self.feat_bytes)
        self.embs = ctx.malloc((max_frames + 1) * self.emb_bytes)
        self.trk = ctx.malloc(max_frames * self.trk_bytes)
        self.started = False
        self.ms = dict.fromkeys(STAGES, 0.0)

    def reset(self):
        self.started = False
        self.ms = dict.fromkeys(STAGES, 0.0)

    def close(self):
        if getattr(self.ctx, "handle", None):
            for p in (self.feats, self.embs, self.trk):
                self.ctx.free(p)
        self.net_a.close()
        self.net_b.close()

    def _tick(self, key, t0):
        if not STAGE_TIMING:               # production: no synchronisation of its own; the host work overlaps the queued kernels
            return t0
        self.ctx.synchronize()
        t1 = time.perf_counter()
        self.ms[key] += (t1 - t0) * 1e3
        return t1

    def run_chunk(self, frames_dev, n, tracker):
        """frames_dev: device pointer of n frames [n][src_h][src_w][3] u8 BGR -> per frame the tracker's output list"""
        assert 0 < n <= self.max_frames
        ctx, fb, eb = self.ctx, self.feat_bytes, self.emb_bytes
        t = time.perf_counter()
        ops.warp_affine_normalize_each(ctx, frames_dev, np.arange(n, dtype=np.int32), np.tile(self.trans_input.reshape(1, 6), (n, 1)),
                                       (self.wp, self.hp), self.lut, CHAN_MAP, out_dev=self.net_a.buffer("input")[0],
                                       frames_dev_shape=(n,) + self.src)
        t = self._tick("pre", t)
        self.net_a.run(n)
        ctx.d2d(self.feats + fb, self.net_a.buffer("feat")[0], n * fb)
        ctx.d2d(self.embs + eb, self.net_a.buffer("emb")[0], n * eb)
        if not self.started:                           # frame 0's previous frame is itself
            ctx.d2d(self.feats, self.feats + fb, fb)
            ctx.d2d(self.embs, self.embs + eb, eb)
            self.started = True
        t = self._tick("program_a", t)
        ops.trades_cva_dev(ctx, self.embs + eb, self.embs, n, self.h // 2, self.w // 2, self.trk)
        t = self._tick("cva", t)
        b = self.net_b
        out = []
        for f in range(n):
            boxes = T.prehm_boxes([tr["bbox"] for tr in tracker.tracks if tr["score"] >= T.PRE_THRESH], self.trans_input, self.hp, self.wp)
            ops.trades_render_prehm(ctx, boxes, self.hp, self.wp, out_dev=b.buffer("pre_hm")[0])
            t = self._tick("render", t)
            ctx.d2d(b.buffer("feat_cur")[0], self.feats + (f + 1) * fb, fb)
            ctx.d2d(b.buffer("feat_prev")[0], self.feats + f * fb, fb)
            ctx.d2d(b.buffer("tracking_offset")[0], self.trk + f * self.trk_bytes, self.trk_bytes)
            b.run(1)
            t = self._tick("program_b", t)
            dets, _ = ops.trades_decode(ctx, b.buffer("hm")[0], b.buffer("reg")[0], b.buffer("ltrb_amodal")[0], b.buffer("tracking_offset")[0],
                                        1, self.h, self.w, min(T.K, self.h * self.w))
            results = T.post_process(dets[0], self.trans_inv)
            t = self._tick("decode", t)
            out.append(tracker.step(results))
            t = self._tick("tracker", t)
        ctx.d2d(self.feats, self.feats + n * fb, fb)  # the chunk's last frame is the next chunk's previous frame
        ctx.d2d(self.embs, self.embs + n * eb, eb)  # (stream-ordered: the next chunk's kernels follow these copies)
        return out


def _detector(src_h, src_w, device=0):
    key = (src_h, src_w, device)
    if key not in _cache:
        ctx = _lib.Context(device)
        _cache[key] = (ctx, TradesDetector(ctx, T.get_state_dict(), src_h, src_w))
    return _cache[key]


def trades_bounding_boxes(file_path):
    from ..streaming import FrameStreamer
    cap = open_video(file_path)
    video_length = int(cap.num_frames)
    width, height = int(cap.width), int(cap.height)
    tracks = []
    if video_length <= 0:
        cap.release()
        return tracks
    ctx, det = _detector(height, width)
    det.reset()
    tracker = TradesTracker(new_thresh=T.NEW_THRESH)          # ids from 1 in every call
    t_all = time.perf_counter()
    streamer = FrameStreamer(ctx, cap, min(BATCH, video_length), max_frames=video_length)
    try:
        for dev_ptr, n, _first in streamer:
            per_frame = det.run_chunk(dev_ptr, n, tracker)
            streamer.release()
            tracks.extend([[parse_result(r) for r in frame] for frame in per_frame])
    finally:
        streamer.close()
        cap.release()
    last_timing.clear()
    last_timing.update(det.ms if STAGE_TIMING else {}, total=(time.perf_counter() - t_all) * 1e3, frames=len(tracks))
    return tracks
