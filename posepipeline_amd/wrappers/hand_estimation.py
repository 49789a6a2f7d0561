"""Drop-in for pose_pipeline/wrappers/hand_estimation.py:10-77 `mmpose_HPE`.

Same signature, same table reads (`HandBbox.bboxes`, the video of `key`), same return value: float32 (T, 42, 3) =
[x_px, y_px, score], rows 0-20 from the frame's first (right-hand) box, 21-41 from the second.  The reference runs
mmpose 1.x `inference_topdown` once per frame; here the frames are streamed to the device in batches and both boxes of
every frame of a batch go through ONE fused pp_topdown call (crop / normalise + mirrored copy -> HRNetv2-W18 ->
flip-merge + DARK / DARK-UDP decode).

Built: `HRNet_dark` (rhd2d, DARK) and `HRNet_udp` (onehand10k, UDP), the HRNetv2-W18 256x256 models of
posepipeline_amd/models/hrnetv2.py (an unpinned restatement: the mmpose hand configs are not in the reference tree).
`RTMPoseHand5`, `RTMPoseCOCO` (RTMPose / SimCC) and `freihand` (ResNet-50) are other model families: NotImplementedError.

Checkpoints are looked up under $PIPELINE_3RDPARTY/mmpose/checkpoints/<basename of the URL the reference names>; nothing
is ever fetched.  A missing file raises with the expected path; POSEPIPE_SYNTHETIC_WEIGHTS=1 substitutes seeded parameters.
"""
from __future__ import annotations

import numpy as np

from .. import _lib, ops, weights
from ..models import hrnetv2
from ..program import Net
from ..video import open_video

NUM_JOINTS = 21
# method -> (spec factory, checkpoint under MODEL_DATA_DIR, post_process, blur kernel, shift_heatmap): the test_cfg of
# mmpose's hrnetv2_w18 rhd2d dark (flip_test, post_process='unbiased', shift_heatmap, modulate_kernel 11) and onehand10k
# udp (use_udp, no shift, modulate_kernel 11) configs
_METHODS = {
    "HRNet_dark": (hrnetv2.hrnetv2_w18_256x256, "mmpose/checkpoints/hrnetv2_w18_rhd2d_256x256_dark-4df3a347_20210330.pth",
                   "unbiased", 11, True),
    "HRNet_udp": (hrnetv2.hrnetv2_w18_256x256, "mmpose/checkpoints/hrnetv2_w18_onehand10k_256x256_udp-0d1b515d_20210330.pth",
                  "udp", 11, False),
}
_OTHER_FAMILIES = {"RTMPoseHand5": "RTMPose-m (SimCC)", "RTMPoseCOCO": "RTMPose-m (SimCC)", "freihand": "ResNet-50"}

BATCH = 32       # frames per fused call: 64 hand crops, 128 network samples with the mirrored copies
_cache: dict = {}


def topdown_settings(method):
    """What `HandStage` hands ops.TopDown for `method`.  No device needed."""
    _, _, post, blur, shift = _METHODS[method]
    # flip test with the IDENTITY permutation: the hand datasets define no left / right swap pairs.
    # chan_map: mmpose 1.x hands the model the BGR frame as decoded and converts ONCE (data_preprocessor bgr_to_rgb=True), so
    # tensor channel 0 is R = channel 2 of the BGR frame -- a single swap, not the body wrapper's double swap (wrappers/mmpose.py,
    # whose reference converts to RGB before mmpose 0.x swaps again).  The normalisation table stays ops.normalize_lut
    # (((v / 255) - mean) / std, the 0.x form of the same constants).
    return dict(num_joints=NUM_JOINTS, flip_perm=np.arange(NUM_JOINTS, dtype=np.int32), shift_heatmap=shift, post=post,
                blur_kernel=blur, chan_map=(2, 1, 0))


def boxes_to_tlwh(boxes_xyxy):
    """[..., 4] (x1, y1, x2, y2) -> (x, y, w, h) float64, what pp_topdown takes.  Its `_box2cs` (aspect ratio 1 for the square
    input, padding 1.25, scale in units of 200 px) is mmpose 1.x's `bbox_xyxy2cs(padding=1.25)` + `_fix_aspect_ratio` up to the
    / 200 .. * 200 convention of the 0.x code: the same centre, the same square side in pixels."""
    b = np.asarray(boxes_xyxy, np.float64)
    return np.concatenate([b[..., :2], b[..., 2:4] - b[..., :2]], axis=-1)


class HandStage:
    """The hand network + fused top-down stage for one method, resident on one device.  `run` takes host frames or a device
    pointer to frames that are already resident (as ops.TopDown.run does), so a cascade can call it on the frames its other
    stages read."""

    def __init__(self, method, device=0, max_frames=BATCH, numerics=None, ctx=None):
        if method in _OTHER_FAMILIES:
            raise NotImplementedError(f"hand pose method {method!r} ({_OTHER_FAMILIES[method]}) is not built; "
                                      f"built: {sorted(_METHODS)}")
        if method not in _METHODS:
            # the reference has no else branch: pose_model_cfg is unbound for an unknown method
            raise UnboundLocalError(f"local variable 'pose_model_cfg' referenced before assignment (unknown method {method!r})")
        spec_fn, ckpt, _, _, _ = _METHODS[method]
        self.method, self.spec = method, spec_fn(NUM_JOINTS)
        self.ctx = _lib.Context(device) if ctx is None else ctx
        sd = weights.get_state_dict(ckpt, hrnetv2.hrnetv2_param_shapes(self.spec), seed=1)
        self.max_frames = int(max_frames)
        self.net = Net(self.ctx, hrnetv2.build_hrnetv2_program(self.spec, sd), max_batch=4 * self.max_frames, numerics=numerics)
        self.td = ops.TopDown(self.net, **topdown_settings(method))

    def run(self, frames, boxes_xyxy, frames_dev_shape=None):
        """frames: numpy [F][H][W][3] u8 BGR, or a device pointer (int) with frames_dev_shape = (F, H, W); boxes_xyxy
        [F][2][4].  Returns float32 [F][42][3]: rows 0-20 the first box of the frame, 21-41 the second."""
        boxes = np.asarray(boxes_xyxy, np.float64)
        f = boxes.shape[0]
        assert boxes.shape == (f, 2, 4) and f <= self.max_frames, (boxes.shape, self.max_frames)
        kp, _ = self.td.run(frames, np.repeat(np.arange(f, dtype=np.int32), 2), boxes_to_tlwh(boxes).reshape(2 * f, 4),
                            frames_dev_shape=frames_dev_shape)
        return kp.reshape(f, 2 * NUM_JOINTS, 3)

    def timing(self):
        return self.td.timing()

    def close(self):
        self.td.close()
        self.net.close()


def _model(method, device=0):
    """HandStage for `method`, built once per process (the reference rebuilds per key, :45)."""
    if (method, device) not in _cache:
        _cache[(method, device)] = HandStage(method, device)
    return _cache[(method, device)]


def mmpose_HPE(key, method="RTMPoseHand5"):
    from ..pipeline import HandBbox, Video
    from ..streaming import FrameStreamer

    stage = _model(method)
    bboxes = (HandBbox & key).fetch1("bboxes")
    video = Video.get_robust_reader(key, return_cap=False)
    n = len(bboxes)
    boxes = np.asarray(bboxes, np.float64).reshape(n, -1, 4)
    assert boxes.shape[1] == 2, f"two boxes per frame (HandBbox method 'TopDown'), found {boxes.shape[1]}"
    results = []
    if n:
        cap = open_video(video)
        streamer = FrameStreamer(stage.ctx, cap, min(BATCH, n), max_frames=n)
        try:
            for dev_ptr, m, first in streamer:
                results.append(stage.run(dev_ptr, boxes[first:first + m], frames_dev_shape=(m, streamer.h, streamer.w)))
                streamer.release()
        finally:
            streamer.close()
            cap.release()
    done = sum(len(r) for r in results)
    assert done == n, "video ended before the hand boxes did"       # reference :55-56 asserts every frame decodes
    return np.concatenate(results) if results else np.zeros((0, 2 * NUM_JOINTS, 3), np.float32)
