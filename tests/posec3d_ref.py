"""Twins of the SkeletonAction stage, written apart from the code they check (tests/test_posec3d.py, tests/test_gpu_posec3d.py).

  * `PoseC3DRef`: the network as a torch.nn module of Conv3d / BatchNorm3d / MaxPool3d with the checkpoint's key names, evaluated on
    the CPU in float32 or float64.  torch does the 3D convolutions itself, so this is an independent oracle of the whole mapping of
    models/posec3d.py onto 2D layer programs (views, copies, BatchNorm folding, the two-step average).
  * `sample_frames_loop`, `pipeline_loop`, `heatmaps_loop`: the sampler and the five transforms of the config's test_pipeline, loop by
    loop in plain numpy on the DECODED arrays (all num_clips * clip_len sampled frames, as mmaction's transforms see them), not on the
    distinct frames as the wrapper's vectorised code does.
mmaction2 is not vendored: both are UNPINNED restatements of its published 0.x sources (see posepipeline_amd/wrappers/mmaction.py).
"""
import numpy as np
import torch
from torch import nn


# ---- the network ---------------------------------------------------------------------------------------------------------------------
class ConvModule(nn.Module):
    def __init__(self, cin, cout, kernel, stride=(1, 1, 1), padding=(0, 0, 0), act=True):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, kernel, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm3d(cout)
        self.act = act

    def forward(self, x):
        x = self.bn(self.conv(x))
        return torch.relu(x) if self.act else x


class Bottleneck3d(nn.Module):
    def __init__(self, inplanes, planes, spatial_stride, inflate, first, temporal_stride=1):
        super().__init__()
        self.conv1 = ConvModule(inplanes, planes, (3, 1, 1) if inflate else (1, 1, 1), padding=(1, 0, 0) if inflate else (0, 0, 0))
        self.conv2 = ConvModule(planes, planes, (1, 3, 3), stride=(temporal_stride, spatial_stride, spatial_stride), padding=(0, 1, 1))
        self.conv3 = ConvModule(planes, planes * 4, 1, act=False)
        if first:
            self.downsample = ConvModule(inplanes, planes * 4, 1, stride=(temporal_stride, spatial_stride, spatial_stride), act=False)
        self.first = first

    def forward(self, x):
        out = self.conv3(self.conv2(self.conv1(x)))
        return torch.relu(out + (self.downsample(x) if self.first else x))


class Backbone(nn.Module):
    def __init__(self, spec):
        super().__init__()
        k = spec.conv1_kernel
        self.conv1 = ConvModule(spec.in_channels, spec.base_channels, (1, k, k), padding=(0, k // 2, k // 2))
        self.maxpool = nn.MaxPool3d((1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1))
        inpl = spec.base_channels
        self.n_stages = len(spec.stage_blocks)
        for s, blocks in enumerate(spec.stage_blocks):
            planes = spec.base_channels * 2 ** s
            layer = []
            for b in range(blocks):
                layer.append(Bottleneck3d(inpl, planes, spec.spatial_strides[s] if b == 0 else 1, bool(spec.inflate[s]), b == 0,
                                          spec.temporal_strides[s] if b == 0 else 1))
                inpl = planes * 4
            setattr(self, f"layer{s + 1}", nn.Sequential(*layer))
        self.out_channels = inpl

    def forward(self, x):
        x = self.maxpool(self.conv1(x))
        for s in range(self.n_stages):
            x = getattr(self, f"layer{s + 1}")(x)
        return x


class Head(nn.Module):
    def __init__(self, cin, n):
        super().__init__()
        self.fc_cls = nn.Linear(cin, n)

    def forward(self, x):
        return self.fc_cls(x.mean(dim=(2, 3, 4)))


class PoseC3DRef(nn.Module):
    def __init__(self, spec):
        super().__init__()
        self.backbone = Backbone(spec)
        self.cls_head = Head(self.backbone.out_channels, spec.num_classes)

    def forward(self, x):
        """x [clips][C][T][H][W] -> logits [clips][num_classes]"""
        return self.cls_head(self.backbone(x))


def param_shapes(spec) -> dict:
    """the twin's state_dict shapes without BatchNorm's num_batches_tracked counters, which no inference reads"""
    return {k: tuple(v.shape) for k, v in PoseC3DRef(spec).state_dict().items() if not k.endswith("num_batches_tracked")}


def logits_ref(spec, sd, maps, dtype) -> np.ndarray:
    """maps [clips][T][H][W][c_pad] NHWC float32 (pad channels ignored) -> logits [clips][num_classes] as float64"""
    m = PoseC3DRef(spec)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    m = m.to(dtype).eval()
    x = torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(maps)[..., :spec.in_channels], (0, 4, 1, 2, 3)))).to(dtype)
    with torch.no_grad():
        return m(x).to(torch.float64).numpy()


def average_clips_ref(logits, dtype=np.float64) -> np.ndarray:
    x = np.asarray(logits, dtype)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).mean(axis=0)


# ---- the sampler and the transforms, loop by loop --------------------------------------------------------------------------------------
def sample_frames_loop(total_frames, clip_len, num_clips, seed=255):
    np.random.seed(seed)
    if total_frames < clip_len:
        if total_frames < num_clips:
            start_inds = list(range(num_clips))
        else:
            start_inds = [i * total_frames // num_clips for i in range(num_clips)]
        inds = []
        for i in start_inds:
            for t in range(clip_len):
                inds.append(i + t)
    elif total_frames < 2 * clip_len:
        inds = []
        for _ in range(num_clips):
            pick = np.random.choice(clip_len + 1, total_frames - clip_len, replace=False)
            skipped = 0
            for t in range(clip_len):
                if t in pick:
                    skipped += 1
                inds.append(t + skipped)
    else:
        bids = [i * total_frames // clip_len for i in range(clip_len + 1)]
        inds = []
        for _ in range(num_clips):
            offset = np.random.randint(np.diff(bids))
            for t in range(clip_len):
                inds.append(bids[t] + int(offset[t]))
    return np.array([i % total_frames for i in inds], np.int64)


def pipeline_loop(window, img_shape, frame_inds, size=64, padding=0.25, threshold=10):
    """window [clip_len][K][3] -> (key points float64 [len(frame_inds)][K][2] in crop pixels, scores float32 [len(frame_inds)][K])"""
    window = np.asarray(window)
    kp = np.stack([window[i, :, :2] for i in frame_inds]).astype(np.float32)          # PoseDecode
    score = np.stack([window[i, :, 2] for i in frame_inds]).astype(np.float32)
    h, w = img_shape
    # PoseCompact
    kp[np.isnan(kp)] = 0.0
    xs = [float(v) for v in kp[..., 0].reshape(-1) if v != 0]
    ys = [float(v) for v in kp[..., 1].reshape(-1) if v != 0]
    min_x, max_x = np.float32(min(xs, default=np.inf)), np.float32(max(xs, default=-np.inf))
    min_y, max_y = np.float32(min(ys, default=np.inf)), np.float32(max(ys, default=-np.inf))
    if not (max_x - min_x < threshold or max_y - min_y < threshold):
        centre = (np.float32(max_x + min_x) / np.float32(2), np.float32(max_y + min_y) / np.float32(2))
        half_width = np.float64(np.float32(max_x - min_x) / np.float32(2)) * (1 + padding)
        half_height = np.float64(np.float32(max_y - min_y) / np.float32(2)) * (1 + padding)
        half_height = max(1.0 * half_width, half_height)
        half_width = max(1 / 1.0 * half_height, half_width)
        bx0, bx1 = int(np.float64(centre[0]) - half_width), int(np.float64(centre[0]) + half_width)
        by0, by1 = int(np.float64(centre[1]) - half_height), int(np.float64(centre[1]) + half_height)
        for f in range(kp.shape[0]):
            for j in range(kp.shape[1]):
                if kp[f, j, 0] != 0:
                    kp[f, j, 0] = np.float32(kp[f, j, 0] - np.float32(bx0))
                if kp[f, j, 1] != 0:
                    kp[f, j, 1] = np.float32(kp[f, j, 1] - np.float32(by0))
        h, w = by1 - by0, bx1 - bx0
    # Resize((-1, 64)): the short side becomes 64
    factor = size / min(h, w)
    new_w, new_h = int(w * factor + 0.5), int(h * factor + 0.5)
    sx, sy = np.float32(new_w / w), np.float32(new_h / h)
    out = np.zeros(kp.shape, np.float64)
    left, top = (new_w - size) // 2, (new_h - size) // 2                              # CenterCrop(64)
    for f in range(kp.shape[0]):
        for j in range(kp.shape[1]):
            out[f, j, 0] = np.float64(np.float32(kp[f, j, 0] * sx)) - left
            out[f, j, 1] = np.float64(np.float32(kp[f, j, 1] * sy)) - top
    return out, score


def patch_value(x, y, mu_x, mu_y, score, h, w, sigma=0.6, dtype=np.float64):
    """one element of GeneratePoseTarget.generate_a_heatmap for one key point, evaluated in `dtype` (float64: the reference)"""
    if score < 1e-4:
        return dtype(0)
    st_x, ed_x = max(int(mu_x - 3 * sigma), 0), min(int(mu_x + 3 * sigma) + 1, w)
    st_y, ed_y = max(int(mu_y - 3 * sigma), 0), min(int(mu_y + 3 * sigma) + 1, h)
    if not (st_x <= x < ed_x and st_y <= y < ed_y):
        return dtype(0)
    d = dtype
    return np.exp(-((d(x) - d(mu_x)) ** 2 + (d(y) - d(mu_y)) ** 2) / d(2) / d(sigma) ** 2) * d(score)


def heatmaps_loop(kps, h, w, perm, c_pad, sigma=0.6, dtype=np.float64):
    """kps [n][K][3] -> [2 n][h][w][c_pad] in `dtype`: the plain samples, then the rendering of Flip(flip_ratio 1, left, right)'s key
    points: x -> w - x where x != 0, joints reordered by perm; pad channels zero"""
    kps = np.asarray(kps, np.float64)
    n, K = kps.shape[:2]
    flipped = kps.copy()
    for f in range(n):
        for k in range(K):
            if flipped[f, k, 0] != 0:
                flipped[f, k, 0] = w - flipped[f, k, 0]
    kps = np.concatenate([kps, flipped[:, np.asarray(perm)]])
    n *= 2
    plain = np.zeros((n, K, h, w), dtype)
    for f in range(n):
        for k in range(K):
            mu_x, mu_y, score = kps[f, k]
            if score < 1e-4:
                continue
            for y in range(max(int(mu_y - 3 * sigma), 0), min(int(mu_y + 3 * sigma) + 1, h)):
                for x in range(max(int(mu_x - 3 * sigma), 0), min(int(mu_x + 3 * sigma) + 1, w)):
                    plain[f, k, y, x] = patch_value(x, y, mu_x, mu_y, score, h, w, sigma, dtype)
    out = np.zeros((n, h, w, c_pad), dtype)
    out[..., :K] = np.transpose(plain, (0, 2, 3, 1))
    return out
