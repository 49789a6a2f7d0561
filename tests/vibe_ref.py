"""References for the SMPL stage (VIBE), written apart from the library code.

  * numpy float64: the GRU, the encoder's Linear + residual, SPIN's regressor, rot6d -> rotmat, the SMPL body model (smplx `lbs`), the
    54 -> 49 joints, VIBE's projection and the rotation matrix -> axis-angle conversion (`*_np`, `head_np`);
  * torch: the same network as modules and tensor code (`nn.GRU`, `nn.Linear`, a torchvision-style Bottleneck ResNet-50), evaluated in
    float32 (the tolerance's yardstick, dev32) and float64 (cross-check of the numpy code).
The body-model arrays and the index tables are arguments everywhere: nothing here imports posepipeline_amd.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def as_dtype(sd, dtype):
    return {k: np.asarray(v, dtype) for k, v in sd.items()}


# ---- numpy float64 ---------------------------------------------------------------------------------------------------------------------
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def gru_np(x, layers):
    """x [B][T][in]; layers [(W_ih, W_hh, b_ih, b_hh)]; zero initial state -> [B][T][H] of the top layer"""
    x = np.asarray(x, np.float64)
    for w_ih, w_hh, b_ih, b_hh in layers:
        w_ih, w_hh, b_ih, b_hh = (np.asarray(a, np.float64) for a in (w_ih, w_hh, b_ih, b_hh))
        hid = w_hh.shape[1]
        h = np.zeros((x.shape[0], hid))
        out = np.zeros((x.shape[0], x.shape[1], hid))
        for t in range(x.shape[1]):
            gi, gh = x[:, t] @ w_ih.T + b_ih, h @ w_hh.T + b_hh
            r = _sig(gi[:, :hid] + gh[:, :hid])
            z = _sig(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])
            n = np.tanh(gi[:, 2 * hid:] + r * gh[:, 2 * hid:])
            h = (1 - z) * n + z * h
            out[:, t] = h
        x = out
    return x


def rot6d_np(x):
    a = np.asarray(x, np.float64).reshape(-1, 3, 2)
    a1, a2 = a[:, :, 0], a[:, :, 1]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=1, keepdims=True), 1e-12)
    u = a2 - (b1 * a2).sum(1, keepdims=True) * b1
    b2 = u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-12)
    return np.stack([b1, b2, np.cross(b1, b2)], axis=-1)


def regressor_np(y, sd, n_iter=3):
    """y [n][2048] -> (pose6d [n][144], shape [n][10], cam [n][3])"""
    sd = as_dtype(sd, np.float64)
    n = y.shape[0]
    pose, shape, cam = (np.tile(sd[f"regressor.init_{k}"], (n, 1)) for k in ("pose", "shape", "cam"))
    lin = lambda name, v: v @ sd[f"regressor.{name}.weight"].T + sd[f"regressor.{name}.bias"]          # noqa: E731
    for _ in range(n_iter):
        xc = lin("fc2", lin("fc1", np.concatenate([y, pose, shape, cam], axis=1)))
        pose, shape, cam = pose + lin("decpose", xc), shape + lin("decshape", xc), cam + lin("deccam", xc)
    return pose, shape, cam


def smpl_np(body, betas, rotmat, vertex_ids, joint_map):
    """-> (verts [F][V][3], joints49 [F][49][3], posed chain joints [F][24][3])"""
    b = as_dtype(body, np.float64)
    betas, rot = np.asarray(betas, np.float64), np.asarray(rotmat, np.float64).reshape(-1, 24, 3, 3)
    nf, nv = betas.shape[0], b["v_template"].shape[0]
    v_shaped = b["v_template"][None] + np.einsum("vcl,fl->fvc", b["shapedirs"], betas)
    joints = np.einsum("jv,fvc->fjc", b["J_regressor"], v_shaped)
    feat = (rot[:, 1:] - np.eye(3)).reshape(nf, 207)
    v_posed = v_shaped + (feat @ b["posedirs"]).reshape(nf, nv, 3)
    verts = np.zeros((nf, nv, 3))
    chain_t = np.zeros((nf, 24, 3))
    for f in range(nf):
        g = [None] * 24
        a = np.zeros((24, 4, 4))
        for i in range(24):
            local = np.eye(4)
            local[:3, :3] = rot[f, i]
            local[:3, 3] = joints[f, i] - (joints[f, PARENTS[i]] if i else 0)
            g[i] = local if i == 0 else g[PARENTS[i]] @ local
            a[i] = g[i]
            a[i][:3, 3] = g[i][:3, 3] - g[i][:3, :3] @ joints[f, i]
            chain_t[f, i] = g[i][:3, 3]
        t = np.einsum("vj,jrc->vrc", b["weights"], a)
        verts[f] = np.einsum("vrc,vc->vr", t[:, :3, :3], v_posed[f]) + t[:, :3, 3]
    extra = np.einsum("kv,fvc->fkc", b["J_regressor_extra"], verts)
    j54 = np.concatenate([chain_t, verts[:, np.asarray(vertex_ids)], extra], axis=1)
    return verts, j54[:, np.asarray(joint_map)], chain_t


def project_np(joints3d, cam):
    cam = np.asarray(cam, np.float64)
    t = np.stack([cam[:, 1], cam[:, 2], 2 * 5000.0 / (224 * cam[:, 0] + 1e-9)], axis=-1)
    p = np.asarray(joints3d, np.float64) + t[:, None]
    return 5000.0 * p[..., :2] / p[..., 2:] / 112.0


def rotmat_to_aa_np(rotmat):
    """SPIN's rotation_matrix_to_angle_axis: quaternion (torchgeometry's branches, on the transposed matrix, eps 1e-6), then
    2 atan2(+-sin, +-cos) / sin"""
    r = np.asarray(rotmat, np.float64).reshape(-1, 3, 3)
    out = np.zeros((r.shape[0], 3))
    for n, m in enumerate(np.transpose(r, (0, 2, 1))):
        if m[2, 2] < 1e-6:
            if m[0, 0] > m[1, 1]:
                t = 1 + m[0, 0] - m[1, 1] - m[2, 2]
                q = [m[1, 2] - m[2, 1], t, m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]]
            else:
                t = 1 - m[0, 0] + m[1, 1] - m[2, 2]
                q = [m[2, 0] - m[0, 2], m[0, 1] + m[1, 0], t, m[1, 2] + m[2, 1]]
        elif m[0, 0] < -m[1, 1]:
            t = 1 - m[0, 0] - m[1, 1] + m[2, 2]
            q = [m[0, 1] - m[1, 0], m[2, 0] + m[0, 2], m[1, 2] + m[2, 1], t]
        else:
            t = 1 + m[0, 0] + m[1, 1] + m[2, 2]
            q = [t, m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]]
        q = np.array(q) * 0.5 / np.sqrt(t)
        sin_sq = float((q[1:] ** 2).sum())
        s, c = np.sqrt(sin_sq), q[0]
        two_theta = 2 * (np.arctan2(-s, -c) if c < 0 else np.arctan2(s, c))
        k = two_theta / s if sin_sq > 0 else 2.0
        out[n] = np.nan_to_num(q[1:] * k, nan=0.0)
    return out


def rodrigues_np(aa):
    """rotation vectors [n][3] -> matrices [n][3][3] (float64)"""
    aa = np.asarray(aa, np.float64).reshape(-1, 3)
    out = np.zeros((aa.shape[0], 3, 3))
    for n, v in enumerate(aa):
        th = np.linalg.norm(v)
        k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        if th < 1e-12:
            out[n] = np.eye(3) + k
        else:
            out[n] = np.eye(3) + np.sin(th) / th * k + (1 - np.cos(th)) / th ** 2 * (k @ k)
    return out


def body_from_params_np(body, pose6d, shape, cam, vertex_ids, joint_map):
    """steps 4 - 8 on regressor outputs -> the wrapper's raw fields"""
    rot = rot6d_np(pose6d).reshape(-1, 24, 3, 3)
    verts, j49, _ = smpl_np(body, shape, rot, vertex_ids, joint_map)
    return dict(cam=np.asarray(cam, np.float64), pose_aa=rotmat_to_aa_np(rot).reshape(-1, 72), betas=np.asarray(shape, np.float64), verts=verts,
                joints3d=j49, kp2d=project_np(j49, cam), rotmat=rot)


def gru_layers(sd, n_layers=2):
    return [tuple(sd[f"encoder.gru.{n}_l{l}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(n_layers)]


def head_np(features, sd, body, vertex_ids, joint_map, seq=32):
    """features [n][2048] of consecutive present frames -> fields, sequences of `seq` frames with a zero initial state each"""
    features = np.asarray(features, np.float64)
    sd64 = as_dtype(sd, np.float64)
    ys = []
    for s0 in range(0, features.shape[0], seq):
        f = features[s0:s0 + seq]
        h = gru_np(f[None], gru_layers(sd64))[0]
        ys.append(np.maximum(h, 0) @ sd64["encoder.linear.weight"].T + sd64["encoder.linear.bias"] + f)
    pose, shape, cam = regressor_np(np.concatenate(ys), sd64)
    return body_from_params_np(body, pose, shape, cam, vertex_ids, joint_map)


# ---- torch ---------------------------------------------------------------------------------------------------------------------------
class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, down):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(inplanes, planes, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = nn.Conv2d(planes, planes * 4, 1, bias=False), nn.BatchNorm2d(planes * 4)
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4)) if down else None

    def forward(self, x):
        idn = x if self.downsample is None else self.downsample(x)
        y = F.relu(self.bn1(self.conv1(x)))
        y = F.relu(self.bn2(self.conv2(y)))
        return F.relu(self.bn3(self.conv3(y)) + idn)


class Backbone(nn.Module):
    """SPIN's hmr.feature_extractor: ResNet-50 -> AvgPool2d(7, 1) -> [n][2048]"""

    def __init__(self):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
        inpl = 64
        for li, (blocks, planes, stride) in enumerate(((3, 64, 1), (4, 128, 2), (6, 256, 2), (3, 512, 2))):
            layer = []
            for b in range(blocks):
                layer.append(Bottleneck(inpl, planes, stride if b == 0 else 1, b == 0))
                inpl = planes * 4
            setattr(self, f"layer{li + 1}", nn.Sequential(*layer))

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return F.avg_pool2d(x, 7, 1).flatten(1)


def torch_backbone(x_nchw, spin_sd, dtype):
    net = Backbone()
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in spin_sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    net = net.to(dtype).eval()
    with torch.no_grad():
        return net(torch.from_numpy(np.asarray(x_nchw)).to(dtype)).numpy()


class Encoder(nn.Module):
    def __init__(self, inp=2048, hidden=1024, layers=2):
        super().__init__()
        self.gru = nn.GRU(inp, hidden, num_layers=layers)
        self.linear = nn.Linear(hidden, inp)

    def forward(self, x):                      # x [n][2048]: one sequence
        y, _ = self.gru(x[:, None])
        return self.linear(F.relu(y[:, 0])) + x


def torch_gru(x, layers, dtype):
    """x [B][T][in] numpy -> [B][T][H] through nn.GRU"""
    hid, inp = layers[0][1].shape[1], layers[0][0].shape[1]
    g = nn.GRU(inp, hid, num_layers=len(layers), batch_first=True)
    g.load_state_dict({f"{n}_l{l}": torch.from_numpy(np.asarray(a)) for l, lay in enumerate(layers)
                       for n, a in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), lay)})
    g = g.to(dtype).eval()
    with torch.no_grad():
        return g(torch.from_numpy(np.asarray(x)).to(dtype))[0].numpy()


def _t_rot6d(x):
    a = x.reshape(-1, 3, 2)
    a1, a2 = a[:, :, 0], a[:, :, 1]
    b1 = F.normalize(a1)
    b2 = F.normalize(a2 - torch.einsum("bi,bi->b", b1, a2).unsqueeze(-1) * b1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=1)), dim=-1)


def _t_smpl(body, betas, rot, vertex_ids, joint_map):
    nf, nv = betas.shape[0], body["v_template"].shape[0]
    v_shaped = body["v_template"][None] + torch.einsum("bl,mkl->bmk", betas, body["shapedirs"])
    joints = torch.einsum("bik,ji->bjk", v_shaped, body["J_regressor"])
    feat = (rot[:, 1:] - torch.eye(3, dtype=rot.dtype)).reshape(nf, -1)
    v_posed = v_shaped + torch.matmul(feat, body["posedirs"]).reshape(nf, nv, 3)
    rel = joints.clone()
    rel[:, 1:] = joints[:, 1:] - joints[:, PARENTS[1:]]
    mats = torch.cat([torch.cat([rot, rel.unsqueeze(-1)], dim=-1),
                      torch.tensor([0, 0, 0, 1], dtype=rot.dtype).expand(nf, 24, 1, 4)], dim=-2)
    chain = [mats[:, 0]]
    for i in range(1, 24):
        chain.append(torch.matmul(chain[PARENTS[i]], mats[:, i]))
    g = torch.stack(chain, dim=1)
    posed = g[:, :, :3, 3]
    jh = torch.cat([joints, torch.zeros(nf, 24, 1, dtype=rot.dtype)], dim=-1).unsqueeze(-1)
    a = g - F.pad(torch.matmul(g, jh), [3, 0])
    t = torch.matmul(body["weights"], a.reshape(nf, 24, 16)).reshape(nf, nv, 4, 4)
    vh = torch.cat([v_posed, torch.ones(nf, nv, 1, dtype=rot.dtype)], dim=-1)
    verts = torch.matmul(t, vh.unsqueeze(-1))[:, :, :3, 0]
    extra = torch.einsum("bik,ji->bjk", verts, body["J_regressor_extra"])
    j54 = torch.cat([posed, verts[:, torch.as_tensor(np.asarray(vertex_ids), dtype=torch.long)], extra], dim=1)
    return verts, j54[:, torch.as_tensor(np.asarray(joint_map), dtype=torch.long)]


def _t_aa(rot):
    m = rot.reshape(-1, 3, 3).transpose(1, 2)
    d2, d01, d0n1 = m[:, 2, 2] < 1e-6, m[:, 0, 0] > m[:, 1, 1], m[:, 0, 0] < -m[:, 1, 1]
    t0 = 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2]
    q0 = torch.stack([m[:, 1, 2] - m[:, 2, 1], t0, m[:, 0, 1] + m[:, 1, 0], m[:, 2, 0] + m[:, 0, 2]], -1)
    t1 = 1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2]
    q1 = torch.stack([m[:, 2, 0] - m[:, 0, 2], m[:, 0, 1] + m[:, 1, 0], t1, m[:, 1, 2] + m[:, 2, 1]], -1)
    t2 = 1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]
    q2 = torch.stack([m[:, 0, 1] - m[:, 1, 0], m[:, 2, 0] + m[:, 0, 2], m[:, 1, 2] + m[:, 2, 1], t2], -1)
    t3 = 1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    q3 = torch.stack([t3, m[:, 1, 2] - m[:, 2, 1], m[:, 2, 0] - m[:, 0, 2], m[:, 0, 1] - m[:, 1, 0]], -1)
    c0, c1, c2, c3 = (x.to(rot.dtype).unsqueeze(-1) for x in (d2 & d01, d2 & ~d01, ~d2 & d0n1, ~d2 & ~d0n1))
    q = q0 * c0 + q1 * c1 + q2 * c2 + q3 * c3
    q = q / torch.sqrt(t0.unsqueeze(-1) * c0 + t1.unsqueeze(-1) * c1 + t2.unsqueeze(-1) * c2 + t3.unsqueeze(-1) * c3) * 0.5
    sin_sq = (q[:, 1:] ** 2).sum(-1)
    s, c = torch.sqrt(sin_sq), q[:, 0]
    two_theta = 2.0 * torch.where(c < 0, torch.atan2(-s, -c), torch.atan2(s, c))
    k = torch.where(sin_sq > 0, two_theta / s, torch.full_like(s, 2.0))
    aa = q[:, 1:] * k.unsqueeze(-1)
    aa[torch.isnan(aa)] = 0.0
    return aa


def torch_body_from_params(body, pose6d, shape, cam, vertex_ids, joint_map, dtype):
    """steps 4 - 8 in torch at `dtype` (numpy in / numpy out), the twin of body_from_params_np"""
    tb = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in body.items()}
    pose6d, shape, cam = (torch.from_numpy(np.asarray(a)).to(dtype) for a in (pose6d, shape, cam))
    with torch.no_grad():
        rot = _t_rot6d(pose6d).reshape(-1, 24, 3, 3)
        return _torch_fields(tb, rot, shape, cam, vertex_ids, joint_map)


def _torch_fields(tb, rot, shape, cam, vertex_ids, joint_map):
    verts, j49 = _t_smpl(tb, shape, rot, vertex_ids, joint_map)
    t = torch.stack([cam[:, 1], cam[:, 2], 2 * 5000.0 / (224 * cam[:, 0] + 1e-9)], dim=-1)
    p = j49 + t[:, None]
    kp = 5000.0 * (p[..., :2] / p[..., 2:]) / 112.0
    return dict(cam=cam.numpy(), pose_aa=_t_aa(rot).reshape(-1, 72).numpy(), betas=shape.numpy(), verts=verts.numpy(), joints3d=j49.numpy(),
                kp2d=kp.numpy(), rotmat=rot.numpy())


def torch_smpl(body, betas, rotmat, cam, vertex_ids, joint_map, dtype):
    """pp_smpl_forward's twin: rotation matrices in"""
    tb = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in body.items()}
    betas, rot, cam = (torch.from_numpy(np.asarray(a)).to(dtype) for a in (betas, rotmat, cam))
    with torch.no_grad():
        return _torch_fields(tb, rot.reshape(-1, 24, 3, 3), betas, cam, vertex_ids, joint_map)


def torch_head(features, sd, body, vertex_ids, joint_map, dtype, seq=32):
    enc = Encoder()
    enc.load_state_dict({k[len("encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith("encoder.")})
    enc = enc.to(dtype).eval()
    t = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items() if k.startswith("regressor.")}
    x = torch.from_numpy(np.asarray(features)).to(dtype)
    with torch.no_grad():
        y = torch.cat([enc(x[s0:s0 + seq]) for s0 in range(0, x.shape[0], seq)])
        n = y.shape[0]
        pose, shape, cam = (t[f"regressor.init_{k}"].expand(n, -1) for k in ("pose", "shape", "cam"))
        for _ in range(3):
            xc = torch.cat([y, pose, shape, cam], 1)
            xc = F.linear(F.linear(xc, t["regressor.fc1.weight"], t["regressor.fc1.bias"]), t["regressor.fc2.weight"], t["regressor.fc2.bias"])
            pose = pose + F.linear(xc, t["regressor.decpose.weight"], t["regressor.decpose.bias"])
            shape = shape + F.linear(xc, t["regressor.decshape.weight"], t["regressor.decshape.bias"])
            cam = cam + F.linear(xc, t["regressor.deccam.weight"], t["regressor.deccam.bias"])
    return torch_body_from_params(body, pose.numpy(), shape.numpy(), cam.numpy(), vertex_ids, joint_map, dtype)


# ---- the crop (host twin of get_person_dataloader's per-frame work) ---------------------------------------------------------------------
def crop_reference(frames_bgr, bboxes, present, oracle_pre):
    """-> (frame ids, squared boxes [n][4], crops u8 RGB [n][224][224][3], tensors [n][3][224][224] float32) with the oracle's
    getAffineTransform / warpAffine / table (oracle_pre = oracle.preprocess)"""
    ids, boxes, crops = [], [], []
    dst = np.float32([[0, 0], [224, 224], [0, 224]])
    for i, (bb, pr) in enumerate(zip(bboxes, present)):
        if not pr:
            continue
        bb = np.asarray(bb, np.float64)
        center, hw = bb[:2] + bb[2:] / 2.0, bb[2:]
        hw = np.array([hw[1], hw[1]]) if hw[0] / hw[1] < 1.0 else np.array([hw[0], hw[0]])
        sq = np.concatenate([center - hw / 2, hw])
        src = np.float32([[sq[0], sq[1]], [sq[0] + sq[2], sq[1] + sq[3]], [sq[0], sq[1] + sq[3]]])
        m = oracle_pre.get_affine_transform_cv(src, dst)
        crops.append(oracle_pre.warp_affine_u8(np.ascontiguousarray(frames_bgr[i][:, :, ::-1]), m, (224, 224)))
        ids.append(i)
        boxes.append(sq)
    crops = np.stack(crops)
    lut = oracle_pre.normalize_lut(MEAN.astype(np.float32), STD.astype(np.float32))
    x = np.stack([lut[c][crops[..., c]] for c in range(3)], axis=1)
    return np.asarray(ids), np.stack(boxes), crops, x.astype(np.float32)
