#!/usr/bin/env python
"""bench.py -- throughput of the MI355X hot path, one JSON line on rank 0.

Workloads (--workload, named in config.workload):
  cascade (default)  BASELINE.json configs[2]/[3] on one GPU: synthetic 1080p frames -> Faster-RCNN R50-FPN
          detect -> SORT association (host) -> HRNet-W48 384x288 top-down 2D with flip_test + DARK decode ->
          VideoPose3D 243-frame lifting.  A step = one chunk of --chunk frames resident in HBM (u8 BGR).
          The detector runs on every frame; because its weights are seeded-random its boxes are meaningless,
          so the boxes fed to the tracker / 2D stage are replayed synthetic ground truth (+jitter), as
          SURVEY.md 8(d) prescribes.
  c2      BASELINE.json configs[1]: HRNet-W32 256x192 on 64 pre-cropped persons per step (flip_test, decode).
  c5      BASELINE.json configs[4] on one GPU: ViTPose-H 256x192 (bf16 MFMA encoder) on 64 pre-cropped persons per step.
  cascade5  the cascade of the default workload with ViTPose-H as its 2D stage (configs[4]'s full pipeline).
One process per GPU (torchrun); ranks work on independent frame shards (weak scaling, no data-path
collective); weights are broadcast from rank 0 over RCCL.  `value` = frames of all ranks / max-over-ranks
wall time of exactly K steps bracketed by barrier + synchronize.
A plain run sets up, warms up, times the K steps and prints the line.  --full adds everything measured outside the timed
steps: stage and per-kernel-family roofline legs, the exact / integer-exact / certified modes, the PCIe legs, the CPU
baseline with its parity readout and the `secondary` configurations.  --dump-outputs DIR writes what the last timed step
returned (rank 0) as DIR/<name>.npy.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 (v_mfma_f32_32x32x16_bf16: 32 cycles / SIMD, 1024 CUs x SIMDs at 2.4 GHz)
# conv_split.hip: 16-bit MFMA products per float32 term -> fp32-equivalent peak = 2500 / products.  fp16 form (round 5, the default):
# two float16 terms per operand, THREE products (833.3); bf16 form (rounds 2 - 4): three bfloat16 terms, SIX products (416.7)
SPLIT_PRODUCTS = {"split_f16": 3, "split_bf16": 6}
SPLIT_DESC = {3: "split into 2 float16 terms under per-channel / per-sample power-of-two scales, 3 v_mfma_f32_32x32x16_f16 per term",
              6: "split exactly into 3 bf16 planes, 6 v_mfma_f32_32x32x16_bf16 per term"}


def split_products(nets):
    """MFMA products per float32 term of the split form these nets run (they share the process default)"""
    kinds = {getattr(n, "split_kind", "exact") for n in nets} - {"exact"}
    return SPLIT_PRODUCTS[kinds.pop()] if len(kinds) == 1 else (6 if not kinds else max(SPLIT_PRODUCTS[k] for k in kinds))
METRIC = "frames/sec (whole node), detect->2D->3D cascade on 1080p; MPJPE vs reference"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks = GPUs of this node (default: WORLD_SIZE when launched by torchrun, else 1).  N > 1 without a "
                         "torchrun environment re-launches this script under `python -m torch.distributed.run` with N ranks")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="cascade", choices=["cascade", "c2", "c5", "cascade5", "track0", "cascade0", "plumbing"])
    ap.add_argument("--chunk", type=int, default=64, help="cascade: frames per step per GPU (32: -4 %; 128: as 64)")
    ap.add_argument("--persons", type=int, default=1, help="cascade: tracked persons per frame")
    ap.add_argument("--batch", type=int, default=64, help="c2 / c5: person-frames per step per GPU")
    ap.add_argument("--cpu-frames", type=int, default=None, help="frames of the CPU-baseline sample (0 = skip)")
    ap.add_argument("--profile-serial", action="store_true",
                    help="cascade: the run to put under `rocprofv3 --kernel-trace --stats`: every launch on one stream, no detector "
                         "look-ahead, no bit-exact / PCIe / CPU legs -- per-kernel durations are then additive and AverageNs of "
                         "conv_split_* x launches_per_step reproduces roofline.ms_per_step_serial")
    ap.add_argument("--no-secondary", action="store_true",
                    help="cascade: skip the `secondary` block (configs[2] with 4 persons, configs[1], the sharded mode on this rank; "
                         "short runs outside the timed region)")
    ap.add_argument("--light", action="store_true", help=argparse.SUPPRESS)   # no side legs at all (used for the secondary lines)
    ap.add_argument("--mode", default="replicas", choices=["replicas", "shard"],
                    help="N > 1: independent frame shards per rank (default, no data-path collective) or ONE clip sharded over "
                         "the ranks with the detection / 2D all_gathers of posepipeline_amd/parallel.py")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need (outside the timed region): roofline / stage legs, the other numerics "
                         "modes, PCIe legs, CPU baseline and parity readout, the `secondary` configurations")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (rank 0) as DIR/<name>.npy, float32 / float64")
    args = ap.parse_args()
    if args.dump_outputs and (args.workload not in DUMPABLE or args.mode != "replicas"):
        ap.error("--dump-outputs: workloads %s in --mode replicas" % ", ".join(DUMPABLE))
    return args


DUMPABLE = ("cascade", "cascade5", "cascade0", "c2", "c5")
DUMP_LIMIT_BYTES = 64 << 20


def _np_out(a):
    """float32, or float64 where the value has 8-byte elements (int64 indices, float64 coordinates): exact either way"""
    a = np.asarray(a)
    return np.ascontiguousarray(a, np.float64 if a.dtype.itemsize == 8 else np.float32)


def cascade_outputs(res):
    """Cascade.step()'s result as flat arrays: the tracker rows of every frame of the chunk, and the 2D / 3D joints decided /
    emitted in this step, tracks in id order, with (track id, frame) per row in the *_index arrays"""
    out = {"tracks": np.array([(f, *row[:6]) for f, rows in enumerate(res["tracks"]) for row in rows], np.float64).reshape(-1, 7)}
    for key in ("keypoints", "keypoints_3d"):
        tids = sorted(res[key])
        out[key] = _np_out(np.concatenate([res[key][t] for t in tids]) if tids else np.zeros((0, 0, 3), np.float32))
        out[key + "_index"] = np.array([(t, f) for t in tids for f in res[key + "_frames"][t]], np.float64).reshape(-1, 2)
    return out


def dump_outputs(d, arrays):
    arrays = {k: _np_out(v) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench.py --dump-outputs: %d bytes of outputs, more than the %d allowed" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(d, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(d, k + ".npy"), a)


def kernel_source_sha():
    """fingerprint of what decides the conv kernels' memory traffic: their sources and the tile table"""
    import hashlib
    h = hashlib.sha256()
    for rel in ("posepipeline_amd/csrc/conv_igemm.hip", "posepipeline_amd/csrc/conv_igemm_p3.hip", "posepipeline_amd/csrc/conv_split.hip",
                "posepipeline_amd/conv_tuning.txt"):
        try:
            with open(os.path.join(ROOT, rel), "rb") as f:
                h.update(f.read())
        except OSError:
            h.update(b"-")
    return h.hexdigest()[:16]


def pmc_traffic(key):
    """HBM bytes per conv launch from rocprofv3 --pmc passes (FETCH_SIZE / WRITE_SIZE cannot be read from inside the process):
    profiles/pmc_traffic.json, written by tools/profile_round.sh together with the fingerprint of the kernel sources it was
    measured on.  A figure measured on other sources is NOT reported (null + the reason), so the number cannot go stale."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            e = json.load(f)[key]
    except (OSError, KeyError, ValueError):
        return None, "no rocprofv3 --pmc measurement for this workload shape (tools/profile_round.sh)"
    if e.get("kernel_sha") != kernel_source_sha():
        return None, "profiles/pmc_traffic.json was measured on other kernel sources (%s): rerun tools/profile_round.sh" % e.get("kernel_sha")
    return e["traffic_bytes_per_launch"], e.get("source", "")


def algorithmic_bytes_per_op(prog, batch):
    """HBM bytes each conv launch of a program would move if every operand were read / written exactly once: input
    activations + weights + bias + residuals + output, float32 (the figure `traffic` is to be compared with); 0 for other ops"""
    per_op = []
    for op in prog.ops:
        if op.type != 1:      # PP_OP_CONV
            per_op.append(0)
            continue
        elems = lambda b: prog.bufs[b][0] * prog.bufs[b][1] * prog.bufs[b][2]
        act = elems(op.in_) + sum(elems(r) for r in (op.res1, op.res2) if r >= 0)
        out = (prog.bufs[op.out][0] * prog.bufs[op.out][1]) * op.cout
        per_op.append(4 * (batch * (act + out) + op.kh * op.kw * op.cin * op.cout + op.cout))
    return per_op


def algorithmic_bytes(prog, batch):
    return sum(algorithmic_bytes_per_op(prog, batch))


def kernel_families(nets_batches, reps=3):
    """Per kernel family (1 = float32 MFMA kernels, 2 = bf16-split kernel): launches, FLOPs, algorithmic bytes and the summed
    HIP-event durations of ONE pass of the given (net, batch) programs, serial on one stream (pp_net_profile: events around
    every op -- the same per-launch durations rocprofv3 --kernel-trace reports for the serial profile)."""
    fam = {1: dict(launches=0, flops=0.0, bytes=0.0, ms=0.0), 2: dict(launches=0, flops=0.0, bytes=0.0, ms=0.0),
           "products": split_products([n for n, _ in nets_batches]), "classes": {}}
    for net, batch in nets_batches:
        net.profile(batch)
        ms = np.median(np.stack([net.profile(batch) for _ in range(reps)]), axis=0)
        kinds = net.conv_kinds()
        ab = algorithmic_bytes_per_op(net.prog, batch)
        for i, k in enumerate(kinds):
            if k in fam:
                f = fam[int(k)]
                f["launches"] += 1
                f["flops"] += net.prog.op_flops[i] * batch
                f["bytes"] += ab[i]
                f["ms"] += float(ms[i])
            if k == 2:       # the split family by layer form: each form has its own roof (round 6)
                op = net.prog.ops[i]
                name = ("3x3 stride 1 (tap kernels)" if op.kh == 3 and op.stride == 1 else "3x3 stride 2 (strided-patch / tap-gather)" if op.kh == 3 else
                        "7x7 stride-2 stem" if op.kh == 7 and op.stride == 2 else "1x1 / full-cover (product and one-tap kernels; fc6 / fc7)")
                c = fam["classes"].setdefault(name, dict(launches=0, flops=0.0, bytes=0.0, ms=0.0))
                c["launches"] += 1
                c["flops"] += net.prog.op_flops[i] * batch
                c["bytes"] += ab[i]
                c["ms"] += float(ms[i])
    return fam


def roofline_families(fam):
    """roofline object of the dominant kernel family (+ the other family beside it), see kernel_families"""
    products = fam.get("products", 6)
    split_peak = BF16_MFMA_PEAK_TFLOPS / products

    def line(f, peak):
        if not f["launches"] or f["ms"] <= 0:
            return None
        a = f["flops"] / (f["ms"] * 1e-3) / 1e12
        return {"launches_per_step": f["launches"], "achieved": a, "peak": peak, "unit": "TFLOP/s", "frac": a / peak,
                "flops_per_launch": f["flops"] / f["launches"], "avg_launch_ms": f["ms"] / f["launches"],
                "algorithmic_bytes": f["bytes"] / f["launches"], "ms_per_step_serial": f["ms"]}
    split_line, fp32_line = line(fam[2], split_peak), line(fam[1], FP32_MFMA_PEAK_TFLOPS)
    if split_line and fam[2]["ms"] >= fam[1]["ms"]:
        roof = dict(split_line)
        roof.update({"bound": "mfma", "kernel": "conv_split*_kernel (3x3 stride-1 / stride-2 convolutions, 1x1 from 128 channels, fc6: float32 operands "
                                                f"{SPLIT_DESC[products]}, float32 accumulate)",
                     "peak_note": f"2500 TFLOP/s dense 16-bit MFMA / {products} products per float32 term; `achieved` counts float32 "
                                  f"(algorithmic) FLOPs, the matrix cores execute {products}x that in 16-bit products",
                     "products_per_term": products,
                     "executed_bf16_tflops": products * split_line["achieved"], "peak_bf16": BF16_MFMA_PEAK_TFLOPS,
                     "fp32_mfma_kernels": fp32_line})
    else:
        roof = dict(fp32_line or {})
        roof.update({"bound": "mfma", "kernel": "conv_igemm_kernel / conv_p3_kernel (v_mfma_f32_16x16x4_f32)", "split_kernel": split_line})
    # the family by layer form, each priced against BOTH roofs: the 3x3 layers are matrix work, the 1x1 layers move X + residual + Y once
    # per tile and sit at the memory roof -- the family's single `frac` above averages the two
    HBM_PEAK_TBS = 8.0
    classes = []
    for name, c in sorted(fam.get("classes", {}).items(), key=lambda kv: -kv[1]["ms"]):
        if c["ms"] <= 0:
            continue
        tf, tb = c["flops"] / (c["ms"] * 1e-3) / 1e12, c["bytes"] / (c["ms"] * 1e-3) / 1e12
        classes.append({"layers": name, "launches_per_step": c["launches"], "ms_per_step_serial": c["ms"], "tflops": tf, "frac_mfma": tf / split_peak,
                        "algorithmic_tb_per_s": tb, "frac_hbm": tb / HBM_PEAK_TBS, "bound": "mfma" if tf / split_peak >= tb / HBM_PEAK_TBS else "hbm"})
    if classes:
        roof["by_layer_form"] = classes
        roof["by_layer_form_note"] = ("the conv_split* launches of one step by layer form, serial HIP-event times; frac_mfma against 2500 / products "
                                      "TFLOP/s, frac_hbm = algorithmic bytes / time against 8 TB/s (a float4 copy reaches 6.29); `bound` = the larger fraction")
    roof["measurement"] = ("HIP events around every launch of one pass of the step's conv programs, serial on one stream "
                           "(pp_net_profile), median of 3 passes; outside the timed region")
    roof["algorithmic_bytes_note"] = ("per launch: every conv operand (input, weights, bias, residuals) read once and every output "
                                      "written once, float32; `traffic` / this = the re-read factor")
    return roof


DTYPE_NOTE = ("; eligible float32 convolutions are evaluated as 2-term float16 splits (22 significand bits under per-channel / "
              "per-sample power-of-two scales, 3 products per term) on the 16-bit matrix cores with float32 accumulation "
              "(float32-accurate at any input magnitude, not bit-identical: tests/test_gpu_split.py; POSEPIPE_SPLIT_F16=0 = the "
              "exact 3-way bf16 split of rounds 2 - 4)")


def launch_ranks(args, argv):
    """`python bench.py --gpus N` with N > 1 outside torchrun: become the launcher.  One process per GPU, rendezvous on
    127.0.0.1 (the container hostname may not resolve), same argv; never returns."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    sys.stdout.flush()
    os.execv(sys.executable, cmd)


class Dist:
    def __init__(self, gpus=None):
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        if gpus is not None and gpus != self.world:
            raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s) (WORLD_SIZE): the line would misreport n_gpus"
                             % (gpus, self.world))
        self.dist = None
        # POSEPIPE_DIST_BACKEND=gloo: rehearsal of the N > 1 code path on a box with fewer GPUs than ranks (ranks share
        # devices, collectives on CPU tensors); the real runs use RCCL ("nccl"), one rank per GPU
        self.backend = os.environ.get("POSEPIPE_DIST_BACKEND", "nccl")
        if self.world > 1:
            import torch
            import torch.distributed as dist
            if self.backend == "nccl":
                torch.cuda.set_device(self.local_rank)
                dist.init_process_group("nccl", device_id=torch.device("cuda", self.local_rank))
            else:
                self.local_rank %= max(torch.cuda.device_count(), 1)
                dist.init_process_group(self.backend)
            self.dist = dist

    def barrier(self, ctx):
        if self.dist is not None:
            self.dist.barrier()
        ctx.synchronize()

    def bcast_blob(self, blob: np.ndarray) -> np.ndarray:
        """weights: one RCCL broadcast from rank 0; every rank then owns the same resident blob"""
        if self.dist is None:
            return blob
        import torch
        dev = "cuda" if self.backend == "nccl" else "cpu"
        t = torch.from_numpy(blob).to(dev) if self.rank == 0 else torch.empty(blob.size, dtype=torch.float32, device=dev)
        self.dist.broadcast(t, src=0)
        return t.cpu().numpy()

    def bcast_blob_fn(self):
        """weights stay on the device: rank 0's blobs arrive as device tensors and pp_net_create_mem reads them in place"""
        if self.dist is None:
            return None
        import torch
        from posepipeline_amd import parallel
        dev = torch.device("cuda", self.local_rank)
        self.blob_log = []
        return parallel.broadcast_blob_fn(self.dist, dev, backend=self.backend, log=self.blob_log)

    def gather_obj(self, obj):
        """every rank's small Python object on rank 0 (per-rank step times of the N > 1 lines)"""
        if self.dist is None:
            return [obj]
        out = [None] * self.world
        self.dist.all_gather_object(out, obj)
        return out

    def max_time(self, dt):
        if self.dist is None:
            return dt
        import torch
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda" if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(tt, op=self.dist.ReduceOp.MAX)
        return float(tt.item())

    def describe(self):
        """what actually ran: world size as the process group reports it, backend, and every rank's device"""
        me = {"rank": self.rank, "local_rank": self.local_rank, "pid": os.getpid()}
        if self.dist is not None:       # (N = 1 never imports torch: a cold `import torch` costs 1 - 2 minutes on a fresh box)
            try:
                import torch
                if torch.cuda.is_available():
                    me["device"] = "cuda:%d %s" % (self.local_rank, torch.cuda.get_device_name(self.local_rank))
            except Exception:
                pass
        ranks = self.gather_obj(me)
        return {"world_size": self.dist.get_world_size() if self.dist is not None else 1,
                "backend": ("rccl (torch.distributed 'nccl')" if self.backend == "nccl" else self.backend) if self.dist is not None else None,
                "launcher": os.environ.get("TORCHELASTIC_RUN_ID") and "torch.distributed.run", "ranks": ranks}

    def close(self):
        if self.dist is not None:
            self.dist.barrier()
            self.dist.destroy_process_group()


# ---- synthetic 1080p clip ---------------------------------------------------------
def synth_1080p(rng, n_frames, persons, h=1080, w=1920):
    """low-frequency background + textured rectangles on linear trajectories; returns frames (BGR u8) and
    per-frame ground-truth boxes [P][5] (x1, y1, x2, y2, score)."""
    bg = rng.integers(40, 200, (h // 40 + 1, w // 40 + 1, 3)).astype(np.uint8)
    bg = np.repeat(np.repeat(bg, 40, axis=0), 40, axis=1)[:h, :w]
    frames = np.empty((n_frames, h, w, 3), np.uint8)
    people = []
    for p in range(persons):
        bw = int(rng.integers(80, 200))
        bh = int(rng.integers(250, 600))
        # slow enough that the looped chunk is one continuous track for the tracker (frame 31 -> frame 0 keeps IoU > 0.5):
        # a step then is the steady state of a long clip -- B new frames of 2D and B frames of 3D per person -- instead of a
        # track death + birth (with their fills) at every step boundary
        people.append(dict(w=bw, h=bh, x=float(rng.uniform(0, w - bw - 60)), y=float(rng.uniform(0, h - bh)),
                           vx=float(rng.uniform(0.2, 0.6)), tex=rng.integers(0, 256, (bh, bw, 3)).astype(np.uint8)))
    boxes = []
    for t in range(n_frames):
        f = bg.copy()
        row = []
        for q in people:
            x0, y0 = int(q["x"] + q["vx"] * t), int(q["y"])
            f[y0:y0 + q["h"], x0:x0 + q["w"]] = q["tex"]
            row.append([x0, y0, x0 + q["w"], y0 + q["h"], 0.9])
        frames[t] = f
        boxes.append(np.array(row, np.float32))
    return frames, boxes


def run_cascade(args, D):
    if args.profile_serial:
        os.environ["POSEPIPE_NET_LANES"] = "1"
        os.environ["POSEPIPE_OVERLAP_DETECTOR"] = "0"
        if args.cpu_frames is None:
            args.cpu_frames = 0
    from posepipeline_amd import _lib
    from posepipeline_amd.cascade import Cascade
    from posepipeline_amd.models import faster_rcnn as fr, hrnet, synth
    from posepipeline_amd.models import videopose3d as vp3d

    ctx = _lib.Context(D.local_rank)
    det_sd = synth.synth_state_dict(fr.faster_rcnn_param_shapes(), seed=2)
    vit = args.workload == "cascade5"      # configs[4]-style cascade: ViTPose-H (bf16 MFMA) as the 2D stage
    if vit:
        from posepipeline_amd.models import vitpose
        pose_spec = vitpose.vitpose_huge()
        pose_sd = vitpose.synth_params(pose_spec, seed=5)
    else:
        pose_spec = hrnet.hrnet_w48_384x288()
        pose_sd = synth.synth_state_dict(hrnet.hrnet_param_shapes(pose_spec), seed=1)
    # lifting weights: metre-sized max-norm contractions (synth.smooth_lifting_state_dict) -- the lifting stage is 0.03 GFLOP per frame, its
    # weight VALUES do not touch the timed region, and with them the readout's 3D difference is a statement in millimetres (seeded
    # He-normal lifting weights amplify 2D differences ~5x and are not metre-sized: DESIGN.md 2a)
    lift_sd = synth.smooth_lifting_state_dict(vp3d.videopose3d_param_shapes(vp3d.VideoPose3DSpec()), seed=3)
    B, P = args.chunk, args.persons
    # N > 1: every program's blob is rank 0's, delivered by one RCCL broadcast per program as a device tensor that
    # pp_net_create_mem consumes in place (the locally built state dicts only define the program structure)
    cas = Cascade(ctx, det_sd, pose_sd, lift_sd, 1080, 1920, chunk=B, max_persons=P, pose_spec=pose_spec, blob_fn=D.bcast_blob_fn())
    if D.world > 1:
        D.blob_log.clear()
    if args.mode == "shard":
        return run_cascade_sharded(args, D, ctx, cas)
    rng = np.random.default_rng(3000 + D.rank)                     # config index 3, per-rank shard
    frames, gt = synth_1080p(rng, B, P)
    dptr = ctx.malloc(frames.nbytes)
    ctx.h2d(dptr, frames)                                          # the chunk is resident in HBM before timing
    jitter = np.random.default_rng(77 + D.rank)

    def replay_boxes():
        out = []
        for g in gt:
            b = g.copy()
            b[:, :4] += jitter.uniform(-2, 2, (len(b), 4)).astype(np.float32)
            b[:, 4] = jitter.uniform(0.5, 1.0, len(b)).astype(np.float32)
            out.append(b)
        return out

    stage = dict(det_pre=0.0, det_image=0.0, det_rpn=0.0, det_roialign=0.0, det_roihead=0.0, det_final=0.0,
                 pose_pre=0.0, pose_backbone=0.0, pose_decode=0.0)

    def step(accumulate=False, more=False):
        # more: another step follows immediately -> its detector pass (same resident chunk) starts under this step's 2D / 3D
        # stages on the detector's own stream (Cascade overlap_detector).  The last step of every timed / warm-up loop passes
        # more=False, so each loop contains exactly as many detector passes as steps and nothing is carried across its ends.
        res = cas.step(None, frames_dev=(dptr, B), replay=replay_boxes(), prefetch=(None, (dptr, B)) if more else None)
        if accumulate:
            t = cas.det_timing
            for k_, v in zip(("det_pre", "det_image", "det_rpn", "det_roialign", "det_roihead", "det_final"), t.values()):
                stage[k_] += v
            a, b_, c = cas.topdown.timing()
            stage["pose_pre"] += a
            stage["pose_backbone"] += b_
            stage["pose_decode"] += c
        return res

    for i in range(args.warmup):
        res = step(more=i + 1 < args.warmup)
    D.barrier(ctx)
    t0 = time.perf_counter()
    for i in range(args.steps):
        res = step(True, more=i + 1 < args.steps)
    D.barrier(ctx)
    dt_own = time.perf_counter() - t0
    dt = D.max_time(dt_own)
    per_rank = D.gather_obj(dt_own / args.steps * 1e3)
    if D.rank != 0:
        return
    K = args.steps
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, cascade_outputs(res))
    flops_step = B * (cas.detector.flops_per_frame + 2 * P * cas.pose_net.prog.flops)
    out = {
        "metric": METRIC, "value": D.world * B * K / dt, "unit": "frames/s", "n_gpus": D.world, "steps": K,
        "warmup": args.warmup, "ms_per_step": dt / K * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None,
        "dtype": ("f32 (detector, lifting) + bf16 (ViT encoder)" if vit else "f32") +
                 DTYPE_NOTE + "; `bit_exact_mode` = the same step on the float32 MFMA kernels only",
        "data": "synthetic",
        "config": {"workload": ("configs[4]-style cascade on one GPU per rank: 1080p detect (Faster-RCNN R50-FPN) -> SORT -> "
                                "ViTPose-H 256x192 (bf16 MFMA encoder) flip_test + UDP decode -> VideoPose3D 243-frame lifting") if vit else
                               ("configs[3] on one GPU per rank: 1080p detect (Faster-RCNN R50-FPN) -> SORT -> HRNet-W48 "
                                "384x288 flip_test + DARK decode -> VideoPose3D 243-frame lifting"),
                   "frames_per_step_per_gpu": B, "persons_per_frame": P,
                   "gflop_per_frame": flops_step / B / 1e9,
                   "detector_boxes": "detector runs on every frame; downstream boxes are replayed synthetic GT (random-weight detector)",
                   "contract": "`value` is the FLOAT-TOLERANCE mode (every program on the fp16-form kernels: joints within 1e-3 px / mm on "
                               "well-conditioned weights, integer outputs NOT guaranteed on near-tie detector decisions); the modes that hold "
                               "north_star's integer contract are `integer_exact_mode` (detector on the float32 MFMA kernels) and "
                               "`integer_exact_mode.certified_mode` (fast detector + per-frame decision margins + exact re-runs)",
                   "detector_lookahead": getattr(cas, "lookahead", "off"),
                   "host_cores_per_rank": (os.cpu_count() or 1) // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", D.world))),
                   "profile_serial": bool(args.profile_serial)},
    }
    if D.world > 1:
        out["per_rank_ms_per_step"] = per_rank
        # (replicas: no data-path collective at all -- the only cross-rank traffic of the timed region is the barrier)
        out["collectives_in_timed_region"] = {"count": 0, "bytes": 0,
                                               "note": "replicas mode shards FRAMES over ranks with no exchange; --mode shard (one clip over the "
                                                       "ranks) reports collectives / collective_bytes / collective_wait per rank"}
    if not args.full:
        return out
    # stage times: inside the timed region the next chunk's detector pass runs UNDER this chunk's 2D stage, so per-stage event
    # times overlap and sum to more than the step; the breakdown reported is from three extra steps without that overlap
    overlapped = {k: v / K for k, v in stage.items()}
    for k_ in stage:
        stage[k_] = 0.0
    step()
    for _ in range(3):
        step(True)
    stage = {k: v / 3 for k, v in stage.items()}
    conv_ms = stage["det_image"] + stage["det_roihead"] + stage["pose_backbone"]
    # serial leg (outside the timed region): the same step with every launch on one stream, so that the per-kernel
    # durations rocprofv3 reports are additive and comparable (POSEPIPE_NET_LANES=1 profile under profiles/)
    nets = (cas.detector.net_a, cas.detector.net_b, cas.pose_net, cas.lift_net)
    for nt in nets:
        nt.set_lanes(False)
    step()
    serial = dict.fromkeys(stage, 0.0)
    saved, stage = stage, serial
    for _ in range(2):
        step(True)
    stage = saved
    serial_conv_ms = (serial["det_image"] + serial["det_roihead"] + serial["pose_backbone"]) / 2
    for nt in nets:
        nt.set_lanes(True)
    n_launch = len(cas.detector.prog_a.ops) + len(cas.detector.prog_b.ops) + len(cas.pose_net.prog.ops)
    if vit:
        # the fp32 conv roofline covers the detector programs only; the ViT stage is reported beside it (its own roofline
        # line is --workload c5)
        pose_flops = B * 2 * P * cas.pose_net.prog.flops
        conv_ms -= stage["pose_backbone"]
        serial_conv_ms -= serial["pose_backbone"] / 2
        n_launch -= len(cas.pose_net.prog.ops)
        flops_conv = flops_step - pose_flops
    else:
        flops_conv = flops_step
    achieved = flops_conv / (conv_ms * 1e-3) / 1e12
    traffic, traffic_note = pmc_traffic("cascade_chunk%d_persons%d" % (B, P))
    # per kernel family, measured live (outside the timed region) with HIP events around every launch of one pass of the conv
    # programs at the step's batch sizes, on one stream
    progs = [(cas.detector.net_a, B), (cas.detector.net_b, B * cas.detector.MAX_ROIS)] + ([] if vit else [(cas.pose_net, 2 * B * P)])
    fam = kernel_families(progs)
    programs = {"achieved": achieved, "launches_per_step": n_launch, "avg_launch_ms": conv_ms / n_launch,
                "note": "all conv programs of a step (4 HIP streams per program, no detector look-ahead): FLOPs / wall time of the programs",
                "serial": {"avg_launch_ms": serial_conv_ms / n_launch, "achieved": flops_conv / (serial_conv_ms * 1e-3) / 1e12,
                           "note": "same step, one stream (pp_net_set_lanes 0): comparable with rocprofv3 --stats AverageNs "
                                   "of profiles/*_serial_kernel_stats.csv"}}
    roof = roofline_families(fam)
    roof.update({"traffic": traffic, "traffic_source": traffic_note, "stage_ms": stage,
                 "stage_ms_note": "per-stage HIP-event times of steps run WITHOUT the detector look-ahead (outside the timed region); in the "
                                  "timed region chunk k + 1's detector pass overlaps chunk k's 2D stage: step = %.1f ms against the %.1f ms "
                                  "these stages sum to" % (dt / K * 1e3, sum(stage.values())),
                 "stage_ms_overlapped": overlapped, "conv_programs": programs})
    # the same workload on the bit-exact float32-MFMA kernels only: a second cascade whose programs are CREATED exact (a net's
    # numerics are fixed at creation, ABI 7); reported beside `value` (N = 1 leg)
    exact_mode = integer_mode = None
    cas_exact = cas_int = None
    side_legs = D.world == 1 and not args.profile_serial and not args.light
    if side_legs:
        cas_exact = Cascade(ctx, det_sd, pose_sd, lift_sd, 1080, 1920, chunk=B, max_persons=P, pose_spec=pose_spec, numerics="exact")

        def step_exact(more=False):
            return cas_exact.step(None, frames_dev=(dptr, B), replay=replay_boxes(), prefetch=(None, (dptr, B)) if more else None)
        step_exact()
        ctx.synchronize()
        t0 = time.perf_counter()
        n_exact = max(2, K // 2)
        for i in range(n_exact):
            step_exact(more=i + 1 < n_exact)
        ctx.synchronize()
        dt_exact = time.perf_counter() - t0
        exact_mode = {"value": B * n_exact / dt_exact, "unit": "frames/s", "steps": n_exact,
                      "note": "the same cascade with its programs created PP_NET_NUMERICS_EXACT (POSEPIPE_CONV_EXACT=1): every "
                              "convolution on v_mfma_f32_16x16x4_f32, results bit-identical to oracle/conv_ref.c"}
        # ... and the integer-exact configuration (round 5): the DETECTOR's programs exact -- which boxes exist, their order, hence
        # track ids / bbox indices / `present` are the oracle's by construction -- the pose and lifting programs on the fast kernels
        cas_int = Cascade(ctx, det_sd, pose_sd, lift_sd, 1080, 1920, chunk=B, max_persons=P, pose_spec=pose_spec, numerics="split", id_numerics="exact")

        def step_int(more=False):
            return cas_int.step(None, frames_dev=(dptr, B), replay=replay_boxes(), prefetch=(None, (dptr, B)) if more else None)
        step_int()
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(n_exact):
            step_int(more=i + 1 < n_exact)
        ctx.synchronize()
        integer_mode = {"value": B * n_exact / (time.perf_counter() - t0), "unit": "frames/s", "steps": n_exact,
                        "note": "Cascade(numerics='split', id_numerics='exact'): detector (RPN / RoI head) on the float32 MFMA kernels, "
                                "HRNet / VideoPose3D on the fp16-form kernels -- integer outputs identical to the exact cascade's on "
                                "every frame (tests/test_gpu_parity_modes.py::test_integer_contract_1080p_64_frames_no_replay), joints "
                                "within 1e-3 px / mm",
                        "ids_no_replay": ids_no_replay({"bit_exact_mode": cas_exact, "integer_exact_mode": cas_int, "default": cas}, dptr, B)}
        if P <= 4:     # (at 8 persons per frame the three cascades above hold the device's memory: their arenas are sized for 1024 pose samples)
            # ... and the CERTIFIED configuration (round 6): the fast detector reports, per frame, how far its closest integer decision is from
            # flipping (pp_detector_enable_margins); frames within the split kernels' error bound are re-run on the float32-MFMA detector.  No
            # replay in this leg's id check; the timed steps replay boxes downstream like every other leg (the detector work is what differs).
            cas_cert = Cascade(ctx, det_sd, pose_sd, lift_sd, 1080, 1920, chunk=B, max_persons=P, pose_spec=pose_spec, numerics="split", id_numerics="certified",
                               overlap_detector=False)
            cert_ids = ids_no_replay({"bit_exact_mode": cas_exact, "certified_mode": cas_cert}, dptr, B)
            probe = dict(cas_cert.certify_stats)
            cas_cert.step(None, frames_dev=(dptr, B), replay=replay_boxes())
            ctx.synchronize()
            t0 = time.perf_counter()
            for i in range(n_exact):
                cas_cert.step(None, frames_dev=(dptr, B), replay=replay_boxes())
            ctx.synchronize()
            integer_mode["certified_mode"] = {
                "value": B * n_exact / (time.perf_counter() - t0), "unit": "frames/s", "steps": n_exact,
                    "frames_certified": probe["certified"], "frames": probe["frames"] - probe["exact_only_frames"],
                "ids_no_replay": cert_ids.get("certified_mode"),
                "thresholds": cas_cert.certify_eps,
                "note": "Cascade(numerics='split', id_numerics='certified'): `frames_certified` of `frames` cleared every decision margin of the fast "
                        "detector pass (pp_detector_margins; thresholds = 4x the measured split-vs-exact deviation per quantity); the others were run "
                        "again on the float32-MFMA detector.  While fewer than half of a chunk certify, the policy runs the exact detector alone "
                        "(then this figure is the integer-exact mode's).  A detection path takes ~10^4 threshold decisions per frame (top-1000 of "
                        "130 560 anchors per level, ~10^5 NMS pairs): with seeded-random weights the closest one sits within the float32 noise of "
                        "ANY non-bit-identical evaluation in nearly every frame -- the margins say so per frame instead of leaving it to chance"}
            cas_cert.release()
    split_peak_line = BF16_MFMA_PEAK_TFLOPS / fam.get("products", 6)
    out.update({"roofline": roof, "bit_exact_mode": exact_mode, "integer_exact_mode": integer_mode if side_legs else None})
    if D.world > 1:
        out["per_rank_roofline_frac"] = [flops_step / (ms * 1e-3) / 1e12 / split_peak_line for ms in per_rank]
    if side_legs:
        # PCIe-inclusive leg (reported beside `value`, never as it): the same chunks streamed from host memory through
        # page-locked staging buffers and the copy stream (posepipeline_amd/streaming.py), upload overlapped with compute
        from posepipeline_amd.video import ArrayVideo
        n_chunks = 6
        host_clip = ArrayVideo(np.concatenate([frames] * n_chunks))
        cas.reset()
        rb = replay_boxes()
        # the staging buffers are page-locked before the clock starts (start-up), then the WHOLE clip is timed: every chunk's
        # read, upload, detector pass and 2D / 3D stages lie inside the window (with the detector pass of chunk k + 1 running
        # under chunk k's 2D stage a window that opened after the first chunk would hold one detector pass too few); the
        # clock stops when the last chunk's results are on the host (flush included), before the staging buffers are freed
        from posepipeline_amd.streaming import FrameStreamer
        streamer = FrameStreamer(ctx, host_clip, B)
        n_seen = 0
        t1 = time.perf_counter()
        for o in cas.run_video(host_clip, replay_fn=lambda first, n: rb[:n], streamer=streamer):
            n_seen += len(o["tracks"])
            t_last = time.perf_counter()
        dt_stream = t_last - t1
        out["pcie_inclusive"] = {"value": n_seen / dt_stream, "unit": "frames/s",
                                 "note": "%d frames read once from host memory, copied into page-locked staging buffers by a "
                                         "reader thread and uploaded on a copy stream while the previous chunks compute "
                                         "(posepipeline_amd/streaming.py); whole clip timed, first (unoverlapped) upload and "
                                         "final flush included" % n_seen}
        # the same clip as an NV12 source (a decoder's native output, half the bytes): NV12 planes through the staging buffers and
        # over PCIe, converted to BGR on the copy stream behind the transfer (csrc/nv12.hip)
        from posepipeline_amd.video import Nv12Video, bgr_to_nv12
        nv_clip = Nv12Video(np.concatenate([bgr_to_nv12(frames)] * n_chunks), frames.shape[1], frames.shape[2])
        cas.reset()
        streamer = FrameStreamer(ctx, nv_clip, B)
        n_seen = 0
        t1 = time.perf_counter()
        for o in cas.run_video(nv_clip, replay_fn=lambda first, n: rb[:n], streamer=streamer):
            n_seen += len(o["tracks"])
            t_last = time.perf_counter()
        out["pcie_inclusive"]["nv12_source"] = {"value": n_seen / (t_last - t1), "unit": "frames/s",
                                                "note": "same clip delivered as NV12 planes (3.1 MB per frame instead of 6.2): "
                                                        "pp_upload_begin_nv12 uploads them and converts on the copy stream"}
    if vit:
        out["roofline"]["vit_stage"] = {"backbone_ms": stage["pose_backbone"], "program_tflops": pose_flops / (stage["pose_backbone"] * 1e-3) / 1e12,
                                        "note": "ViTPose-H program (bf16 GEMMs + fp32 patch embedding / head); roofline line: --workload c5"}
    n_cpu = 8 if args.cpu_frames is None else args.cpu_frames
    if n_cpu > 0 and side_legs and not vit:             # the CPU baseline is a rank-0, N=1 leg (c5 carries the ViT one)
        out["cpu_baseline"] = cpu_baseline_cascade(det_sd, pose_sd, lift_sd, frames, gt, n_cpu,
                                                   {"bit_exact_mode": cas_exact, "integer_exact_mode": cas_int, "default": cas})
    # (the `secondary` block -- the other configurations, one process each -- is added by main() once this function has returned
    # and the cascades above are released)
    out["_wants_secondary"] = bool(side_legs and not vit and not args.no_secondary and args.mode == "replicas")
    return out


def secondary_lines(args):
    """The other single-GPU configurations, measured right after the headline (outside its timed region; a few short steps each), so
    that the driver's record holds them as measurements and not only the builder's profiles/: configs[2] (4 tracked persons per
    1080p frame), configs[1] (HRNet-W32 256x192, pre-cropped), the one-clip-sharded-over-ranks mode on this rank, configs[4]
    (ViTPose-H, with its own CPU baseline) and the cascade with the reference recipes' default tracker (tracking_method 0).
    Every leg is its OWN PROCESS with a timeout (round 5): a HIP abort, an out-of-memory kill or a hang in a side leg
    cannot take the headline measurement -- already taken, printed by main() after this returns -- down with it."""
    import subprocess
    legs = (("cascade_persons4", "configs[2]: the cascade with 4 tracked persons per 1080p frame", ["--persons", "4", "--steps", "4", "--warmup", "1", "--cpu-frames", "0"]),
            ("c2", "configs[1]: HRNet-W32 256x192, 64 pre-cropped person-frames per step", ["--workload", "c2", "--steps", "20", "--warmup", "3", "--cpu-frames", "0"]),
            ("shard_1rank", "configs[3] in --mode shard (one clip sharded over ranks, parallel.py) on this rank",
             ["--mode", "shard", "--steps", "4", "--warmup", "1", "--cpu-frames", "0"]),
            ("c5", "configs[4]: ViTPose-H 256x192 (bf16 MFMA encoder), 64 pre-cropped person-frames per step, flip test + UDP decode",
             ["--workload", "c5", "--steps", "10", "--warmup", "2", "--cpu-frames", "1"]),
            ("cascade0", "the cascade with the reference recipes' default tracker (tracking_method 0: YOLOv4 416 + mars-small128 + DeepSORT)",
             ["--workload", "cascade0", "--steps", "4", "--warmup", "1", "--cpu-frames", "0"]))
    sec, t_all = {}, time.perf_counter()
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    for key, what, over in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--full", "--light", "--no-secondary", "--chunk", str(args.chunk)] + over
        t0 = time.perf_counter()
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                raise RuntimeError("exit code %d: %s" % (p.returncode, (p.stderr or p.stdout)[-300:]))
            r = json.loads(lines[-1])
        except Exception as e:       # a secondary leg never takes the headline line down with it
            sec[key] = {"what": what, "error": "%s: %s" % (type(e).__name__, str(e)[-400:]), "leg_wall_s": time.perf_counter() - t0}
            continue
        roof = r.get("roofline", {})
        sec[key] = {"what": what, "value": r["value"], "unit": r["unit"], "ms_per_step": r["ms_per_step"], "steps": r["steps"],
                    "warmup": r["warmup"], "frames_per_step": r["config"].get("frames_per_step_per_gpu"),
                    "persons_per_frame": r["config"].get("persons_per_frame"),
                    "roofline": {k: roof.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_ms", "launches_per_step",
                                                          "products_per_term")
                                 if roof.get(k) is not None},
                    "fp32_mfma_kernels": {k: (roof.get("fp32_mfma_kernels") or {}).get(k) for k in ("achieved", "peak", "frac", "ms_per_step_serial")
                                          } if roof.get("fp32_mfma_kernels") else None,
                    "leg_wall_s": time.perf_counter() - t0}
        if r.get("cpu_baseline"):
            sec[key]["cpu_baseline"] = {k: r["cpu_baseline"].get(k) for k in ("value", "unit", "cores", "kind", "sample") if k in r["cpu_baseline"]}
    sec["wall_s"] = time.perf_counter() - t_all
    sec["note"] = ("measured after the headline's timed region on the same GPU, one process per leg (timeout 240 s); command lines: "
                   "--persons 4 / --workload c2 / --mode shard / --workload c5 --cpu-frames 1 / --workload cascade0")
    return sec


def run_cascade_sharded(args, D, ctx, cas):
    """--mode shard: ONE clip of world x steps x chunk frames, frames sharded contiguously over the ranks
    (posepipeline_amd/parallel.py): local detection -> all_gather of detection slabs -> identical association on every rank
    -> 2D on the own shard -> all_gather of the 2D rows -> lifting.  A step = one chunk per rank; the timed region is the
    whole sharded run over `steps` chunks per rank (after a run over `warmup` chunks)."""
    from posepipeline_amd import parallel
    B, P, K = args.chunk, args.persons, args.steps
    rng = np.random.default_rng(3000 + D.rank)
    frames, gt = synth_1080p(rng, B, P)
    dptr = ctx.malloc(frames.nbytes)
    ctx.h2d(dptr, frames)                                          # the rank's frames are resident in HBM before timing
    rb = [np.concatenate([g[:, :4], np.full((len(g), 1), 0.9, np.float32)], axis=1) for g in gt]
    stages = parallel.cascade_stages(cas, lambda first, n: rb[:n])

    class _Local:      # world_size 1: the torch.distributed calls parallel.py uses
        numpy_only = True      # parallel._Gather keeps the slab on the host: no torch import in a one-rank run
        def get_rank(self): return 0
        def get_world_size(self): return 1
        def all_gather(self, outs, t): outs[0].copy_(t)

    dist = D.dist if D.dist is not None else _Local()
    dev = "cpu" if D.dist is None or D.backend != "nccl" else "cuda"

    def run(chunks_per_rank, tm=None):
        n = D.world * chunks_per_rank * B
        lo = parallel.shard_bounds(n, D.world)[D.rank]
        return parallel.process_video_sharded(dist, n, lambda lo_, hi_: [(lo + i * B, B, dptr) for i in range(chunks_per_rank)],
                                              *stages, src_hw=(1080, 1920), device=dev, max_persons=P, timings=tm)

    if args.warmup > 0:
        run(args.warmup)
    D.barrier(ctx)
    tm = {}
    t0 = time.perf_counter()
    res = run(K, tm)
    D.barrier(ctx)
    dt_own = time.perf_counter() - t0
    dt = D.max_time(dt_own)
    flops_step = B * (cas.detector.flops_per_frame + 2 * P * cas.pose_net.prog.flops)
    peak = BF16_MFMA_PEAK_TFLOPS / split_products([cas.pose_net])
    mine = {k: (int(v) if k in ("rounds", "collectives", "collective_bytes") else round(v * 1e3, 3)) for k, v in tm.items()}
    # what makes the first real multi-GPU run readable in one shot: every rank's own end-to-end rate against the kernel peak, its
    # collective volume and the part of it that was exposed
    mine["roofline_frac"] = flops_step * K / dt_own / 1e12 / peak
    mine["collective_ms_per_round"] = mine.get("collective_wait", 0.0) / max(1, mine.get("rounds", 1))
    per_rank = D.gather_obj(mine)
    if D.rank != 0:
        return
    return {
        "metric": METRIC, "value": D.world * B * K / dt, "unit": "frames/s", "n_gpus": D.world, "steps": K, "warmup": args.warmup,
        "ms_per_step": dt / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32" + DTYPE_NOTE, "data": "synthetic",
        "config": {"workload": "configs[3]: ONE 1080p clip of %d frames sharded over %d rank(s): detect (Faster-RCNN R50-FPN) -> all_gather of "
                               "detection slabs -> SORT on every rank -> HRNet-W48 384x288 flip_test + DARK decode on the own shard -> "
                               "all_gather of 2D rows -> VideoPose3D 243-frame lifting" % (D.world * B * K, D.world),
                   "mode": "shard", "frames_per_step_per_gpu": B, "persons_per_frame": P, "gflop_per_frame": flops_step / B / 1e9,
                   "tracks": len(res["keypoints_3d"]),
                   "detector_boxes": "detector runs on every frame; downstream boxes are replayed synthetic GT (random-weight detector)"},
        "roofline": {"bound": "mfma", "kernel": "conv_split_kernel (+ the float32 MFMA kernels on the layers it does not take), whole step",
                     "achieved": flops_step * K / dt / 1e12,
                     "peak": peak, "unit": "TFLOP/s", "frac": flops_step * K / dt / 1e12 / peak,
                     "traffic": None, "peak_note": "2500 TFLOP/s dense 16-bit MFMA / %d products per float32 term" % split_products([cas.pose_net]),
                     "note": "END-TO-END float32-equivalent conv FLOP rate per GPU over the whole sharded run (host phases and collectives "
                             "included) against the split kernel's peak; the per-kernel roofline line is the default mode's"},
        "host_cores_per_rank": (os.cpu_count() or 1) // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", D.world))),
        "per_rank_phase_ms": per_rank,
        "per_rank_note": "per rank: phase wall times (ms), roofline_frac = the rank's own end-to-end conv FLOP rate / kernel peak, collectives / "
                         "collective_bytes (received, summed over the run), collective_wait = ms blocked in collectives (the rest overlapped compute)",
    }


def _lib_check(rc):
    if rc != 0:
        raise RuntimeError("libposepipe_hip call failed: %d" % rc)


def ids_no_replay(cascades, dptr, B):
    """One chunk through every cascade WITHOUT replay (detector boxes -> tracker -> followed persons): per mode, the frames whose
    track-id list / tracked rows differ from the bit-exact cascade's (whose detections equal the oracle's bit for bit)."""
    runs = {}
    for mode, cas in cascades.items():
        if cas is None:
            continue
        cas.reset()
        o = cas.step(None, frames_dev=(dptr, B))
        cas.flush()
        cas.reset()
        runs[mode] = o["tracks"]
    ref = runs.get("bit_exact_mode")
    out = {"frames": B, "tracked_boxes_per_frame": [min(len(t) for t in ref), max(len(t) for t in ref)] if ref else None}
    for mode, tr in runs.items():
        if mode == "bit_exact_mode" or ref is None:
            continue
        out[mode] = {"id_mismatches": sum([r[0] for r in a] != [r[0] for r in b] for a, b in zip(tr, ref)),
                     "frames_with_different_rows": sum(not (len(a) == len(b) and np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32)))
                                                       for a, b in zip(tr, ref))}
    out["note"] = ("no replay: the detector's own boxes feed the tracker; `id_mismatches` = frames whose track-id list differs from the "
                   "bit-exact cascade's.  Seeded-random detector weights put ~5000 proposal scores per frame on near-ties, which flip under "
                   "any float32 reordering: the all-split default is held to the margin-aware set relation, the integer-exact mode to 0")
    return out


def cpu_baseline_cascade(det_sd, pose_sd, lift_sd, frames, gt, n_frames, cascades, timed_frames=2):
    """CPU restatement of the reference wrapper path (oracle/) per 1080p frame: detector, then the top-down stage on the
    frame's (replayed) person box, then one 243-frame lifting window -- the per-frame bodies of wrappers/mmtrack.py:37-60,
    wrappers/mmpose.py:60-76 and wrappers/videopose3d.py:77-85.  The first `timed_frames` frames are the timed sample; all
    `n_frames` (spread over the chunk) go through the GPU path as well -- the detector's own boxes, NOT replayed -- once per
    numerics mode (cascades: {"bit_exact_mode": a cascade created exact, "default": the timed one}) for the parity readout."""
    from oracle import clib
    from oracle import decode as odec
    from oracle import detector as odet
    from oracle import nets as onets
    from oracle import preprocess as opre
    from posepipeline_amd.models import hrnet
    from posepipeline_amd.wrappers.videopose3d import lift, normalize_screen_coordinates
    clib.lib()
    det_model, pose_model, lift_model = odet.FasterRCNNRef(det_sd), onets.HRNetRef(pose_sd, 48), onets.VideoPose3DRef(lift_sd)
    pick = sorted({int(round(i * (len(frames) - 1) / max(1, n_frames - 1))) for i in range(n_frames)})
    ref, crops, dt, t_det = [], [], 0.0, 0.0
    for j, fi in enumerate(pick):
        frame_bgr, gt_box = frames[fi], gt[fi][0]
        t0 = time.perf_counter()
        dets = odet.detect(det_model, frame_bgr[:, :, ::-1])
        t1 = time.perf_counter()
        bb = np.array([gt_box[0], gt_box[1], gt_box[2] - gt_box[0], gt_box[3] - gt_box[1]], np.float64)
        t, c, s, _ = opre.top_down_input(frame_bgr[:, :, ::-1], bb, (288, 384))
        hm = pose_model.forward(t[None])
        hmf = pose_model.forward(np.ascontiguousarray(t[None, :, :, ::-1]))
        kp, _ = odec.decode_topdown(hm, hmf, hrnet.COCO_FLIP_PAIRS, c[None], s[None], post_process="unbiased", kernel=17)
        kn = normalize_screen_coordinates(kp[:, :, :2].astype(np.float64), 1920, 1080).astype(np.float32)
        k3 = lift_model.forward(onets.videopose3d_windows(kn, 121))
        if j < timed_frames:
            dt += time.perf_counter() - t0
            t_det += t1 - t0
        ref.append((fi, bb, dets, kp, k3))
        crops.append((t, c, s, kp))
    n_timed = min(timed_frames, len(pick))
    readout = {}
    for mode, cas in cascades.items():
        if cas is None:
            continue
        eq, box_d, sc_d, d2, d3, n_det, n_match, n_dev = 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0
        for fi, bb, dets, kp, k3 in ref:
            g = cas.detector.run(frames[fi][None])[0]
            kg, _ = cas.topdown.run(frames[fi][None], np.zeros(1, np.int32), bb[None])
            k3g = lift(cas.lift_net, cas.lift_spec, normalize_screen_coordinates(kg[:, :, :2].astype(np.float64), 1920, 1080))
            eq += bool(g.shape == dets.shape and np.array_equal(g, dets))
            n_det += len(dets)
            n_dev += len(g)
            # row order follows the scores, and near-tied scores swap places under any change of the float32 summation order:
            # match every oracle detection to the device detection with the nearest box
            for row in dets:
                if len(g):
                    d = np.abs(g[:, :4] - row[:4]).max(axis=1)
                    j = int(np.argmin(d))
                    if d[j] <= 0.05:
                        n_match += 1
                        box_d = max(box_d, float(d[j]))
                        sc_d = max(sc_d, float(abs(g[j, 4] - row[4])))
            d2 = max(d2, float(np.abs(kg[0, :, :2] - kp[0, :, :2]).max()))
            d3 = max(d3, float(np.abs(k3g - k3).max()))
        readout[mode] = {"frames": len(ref), "frames_with_bit_identical_detections": eq, "oracle_detections": n_det,
                         "device_detections": n_dev, "oracle_detections_matched_within_0.05px": n_match,
                         "max_abs_diff_boxes_px": box_d, "max_abs_diff_scores": sc_d, "max_abs_diff_2d_px": d2, "max_abs_diff_3d": d3,
                         "note": "seeded-random detector / pose weights (lifting weights: metre-sized contractions): the detector's 100-of-~1000 cut and NMS sit on near-ties, heat-maps are noise "
                                 "(ill-conditioned arg-max / DARK step); the tolerance claims are tests/test_gpu_parity_modes.py "
                                 "(well-conditioned weights, margin-aware detector check)"}
    readout["fp32_reordering_control"] = reordering_control(cascades.get("default"), pose_sd, crops)
    readout["well_conditioned_end_to_end"] = parity_well_conditioned(cascades.get("default"), frames, gt, pick[:3])
    return {"value": n_timed / dt, "unit": "frames/s", "cores": clib.N_THREADS, "kind": "port",
            "sample": "%d synthetic 1080p frame(s) through the CPU restatement of detect + top-down 2D (W48, flip) + one lifting window "
                      "(%.1f s, detector %.1f s); parity readout over %d frames" % (n_timed, dt, t_det, len(ref)),
            "parity_vs_gpu": readout}


def reordering_control(cas, pose_sd, crops):
    """How far do the SAME frames' joints move under a float32 evaluation that is as valid as the oracle's but sums in another order?
    The bit-exact float32-MFMA kernels on the TRANSPOSED network (inputs and every kernel transposed, heat-maps transposed back: the
    FMA chain visits the taps in another order -- what separates the oracle from the reference's own cuDNN / BLAS), decoded by the
    same decode kernel, against the oracle's joints.  It is what `max_abs_diff_2d_px` of the modes above is to be read against: with
    the timed workload's seeded-random pose weights the heat-maps are noise and DARK's Taylor step is ill-conditioned.
    crops: [(tensor [3][H][W], center, scale, oracle joints [1][K][3])]."""
    if cas is None or not crops:
        return None
    from posepipeline_amd import ops
    from posepipeline_amd.models import hrnet
    from posepipeline_amd.program import Net
    spec = hrnet.hrnet_w48_384x288()
    tspec = hrnet.HRNetSpec(spec.width, spec.num_joints, spec.in_w, spec.in_h)
    tsd = {k: (np.ascontiguousarray(np.transpose(v, (0, 1, 3, 2))) if np.ndim(v) == 4 else v) for k, v in pose_sd.items()}
    tnet = Net(cas.ctx, hrnet.build_hrnet_program(tspec, tsd), max_batch=2, numerics="exact")
    worst, n_over, n_joint = 0.0, 0, 0
    for t, c, sc, kp in crops:
        x = np.zeros((2, spec.in_w, spec.in_h, 4), np.float32)          # transposed NHWC: [W][H][c]
        x[0, :, :, :3] = np.transpose(t, (2, 1, 0))
        x[1, :, :, :3] = np.transpose(t[:, :, ::-1], (2, 1, 0))          # the flipped crop
        hm = tnet.forward(x).reshape(2, 17, spec.in_w // 4, spec.in_h // 4)      # (heat-maps leave as NCHW planes: [K][W/4][H/4] here)
        hm = np.ascontiguousarray(np.transpose(hm, (0, 1, 3, 2)))               # -> [2][K][H/4][W/4]
        cs = np.array([[c[0], c[1], sc[0], sc[1]]], np.float32)
        kc, _ = ops.flip_merge_decode(cas.ctx, hm[:1], hm[1:], cs, flip_perm=hrnet.flip_perm(17), post="unbiased", blur_kernel=17)
        d = np.abs(kc[0, :, :2] - kp[0, :, :2]).max(axis=1)
        worst = max(worst, float(d.max()))
        n_over += int((d > 1e-3).sum())
        n_joint += d.size
    return {"max_abs_diff_2d_px": worst, "joints_beyond_1e-3_px": n_over, "joints": n_joint,
            "note": "the bit-exact float32-MFMA kernels on the TRANSPOSED HRNet (another summation order of the same float32 arithmetic) "
                    "vs the oracle's joints on the same crops: the movement ANY equally valid float32 evaluation shows on these "
                    "(seeded-random, ill-conditioned) heat-maps -- the yardstick for the modes' max_abs_diff_2d_px"}


def parity_well_conditioned(cas, frames, gt, pick):
    """north_star's tolerance on the cascade's OUTPUT, read where it is well-posed: the same 2D -> 3D stages in the DEFAULT
    numerics with well-conditioned weights (synth.smooth_state_dict / smooth_lifting_state_dict: single-peaked heat-maps,
    metre-sized 3D outputs, lifting sensitivity <= 1) on blob persons pasted at the replayed boxes; oracle 2D chain -> oracle
    lifting against the device's 2D -> 3D.  The assertion of the same figures is tests/test_gpu_parity_modes.py::
    test_end_to_end_3d_against_the_oracle_chain; this is the readout beside the timed line."""
    if cas is None:
        return None
    from oracle import decode as odec
    from oracle import nets as onets
    from oracle import preprocess as opre
    from posepipeline_amd import ops
    from posepipeline_amd.models import hrnet, synth
    from posepipeline_amd.models import videopose3d as vp3d
    from posepipeline_amd.program import Net
    from posepipeline_amd.wrappers.videopose3d import lift, normalize_screen_coordinates
    ctx, spec, lspec = cas.ctx, hrnet.hrnet_w48_384x288(), vp3d.VideoPose3DSpec()
    pose_sd = synth.smooth_state_dict(hrnet.hrnet_param_shapes(spec), seed=11)
    lift_sd = synth.smooth_lifting_state_dict(vp3d.videopose3d_param_shapes(lspec), seed=3)
    net = Net(ctx, hrnet.build_hrnet_program(spec, pose_sd), max_batch=2)
    lnet = Net(ctx, vp3d.build_videopose3d_program(lspec, lift_sd), max_batch=1)
    td = ops.TopDown(net, 17, flip_perm=hrnet.flip_perm(17), post="unbiased", blur_kernel=17)
    pose_model, lift_model = onets.HRNetRef(pose_sd, 48), onets.VideoPose3DRef(lift_sd)
    rng = np.random.default_rng(9)
    k2_dev, k2_ref = [], []
    for fi in pick:
        g = gt[fi][0]
        x0, y0, x1, y1 = (int(v) for v in g[:4])
        img = np.full_like(frames[fi], 30)
        yy, xx = np.mgrid[0:y1 - y0, 0:x1 - x0].astype(np.float32)
        for c in range(3):                      # one bright blob per colour plane: what a smoothing pose network peaks on
            cy, cx, sg = rng.uniform(0.4, 0.6) * (y1 - y0), rng.uniform(0.4, 0.6) * (x1 - x0), rng.uniform(0.05, 0.09) * (y1 - y0)
            img[y0:y1, x0:x1, c] = np.clip(30 + 190 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg)), 0, 255).astype(np.uint8)
        bb = np.array([g[0], g[1], g[2] - g[0], g[3] - g[1]], np.float64)
        kg, _ = td.run(img[None], np.zeros(1, np.int32), bb[None])
        t, c, sc, _ = opre.top_down_input(img[:, :, ::-1], bb, (288, 384))
        hm = pose_model.forward(t[None])
        hmf = pose_model.forward(np.ascontiguousarray(t[None, :, :, ::-1]))
        kp, _ = odec.decode_topdown(hm, hmf, hrnet.COCO_FLIP_PAIRS, c[None], sc[None], post_process="unbiased", kernel=17)
        k2_dev.append(kg[0])
        k2_ref.append(kp[0])
    k2_dev, k2_ref = np.asarray(k2_dev), np.asarray(k2_ref)
    norm = lambda k: normalize_screen_coordinates(k[:, :, :2].astype(np.float64), 1920, 1080).astype(np.float32)
    k3_dev = lift(lnet, lspec, normalize_screen_coordinates(k2_dev[:, :, :2].astype(np.float64), 1920, 1080))
    k3_ref = lift_model.forward(onets.videopose3d_windows(norm(k2_ref), 121))
    d3, r3 = float(np.abs(k3_dev - k3_ref).max()), float(np.abs(k3_ref).max())
    net.close()
    lnet.close()
    return {"numerics": net.numerics, "frames": len(pick), "max_abs_diff_2d_px": float(np.abs(k2_dev[:, :, :2] - k2_ref[:, :, :2]).max()),
            "max_abs_diff_3d_m": d3, "max_abs_diff_3d_of_output_range": d3 / r3, "output_range_m": r3,
            "lifting_sensitivity_bound": synth.max_norm_gain_bound(lift_sd),
            "bars": "2D <= 1e-3 px, 3D <= 1e-6 m (1e-3 mm) and <= 1e-6 of the output range"}


def run_c2(args, D):
    from posepipeline_amd import _lib, ops
    from posepipeline_amd.models import hrnet, synth
    from posepipeline_amd.program import Net

    ctx = _lib.Context(D.local_rank)
    spec = hrnet.hrnet_w32_256x192()
    sd = synth.synth_state_dict(hrnet.hrnet_param_shapes(spec), seed=1)
    prog = hrnet.build_hrnet_program(spec, sd)
    prog.blob = D.bcast_blob(prog.blob)
    n = args.batch
    net = Net(ctx, prog, max_batch=2 * n)
    # mmpose's W32 256x192 configs decode with post_process='default' 
    td = ops.TopDown(net, num_joints=17, flip_perm=hrnet.flip_perm(17), post="default")
    rng = np.random.default_rng(1000 + D.rank)                    # config index 1, per-rank shard
    x = np.zeros((n, spec.in_h, spec.in_w, 4), np.float32)
    x[..., :3] = rng.standard_normal((n, spec.in_h, spec.in_w, 3)).astype(np.float32)
    cs = np.tile(np.array([[96.0, 128.0, 192 / 200 * 1.25, 256 / 200 * 1.25]], np.float32), (n, 1))
    dptr, _, _ = net.buffer("input")
    ctx.h2d(dptr, x)                                              # inputs resident in HBM before timing
    for _ in range(args.warmup):
        kp = td.run_precropped(dptr, cs, n=n)
    D.barrier(ctx)
    t0 = time.perf_counter()
    t_net = t_pre = t_dec = 0.0
    for _ in range(args.steps):
        kp = td.run_precropped(dptr, cs, n=n)
        a, b, c = td.timing()
        t_pre, t_net, t_dec = t_pre + a, t_net + b, t_dec + c
    D.barrier(ctx)
    dt = D.max_time(time.perf_counter() - t0)
    if D.rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"keypoints": kp})
    n_launch = len(prog.ops)
    flops_step = prog.flops * 2 * n
    net_ms = t_net / args.steps
    achieved = flops_step / (net_ms * 1e-3) / 1e12
    out = {
        "metric": METRIC, "value": D.world * n * args.steps / dt, "unit": "frames/s", "n_gpus": D.world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32" + DTYPE_NOTE, "data": "synthetic",
        "config": {"workload": "configs[1]: HRNet-W32 256x192 top-down 2D, pre-cropped persons, flip_test, decode 'default'",
                   "frames_per_step_per_gpu": n, "backbone_samples_per_step": 2 * n,
                   "not_in_this_line": "detector, tracker, 3D lifting (see --workload cascade)"},
    }
    if not args.full:
        return out
    out["roofline"] = {**roofline_families(kernel_families([(net, 2 * n)])),
                       "traffic": pmc_traffic("c2_batch%d" % n)[0],
                       "program": {"achieved": achieved, "launches": n_launch, "flops_per_launch": flops_step / n_launch,
                                   "avg_launch_ms": net_ms / n_launch,
                                   "note": "whole backbone program inside the timed region (4 HIP streams): FLOPs / wall time"},
                       "stage_ms": {"pre": t_pre / args.steps, "backbone": net_ms, "decode": t_dec / args.steps}}
    n_cpu = 6 if args.cpu_frames is None else args.cpu_frames
    if n_cpu > 0 and D.world == 1:
        out["cpu_baseline"] = cpu_baseline_c2(sd, x[:n_cpu], cs[:n_cpu], kp[:n_cpu])
    return out


def cpu_baseline_c2(sd, x, cs, kp_gpu):
    """per-frame batch-1 loop like pose_pipeline/wrappers/mmpose.py:60-76 on the CPU oracle"""
    from oracle import clib
    from oracle import decode as odec
    from oracle import nets as onets
    from posepipeline_amd.models import hrnet
    model = onets.HRNetRef(sd, 32)
    clib.lib()
    t0 = time.perf_counter()
    kps = []
    for i in range(x.shape[0]):
        img = np.ascontiguousarray(np.transpose(x[i:i + 1, :, :, :3], (0, 3, 1, 2)))
        hm = model.forward(img)
        hmf = model.forward(np.ascontiguousarray(img[:, :, :, ::-1]))
        k, _ = odec.decode_topdown(hm, hmf, hrnet.COCO_FLIP_PAIRS, cs[i:i + 1, :2], cs[i:i + 1, 2:], post_process="default")
        kps.append(k[0])
        if time.perf_counter() - t0 > 20.0:       # bounded sample: stop after ~20 s of CPU work
            break
    dt = time.perf_counter() - t0
    m = len(kps)
    return {"value": m / dt, "unit": "frames/s", "cores": clib.N_THREADS, "kind": "port",
            "sample": "%d of the same pre-cropped frames, batch-1 loop, C/OpenMP fmaf-chain convs + numpy decode (%.1f s)" % (m, dt),
            "max_abs_diff_px_vs_gpu": float(np.abs(np.array(kps) - kp_gpu[:m]).max())}


def run_c5(args, D):
    """BASELINE.json configs[4] on one GPU per rank: ViTPose-H 256x192 top-down 2D (bf16 MFMA encoder, flip test, UDP
    decode) on pre-cropped persons.  ViTPose is not in the reference tree: a parity-test configuration
    with its own bench line, not the headline metric."""
    from posepipeline_amd import _lib, ops
    from posepipeline_amd.models import hrnet, vitpose
    from posepipeline_amd.program import Net

    ctx = _lib.Context(D.local_rank)
    spec = vitpose.vitpose_huge()
    p = vitpose.synth_params(spec, seed=5)
    prog = vitpose.build_vitpose_program(spec, p)
    prog.blob = D.bcast_blob(prog.blob)
    n = args.batch
    net = Net(ctx, prog, max_batch=2 * n)
    td = ops.TopDown(net, num_joints=17, flip_perm=hrnet.flip_perm(17), shift_heatmap=False, post="udp", blur_kernel=11)
    rng = np.random.default_rng(5000 + D.rank)
    x = np.zeros((n, spec.in_h, spec.in_w, 4), np.float32)
    x[..., :3] = rng.standard_normal((n, spec.in_h, spec.in_w, 3)).astype(np.float32)
    cs = np.tile(np.array([[96.0, 128.0, 192 / 200 * 1.25, 256 / 200 * 1.25]], np.float32), (n, 1))
    dptr, _, _ = net.buffer("input")
    ctx.h2d(dptr, x)
    for _ in range(args.warmup):
        kp = td.run_precropped(dptr, cs, n=n)
    D.barrier(ctx)
    t0 = time.perf_counter()
    t_net = t_pre = t_dec = 0.0
    for _ in range(args.steps):
        kp = td.run_precropped(dptr, cs, n=n)
        a, b, c = td.timing()
        t_pre, t_net, t_dec = t_pre + a, t_net + b, t_dec + c
    D.barrier(ctx)
    dt = D.max_time(time.perf_counter() - t0)
    if D.rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"keypoints": kp})
    out = {
        "metric": METRIC, "value": D.world * n * args.steps / dt, "unit": "frames/s", "n_gpus": D.world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": "configs[4] on one GPU per rank: ViTPose-H 256x192 top-down 2D, pre-cropped persons, flip_test, "
                               "UDP decode (bf16 MFMA encoder, fp32 patch embedding and deconvolution head)",
                   "frames_per_step_per_gpu": n, "backbone_samples_per_step": 2 * n,
                   "gflop_per_frame": prog.flops * 2 / 1e9,
                   "not_in_this_line": "detector, tracker, 3D lifting (see --workload cascade); ViTPose is not in the reference tree"},
    }
    if not args.full:
        return out
    # roofline leg (outside the timed region): HIP events after every encoder launch, summed per kernel family
    ms3 = np.zeros(3, np.float32)
    n_gemm = ctypes.c_int(0)
    _lib.check(ctx.lib.pp_net_vit_timing(net.handle, 1, None, None))
    td.run_precropped(dptr, cs, n=n)
    _lib.check(ctx.lib.pp_net_vit_timing(net.handle, 0, _lib.ptr(ms3), ctypes.byref(n_gemm)))
    m_rows, d, hid = 2 * n * spec.tokens, spec.dim, spec.dim * spec.mlp_ratio
    gemm_flops = 2.0 * m_rows * (4 * d * d + 2 * d * hid) * spec.depth
    achieved = gemm_flops / (float(ms3[0]) * 1e-3) / 1e12
    net_ms = t_net / args.steps
    out["roofline"] = {"bound": "mfma", "kernel": "gemm_bf16_kernel (%d launches per step: qkv / proj / fc1 / fc2 of %d blocks)" % (n_gemm.value, spec.depth),
                       "achieved": achieved, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / BF16_MFMA_PEAK_TFLOPS,
                       "traffic": pmc_traffic("c5_batch%d" % n)[0], "flops_per_launch": gemm_flops / max(n_gemm.value, 1),
                       "avg_launch_ms": float(ms3[0]) / max(n_gemm.value, 1),
                       "encoder_ms": {"gemm": float(ms3[0]), "layernorm": float(ms3[1]), "attention": float(ms3[2])},
                       "program_tflops": prog.flops * 2 * n / (net_ms * 1e-3) / 1e12,
                       "stage_ms": {"pre": t_pre / args.steps, "backbone": net_ms, "decode": t_dec / args.steps}}
    n_cpu = 1 if args.cpu_frames is None else args.cpu_frames
    if n_cpu > 0 and D.world == 1:
        hm_gpu = net.read("output", 2 * n).reshape(2 * n, 17, *spec.heatmap_hw)
        out["cpu_baseline"] = cpu_baseline_c5(p, spec, x[:n_cpu], cs[:n_cpu], kp[:n_cpu], hm_gpu[:n_cpu], hm_gpu[n:n + n_cpu])
    return out


def cpu_baseline_c5(p, spec, x, cs, kp_gpu, hm_gpu, hmf_gpu):
    """batch-1 loop on the CPU oracle (numpy float64 contractions of the bf16-rounded operands).  The bf16 network is
    compared on its heatmaps (a randomly initialised net has no stable argmax); the decode is compared on the GPU's own
    heatmaps."""
    from oracle import decode as odec
    from oracle import vit as ovit
    from posepipeline_amd.models import hrnet
    t0 = time.perf_counter()
    m, err = 0, 0.0
    for i in range(x.shape[0]):
        hm = ovit.forward(x[i:i + 1], p, spec, emulate_bf16=True)
        hmf = ovit.forward(np.ascontiguousarray(x[i:i + 1, :, ::-1]), p, spec, emulate_bf16=True)
        odec.decode_topdown_udp(hm, hmf, hrnet.COCO_FLIP_PAIRS, cs[i:i + 1, :2], cs[i:i + 1, 2:], kernel=11)
        m += 1
        err = max(err, float(np.abs(hm[0] - hm_gpu[i]).max() / np.abs(hm[0]).max()),
                  float(np.abs(hmf[0] - hmf_gpu[i]).max() / np.abs(hmf[0]).max()))
        if time.perf_counter() - t0 > 20.0:
            break
    dt = time.perf_counter() - t0
    k_ref, _ = odec.decode_topdown_udp(hm_gpu[:m], hmf_gpu[:m], hrnet.COCO_FLIP_PAIRS, cs[:m, :2], cs[:m, 2:], kernel=11)
    try:        # threads the BLAS behind numpy actually runs (the contractions are > 95 % of this leg)
        from threadpoolctl import threadpool_info
        cores = max([i.get("num_threads", 1) for i in threadpool_info() if i.get("user_api") == "blas"] or [1])
    except Exception:
        cores = os.cpu_count()
    return {"value": m / dt, "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "%d of the same pre-cropped frames, batch-1 loop, numpy/BLAS float64 contractions + numpy decode (%.1f s)" % (m, dt),
            "heatmap_max_rel_diff_vs_gpu": err,
            "decode_max_abs_diff_px_on_gpu_heatmaps": float(np.abs(k_ref - kp_gpu[:m]).max())}


def run_track0(args, D):
    """tracking_method 0 (DeepSortYOLOv4): YOLOv4 person detector + mars-small128 features +
    DeepSORT on 1080p frames resident in HBM.  Not the headline metric; same JSON shape for comparison."""
    from posepipeline_amd import _lib, ops
    from posepipeline_amd.models import mars, yolov4
    from posepipeline_amd.tracking import Tracker

    ctx = _lib.Context(D.local_rank)
    B = args.chunk
    ysd = yolov4.synth_params(yolov4.yolov4_param_shapes(), seed=4, head_bias=-2.0)
    msd = yolov4.synth_params(mars.mars_param_shapes(), seed=5)
    det = yolov4.YoloV4Detector(ctx, ysd, 1080, 1920, max_frames=B)
    enc = mars.MarsEncoder(ctx, msd, 1080, 1920, max_patches=256)
    rng = np.random.default_rng(5000 + D.rank)
    frames, gt = synth_1080p(rng, B, args.persons)
    dptr = ctx.malloc(frames.nbytes)
    ctx.h2d(dptr, frames)
    tracker = Tracker(mode=0, feat_dim=128, max_cosine_distance=0.3)
    t_net = [0.0]
    # as in the cascade: the random-weight detector runs (and is decoded) for timing, downstream boxes are the replayed
    # synthetic persons (x, y, w, h ints like yolo.detect_image returns, score 0.9)
    replay = [(np.array([[int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])] for b in g], np.int64).reshape(-1, 4),
               np.full(len(g), 0.9, np.float32)) for g in gt]

    def step():
        n = det.preprocess(None, frames_dev=(dptr, B))
        ctx.timer_start()
        det.net.run(n)
        t_net[0] += ctx.timer_stop()
        det.decode(n)
        dets = replay
        feats = enc.encode(None, [b for b, _ in dets], frames_dev=(dptr, B))
        n_trk = 0
        for (boxes, conf), feat in zip(dets, feats):
            tlwh, sc = boxes.astype(np.float64), conf.astype(np.float64)
            keep = ops.nms(ctx, tlwh, sc, 1.0, convention=1) if len(tlwh) else np.zeros(0, np.int64)
            ids, _, _ = tracker.step(tlwh[keep], sc[keep], feat[keep])
            n_trk += len(ids)
        return sum(len(b) for b, _ in dets), n_trk

    for _ in range(args.warmup):
        step()
    t_net[0] = 0.0
    D.barrier(ctx)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        n_det, n_trk = step()
    D.barrier(ctx)
    dt = D.max_time(time.perf_counter() - t0)
    if D.rank != 0:
        return
    net_ms = t_net[0] / args.steps
    flops_step = det.prog.flops * B
    achieved = flops_step / (net_ms * 1e-3) / 1e12
    n_launch = sum(1 for op in det.prog.ops if op.type == 1)
    out = {
        "metric": "frames/sec, DeepSortYOLOv4 tracking stage on 1080p (not the headline metric)",
        "value": D.world * B * args.steps / dt, "unit": "frames/s", "n_gpus": D.world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "tracking_method 0: letterbox -> YOLOv4 416 -> decode/NMS -> mars-small128 -> DeepSORT",
                   "frames_per_step_per_gpu": B, "persons_per_frame": args.persons, "tracks_per_step": n_trk,
                   "detector_boxes": "detector + decode + NMS run on every frame; downstream boxes are replayed synthetic persons"},
    }
    if not args.full:
        return out
    # per kernel family, live (HIP events around every launch of one serial pass): YOLOv4's 3x3 / wide 1x1 layers run on the
    # split kernels since round 2, so the dominant family and ITS peak are reported, not the fp32 kernels' 157.3
    out["roofline"] = {**roofline_families(kernel_families([(det.net, B)])), "traffic": None,
                       "program": {"achieved": achieved, "launches": n_launch, "flops_per_launch": flops_step / n_launch,
                                   "avg_launch_ms": net_ms / n_launch,
                                   "note": "YOLOv4 program inside the timed region (Mish epilogues in fp64): FLOPs / wall time"}}
    return out


def run_cascade0(args, D):
    """The same cascade with the reference recipes' DEFAULT tracking method (tracking_method 0, DeepSortYOLOv4:
    utils/standard_pipelines.py:12,58,112) in place of mmtracking's Faster-RCNN + SORT.  Secondary line: the headline
    metric stays --workload cascade (the mmpose / mmtracking path BASELINE.json names)."""
    from posepipeline_amd import _lib
    from posepipeline_amd.cascade import Cascade
    from posepipeline_amd.models import hrnet, mars, synth, yolov4
    from posepipeline_amd.models import videopose3d as vp3d

    ctx = _lib.Context(D.local_rank)
    B, P = args.chunk, args.persons
    ysd = yolov4.synth_params(yolov4.yolov4_param_shapes(), seed=4, head_bias=-2.0)
    msd = yolov4.synth_params(mars.mars_param_shapes(), seed=5)
    pose_spec = hrnet.hrnet_w48_384x288()
    pose_sd = synth.synth_state_dict(hrnet.hrnet_param_shapes(pose_spec), seed=1)
    lift_sd = synth.synth_state_dict(vp3d.videopose3d_param_shapes(vp3d.VideoPose3DSpec()), seed=3)
    cas = Cascade(ctx, (ysd, msd), pose_sd, lift_sd, 1080, 1920, chunk=B, max_persons=P, tracking="DeepSortYOLOv4")
    rng = np.random.default_rng(3000 + D.rank)
    frames, gt = synth_1080p(rng, B, P)
    dptr = ctx.malloc(frames.nbytes)
    ctx.h2d(dptr, frames)
    st = {"yolo": 0.0, "pose": 0.0}

    def step():
        res = cas.step(None, frames_dev=(dptr, B), replay=gt)
        st["yolo"] += cas.detector.last_net_ms
        st["pose"] += cas.topdown.timing()[1]
        return res

    for _ in range(args.warmup):
        step()
    st["yolo"] = st["pose"] = 0.0
    D.barrier(ctx)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    D.barrier(ctx)
    dt = D.max_time(time.perf_counter() - t0)
    if D.rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, cascade_outputs(res))
    K = args.steps
    conv_ms = (st["yolo"] + st["pose"]) / K
    flops_step = B * (cas.detector.flops_per_frame + 2 * P * cas.pose_net.prog.flops)
    n_launch = len(cas.detector.prog.ops) + len(cas.pose_net.prog.ops)
    achieved = flops_step / (conv_ms * 1e-3) / 1e12
    out = {
        "metric": METRIC, "value": D.world * B * K / dt, "unit": "frames/s", "n_gpus": D.world, "steps": K, "warmup": args.warmup,
        "ms_per_step": dt / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "the cascade with the reference recipes' default tracker (tracking_method 0): 1080p letterbox -> YOLOv4 416 "
                               "-> mars-small128 -> DeepSORT -> HRNet-W48 384x288 flip_test + DARK decode -> VideoPose3D 243-frame lifting",
                   "frames_per_step_per_gpu": B, "persons_per_frame": P, "gflop_per_frame": flops_step / B / 1e9,
                   "tracks_in_last_frame": len(res["tracks"][-1]),
                   "detector_boxes": "detector + decode + NMS run on every frame; downstream boxes are replayed synthetic GT (random-weight detector)"},
    }
    if not args.full:
        return out
    out["roofline"] = {**roofline_families(kernel_families([(cas.detector.net, B), (cas.pose_net, 2 * B * P)])), "traffic": None,
                       "programs": {"achieved": achieved, "launches": n_launch, "flops_per_launch": flops_step / n_launch,
                                    "avg_launch_ms": conv_ms / n_launch,
                                    "note": "YOLOv4 + HRNet-W48 programs inside the timed region: FLOPs / wall time"},
                       "stage_ms": {"yolo_backbone": st["yolo"] / K, "pose_backbone": st["pose"] / K}}
    return out


def run_plumbing(args, D):
    """No kernels: the rank plumbing of an N-rank run (launcher, process group, weight broadcast, barrier, max-over-ranks
    clock) -- `python bench.py --gpus 2 --workload plumbing` with POSEPIPE_DIST_BACKEND=gloo rehearses the multi-GPU launch on a
    box without GPUs (tests/test_distributed_gloo.py)."""
    class _NoCtx:
        def synchronize(self):
            pass
    blob = np.arange(4096, dtype=np.float32) * (1.0 if D.rank == 0 else -1.0)
    got = D.bcast_blob(blob)
    D.barrier(_NoCtx())
    t = D.max_time(1.0 + D.rank)
    oks = D.gather_obj(bool(np.array_equal(got, np.arange(4096, dtype=np.float32))))
    return {"metric": "rank plumbing only (no kernels)", "value": 0.0, "unit": "frames/s", "n_gpus": D.world, "steps": args.steps,
            "warmup": args.warmup, "slowest_rank_clock": t, "weights_identical_on_every_rank": all(oks)}


def main():
    args = parse()
    if args.gpus is not None and args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args, sys.argv[1:])
    D = Dist(args.gpus)
    try:
        out = {"cascade": run_cascade, "c2": run_c2, "c5": run_c5, "cascade5": run_cascade, "track0": run_track0,
               "cascade0": run_cascade0, "plumbing": run_plumbing}[args.workload](args, D)
        topo = D.describe()
        if D.rank == 0 and out is not None:
            out["distributed"] = topo
            if out.pop("_wants_secondary", False):
                import gc
                gc.collect()                                   # the headline's cascades are gone: their HBM is free for the legs
                try:
                    out["secondary"] = secondary_lines(args)
                except Exception as e:                         # never at the price of the headline line
                    out["secondary"] = {"error": "%s: %s" % (type(e).__name__, e)}
            print(json.dumps(out), flush=True)
        elif out is not None:
            out.pop("_wants_secondary", None)
    finally:
        D.close()


if __name__ == "__main__":
    main()
