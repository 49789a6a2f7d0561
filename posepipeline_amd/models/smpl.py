"""The SMPL body model's data: the joint sets, the kinematic tree, a loader for the real model and a seeded synthetic stand-in.

The arithmetic runs on the device (csrc/smpl.hip, ops.SmplModel); tests/vibe_ref.py restates it in numpy.  What lives here is what
both need to agree on:

  PARENTS          SMPL's 24-joint kinematic tree (smplx `parents`, root = -1)
  VERTEX_IDS_SMPLH the 21 mesh vertices smplx's VertexJointSelector appends to the 24 chain joints (its `smplh` table): nose, right /
                   left eye, right / left ear, then left big toe, left small toe, left heel, right big toe, right small toe, right
                   heel, then five left and five right finger tips (thumb, index, middle, ring, pinky)
  JOINT_NAMES_49 / JOINT_MAP_54  SPIN's constants.py: the 49 joints of `SMPLPerson.joints3d` (25 OpenPose + 24 ground-truth joints) and,
                   for each, its index among the 54 joints (24 chain, 21 picked, 9 from J_regressor_extra)

UNPINNED: smplx and SPIN are not in the reference tree; the tables are restated from their published sources.  The
joint NAMES are pinned: tests/golden/joint_names_49.json holds the reference's list (pose_pipeline/utils/smpl.py:6-58).

Body model file: `vibe/SMPL_NEUTRAL.npz` under MODEL_DATA_DIR with v_template [6890][3], shapedirs [6890][3][10], posedirs
[207][20670], J_regressor [24][6890], weights [6890][24], J_regressor_extra [9][6890] (the reference unpickles SMPL_NEUTRAL.pkl,
which needs chumpy, and reads J_regressor_extra.npy beside it).  It is never fetched.
"""
from __future__ import annotations

import os

import numpy as np

from .. import weights as _weights

N_VERTS = 6890
N_JOINTS = 24
BODY_MODEL = "vibe/SMPL_NEUTRAL.npz"
PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)

VERTEX_IDS_SMPLH = (332, 6260, 2800, 4071, 583,                      # nose, right eye, left eye, right ear, left ear
                    3216, 3226, 3387, 6617, 6624, 6787,              # left big toe, small toe, heel; right big toe, small toe, heel
                    2746, 2319, 2445, 2556, 2673,                    # left thumb, index, middle, ring, pinky
                    6191, 5782, 5905, 6016, 6133)                    # right thumb, index, middle, ring, pinky

_OPENPOSE = ("Nose", "Neck", "RShoulder", "RElbow", "RWrist", "LShoulder", "LElbow", "LWrist", "MidHip", "RHip", "RKnee", "RAnkle", "LHip",
             "LKnee", "LAnkle", "REye", "LEye", "REar", "LEar", "LBigToe", "LSmallToe", "LHeel", "RBigToe", "RSmallToe", "RHeel")
_LIMBS = ("Ankle", "Knee", "Hip"), ("Wrist", "Elbow", "Shoulder")
# 25 OpenPose joints, then the 24 joints of the training sets: right leg up, left leg down, right arm up, left arm down, the spine, the face
JOINT_NAMES_49 = ([f"OP {n}" for n in _OPENPOSE]
                  + [f"Right {p}" for p in _LIMBS[0]] + [f"Left {p}" for p in reversed(_LIMBS[0])]
                  + [f"Right {p}" for p in _LIMBS[1]] + [f"Left {p}" for p in reversed(_LIMBS[1])]
                  + ["Neck (LSP)", "Top of Head (LSP)", "Pelvis (MPII)", "Thorax (MPII)", "Spine (H36M)", "Jaw (H36M)", "Head (H36M)",
                     "Nose", "Left Eye", "Right Eye", "Left Ear", "Right Ear"])

# index among the 54 joints of each of the 49 (SPIN constants.JOINT_MAP in JOINT_NAMES order)
JOINT_MAP_54 = (24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                8, 5, 45, 46, 4, 7, 21, 19, 17, 16, 18, 20, 47, 48, 49, 50, 51, 52, 53, 24, 26, 25, 28, 27)

ARRAYS = {"v_template": lambda v: (v, 3), "shapedirs": lambda v: (v, 3, 10), "posedirs": lambda v: (207, 3 * v),
          "J_regressor": lambda v: (24, v), "weights": lambda v: (v, 24), "J_regressor_extra": lambda v: (9, v)}


def vertex_ids(n_verts: int = N_VERTS) -> np.ndarray:
    """the 21 picked vertices; for a smaller (test) mesh the same ids folded into its range"""
    return (np.asarray(VERTEX_IDS_SMPLH, np.int64) % n_verts).astype(np.int32)


def synth_body_model(seed: int = 0, n_verts: int = N_VERTS) -> dict:
    """A seeded stand-in with the real model's shapes and scales: vertices in a 1 m box, shapedirs ~1e-2, posedirs ~1e-3, every
    J_regressor (and J_regressor_extra) row non-negative and summing to 1 over 32 random vertices, every skinning-weight row
    non-negative and summing to 1 over 4 random joints.  float32 arrays (the sums are 1 to float32 rounding)."""
    rng = np.random.default_rng(seed)
    v = int(n_verts)

    def sparse_rows(rows, cols, nnz):
        out = np.zeros((rows, cols), np.float64)
        for r in range(rows):
            idx = rng.choice(cols, size=min(nnz, cols), replace=False)
            w = rng.uniform(0.1, 1.0, idx.size)
            out[r, idx] = w / w.sum()
        return out.astype(np.float32)

    return {"v_template": rng.uniform(-0.5, 0.5, (v, 3)).astype(np.float32),
            "shapedirs": (rng.standard_normal((v, 3, 10)) * 1e-2).astype(np.float32),
            "posedirs": (rng.standard_normal((207, 3 * v)) * 1e-3).astype(np.float32),
            "J_regressor": sparse_rows(24, v, 32),
            "weights": sparse_rows(v, 24, 4),
            "J_regressor_extra": sparse_rows(9, v, 32)}


def check_body_model(body: dict) -> dict:
    v = int(np.shape(body["v_template"])[0])
    for k, shp in ARRAYS.items():
        if k not in body:
            raise KeyError(f"SMPL body model: array {k!r} is missing")
        if tuple(np.shape(body[k])) != shp(v):
            raise ValueError(f"SMPL body model: {k} has shape {tuple(np.shape(body[k]))}, expected {shp(v)}")
    return {k: np.ascontiguousarray(body[k], np.float32) for k in ARRAYS}


def load_body_model(seed: int = 3) -> dict:
    """vibe/SMPL_NEUTRAL.npz when it exists; the synthetic stand-in under POSEPIPE_SYNTHETIC_WEIGHTS=1; else FileNotFoundError"""
    path = os.path.join(_weights.model_data_dir(), BODY_MODEL)
    if os.path.exists(path):
        with np.load(path) as z:
            return check_body_model({k: z[k] for k in z.files})
    if os.environ.get("POSEPIPE_SYNTHETIC_WEIGHTS") == "1":
        return synth_body_model(seed)
    raise FileNotFoundError(f"{path} (set POSEPIPE_SYNTHETIC_WEIGHTS=1 to run with a seeded synthetic body model)")
