#!/usr/bin/env python
"""tests/golden/fairmot_e2e.npz: the FairMOT reference chain of tests/fairmot_ref.py on the 6-frame 96 x 64 clip of
tests/test_gpu_fairmot.py, at the full 608 x 1088 network size, with the seeded weights POSEPIPE_SYNTHETIC_WEIGHTS=1 gives -- once
with the network in float64 (the reference) and once in float32 (its deviation sets the test's tolerance).  A float64 forward takes
about 20 s per frame on a CPU, which is why the result is recorded.  Asserts what the test relies on: no candidate score of either
chain within 1e-3 of conf_thres = 0.2, and the same tracks in both chains.

usage: python tests/golden/make_goldens_fairmot.py        (CPU only, about 3 minutes)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from posepipeline_amd.models import dla          # noqa: E402
from tests import fairmot_ref as R               # noqa: E402

SEED = 0


def main():
    sd = dla.synth_dla34_state_dict(dla.dla34_param_shapes(), 11)          # what dla.get_state_dict() seeds
    frames = R.rectangles_clip(6, 64, 96, seed=SEED)
    t64, s64 = R.chain(sd, frames, np.float64)
    t32, s32 = R.chain(sd, frames, np.float32)
    for a, b in zip(s64, s32):
        for s in (a, b):
            assert np.abs(s - 0.2).min() > 1e-3, np.abs(s - 0.2).min()
        assert int((a > 0.2).sum()) == int((b > 0.2).sum())
    t32 = R.relabel(t32, t64)
    out = {"seed": np.int64(SEED), "n_candidates": np.array([int((s > 0.2).sum()) for s in s64])}
    for f, (a, b) in enumerate(zip(t64, t32)):
        ids = [i for i, _, _ in a]
        assert sorted(ids) == sorted(i for i, _, _ in b), f
        by_id = {i: (box, s) for i, box, s in b}
        out[f"ids{f}"] = np.array(ids, np.int64)
        out[f"tlwh64_{f}"] = np.array([box for _, box, _ in a]).reshape(-1, 4)
        out[f"tlwh32_{f}"] = np.array([by_id[i][0] for i in ids]).reshape(-1, 4)
        out[f"score64_{f}"] = np.array([s for _, _, s in a], np.float64)
        out[f"score32_{f}"] = np.array([by_id[i][1] for i in ids], np.float64)
        print(f, len(ids), "tracks; candidates", out["n_candidates"][f], "box deviation", float(np.abs(out[f"tlwh64_{f}"] - out[f"tlwh32_{f}"]).max()) if ids else 0.0)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "fairmot_e2e.npz"), **out)


if __name__ == "__main__":
    main()
