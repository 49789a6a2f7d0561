#!/usr/bin/env python
"""Values of the HigherHRNet-W48 bottom-up config the reference vendors, as JSON.

Runs only where a checkout of the reference (peabody124/PosePipeline) exists; tests/golden/arch_config_higherhrnet.json, which
it writes next to this script, is committed and is what tests/test_bottomup.py reads.  Nothing here copies the config file:
3rdparty/mmpose/config/bottom_up/higherhrnet/coco/higher_hrnet48_coco_512x512.py is EXECUTED (it is plain Python assignments)
and the settings a test needs are stored: `data_cfg`, the backbone (`extra`), `keypoint_head` without the loss, `test_cfg` and the
normalisation mean / std of the test pipeline.

usage: python tests/golden/make_goldens_higherhrnet.py <reference checkout>      (deterministic; rewrites the JSON)
"""
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
CFG = "3rdparty/mmpose/config/bottom_up/higherhrnet/coco/higher_hrnet48_coco_512x512.py"


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ns: dict = {}
    with open(os.path.join(sys.argv[1], CFG)) as f:
        exec(compile(f.read(), CFG, "exec"), ns)
    model = ns["model"]
    norm = [s for s in ns["val_pipeline"][2]["transforms"] if s["type"] == "NormalizeTensor"][0]
    out = {
        "source": CFG,
        "model_type": model["type"],
        "data_cfg": ns["data_cfg"],
        "backbone": {k: model["backbone"][k] for k in ("type", "in_channels", "extra")},
        "keypoint_head": {k: v for k, v in model["keypoint_head"].items() if k != "loss_keypoint"},
        "test_cfg": model["test_cfg"],
        "normalize": {"mean": norm["mean"], "std": norm["std"]},
        "val_pipeline_types": [s["type"] for s in ns["val_pipeline"]],
        "test_pipeline_is_val_pipeline": ns["test_pipeline"] is ns["val_pipeline"] or ns["test_pipeline"] == ns["val_pipeline"],
    }
    with open(os.path.join(OUT, "arch_config_higherhrnet.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
