#!/usr/bin/env python
"""Values of the HRFormer-B config the reference vendors, as JSON.

Runs only where a checkout of the reference (peabody124/PosePipeline) exists; tests/golden/arch_config_hrformer.json, which
it writes next to this script, is committed and is what tests/test_hrformer.py reads.  Nothing here copies the config file:
3rdparty/mmpose/config/top_down/hrformer_base_coco_384x288.py is EXECUTED (it is plain Python assignments) and the values a
test needs are stored: the backbone's `extra`, the head, `test_cfg`, image and heat-map size, mean / std and the step types of
the test pipeline.

usage: python tests/golden/make_goldens_hrformer.py <reference checkout>      (deterministic; rewrites the JSON)
"""
import json
import os
import re
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
CFG = "3rdparty/mmpose/config/top_down/hrformer_base_coco_384x288.py"


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ns: dict = {}
    with open(os.path.join(sys.argv[1], CFG)) as f:
        text = f.read()
    # mmcv substitutes `{{_base_.name}}` textually with the base file's value; the dataset description is not read here
    text = re.sub(r"\{\{\s*_base_\.\w+\s*\}\}", "None", text)
    exec(compile(text, CFG, "exec"), ns)
    model, data = ns["model"], ns["data_cfg"]
    head = model["keypoint_head"]
    norm = [s for s in ns["val_pipeline"] if s["type"] == "NormalizeTensor"][0]
    out = {
        "source": CFG,
        "model_type": model["type"],
        "backbone_type": model["backbone"]["type"],
        "extra": model["backbone"]["extra"],
        "head": {k: head[k] for k in ("type", "in_channels", "out_channels", "num_deconv_layers", "extra")},
        "test_cfg": model["test_cfg"],
        "image_size": data["image_size"],
        "heatmap_size": data["heatmap_size"],
        "mean": norm["mean"],
        "std": norm["std"],
        "val_pipeline_types": [s["type"] for s in ns["val_pipeline"]],
        "test_pipeline_is_val_pipeline": ns["test_pipeline"] is ns["val_pipeline"] or ns["test_pipeline"] == ns["val_pipeline"],
    }
    with open(os.path.join(OUT, "arch_config_hrformer.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
