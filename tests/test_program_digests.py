"""Every program builder of posepipeline_amd/models, byte for byte.

A sha256 over everything a Program holds (the pp_op records, the buffer table and its halos, the weight blob, the named buffers, the
per-op names and FLOPs and the parameter offsets), for each builder on seeded synthetic parameters at a small size, with the halo
layout on (POSEPIPE_CONV_HALO unset) and off ("0").  The table below was recorded on the commit before ProgramBuilder's op records
got their one constructor (ProgramBuilder._emit) by running `python -m tests.test_program_digests` there: a change to how the
builder writes a record, plans a halo or recycles a buffer shows up here as a changed digest.  After a change that MEANS to alter a
program, run the same command and paste its output over the table."""
import hashlib
import json

import numpy as np
import pytest

from posepipeline_amd.models import (dla, faster_rcnn, gastnet, higherhrnet, hrformer, hrnet, hrnetv2, mars, poseformer, reid_r50,
                                     synth, trades, vibe, videopose3d, vitpose, yolov4, yolox)
from posepipeline_amd.program import ProgramBuilder


def program_digest(prog):
    h = hashlib.sha256()
    for op in prog.ops:
        h.update(bytes(op))
    h.update(np.asarray(prog.bufs, np.int32).tobytes())
    h.update(np.asarray(prog.buf_pad or [0] * len(prog.bufs), np.int32).tobytes())
    h.update(np.ascontiguousarray(prog.blob, np.float32).tobytes())
    h.update(json.dumps([sorted(prog.named.items()), list(prog.op_names), sorted(prog.param_offsets.items())]).encode())
    h.update(np.asarray(list(prog.op_flops) + [prog.flops], np.float64).tobytes())
    return h.hexdigest()


def _yolov4():
    return yolov4.build_yolov4_program(yolov4.synth_params(yolov4.yolov4_param_shapes(num_classes=2), seed=0), size=64, num_classes=2)


def _hrnet():
    spec = hrnet.HRNetSpec(32, 17, 64, 64)
    return hrnet.build_hrnet_program(spec, synth.synth_state_dict(hrnet.hrnet_param_shapes(spec), seed=4))


def _videopose3d():
    spec = videopose3d.VideoPose3DSpec(channels=64)
    return videopose3d.build_videopose3d_program(spec, synth.synth_state_dict(videopose3d.videopose3d_param_shapes(spec), seed=5))


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _detector_sd():
    return _cached("detector", lambda: synth.synth_state_dict(faster_rcnn.faster_rcnn_param_shapes(), seed=2))


def _image():
    return faster_rcnn.build_image_program(_detector_sd(), 64, 96)


def _roi():
    return faster_rcnn.build_roi_program(_detector_sd())


def _hrnetv2():
    spec = hrnetv2.HRNetV2Spec(18, 21, 64, 96)
    return hrnetv2.build_hrnetv2_program(spec, synth.synth_state_dict(hrnetv2.hrnetv2_param_shapes(spec), seed=4))


def _hrformer():
    # tests/hrformer_ref.py's tiny_spec: every map needs window padding, and 6 -> 8 channel padding
    spec = hrformer.HRFormerSpec(channels=(6, 12, 24, 48), heads=(1, 2, 4, 8), in_h=96, in_w=64, stages=((1, 2), (1, 3), (1, 4)),
                                 blocks_per_branch=1)
    return hrformer.build_hrformer_program(spec, hrformer.synth_params(spec, seed=4))


def _yolox():
    return yolox.build_yolox_program(synth.synth_state_dict(yolox.yolox_param_shapes(), seed=6), 64, 96)


def _reid():
    return reid_r50.build_reid_program(synth.synth_state_dict(reid_r50.reid_param_shapes(), seed=3))


def _vibe_backbone():
    return vibe.build_backbone_program(synth.synth_state_dict(vibe.spin_param_shapes(), seed=31))


def _vibe_head():
    return vibe.build_head_program(vibe.synth_params(vibe.vibe_param_shapes(), seed=4))


def _mars():
    return mars.build_mars_program(yolov4.synth_params(mars.mars_param_shapes(), seed=1))


def _higherhrnet():
    spec = higherhrnet.HigherHRNetSpec(image_size=128, width=16)
    return higherhrnet.build_higherhrnet_program(spec, synth.synth_state_dict(higherhrnet.higherhrnet_param_shapes(spec), seed=2), 64, 128)


def _vitpose():
    spec = vitpose.VitPoseSpec(dim=128, depth=2, heads=2, mlp_ratio=4, num_joints=5, deconv=(32, 32))
    return vitpose.build_vitpose_program(spec, vitpose.synth_params(spec, seed=0))


def _dla34():
    return dla.build_dla34_program(dla.synth_dla34_state_dict(dla.dla34_param_shapes(), 11), 64, 96)


def _gastnet():
    spec = gastnet.GastNetSpec(channels=16, filter_widths=(3, 3, 3), chunk=8)
    return gastnet.build_gastnet_program(spec, gastnet.synth_params(gastnet.gastnet_param_shapes(spec), seed=3))


def _trades_sd():
    return _cached("trades", lambda: trades.synth_trades_state_dict(trades.trades_param_shapes(), 11))


def _trades_a():
    return trades.build_program_a(_trades_sd(), 64, 96)


def _trades_b():
    return trades.build_program_b(_trades_sd(), 16, 24)


def _poseformer():
    spec = poseformer.PoseFormerSpec()
    return poseformer.build_poseformer_program(spec, poseformer.synth_params(poseformer.poseformer_param_shapes(spec), seed=11))


BUILDERS = {
    "yolov4": _yolov4, "hrnet": _hrnet, "videopose3d": _videopose3d, "image": _image, "roi": _roi, "hrnetv2": _hrnetv2,
    "hrformer": _hrformer, "yolox": _yolox, "reid": _reid, "vibe_backbone": _vibe_backbone, "vibe_head": _vibe_head, "mars": _mars,
    "higherhrnet": _higherhrnet, "vitpose": _vitpose, "dla34": _dla34, "gastnet": _gastnet, "trades_a": _trades_a,
    "trades_b": _trades_b, "poseformer": _poseformer,
}

# name -> (digest with POSEPIPE_CONV_HALO unset, digest with POSEPIPE_CONV_HALO=0)
DIGESTS = {
    "yolov4": ("bafe6991e176c3d750ec244f4b9a387e1cbe389af00068f767ef4525582b7a00",
              "5678e939aaec912f950dfe44382332d2aaa49c4c567462f493bf79a15d29bc64"),
    "hrnet": ("98eedb530dae8dbda37c617333bd61f765ad9f44231b626358a0aed63e07aa88",
             "3e489e5451a8116f907a1e3fb8d7206c83288bc08c83cd6b553856c5764da14b"),
    "videopose3d": ("3dd9d53528e7fba9433f9459fee7566dfb79c646c006f1af03af7d9c8c1d8217",
                   "3dd9d53528e7fba9433f9459fee7566dfb79c646c006f1af03af7d9c8c1d8217"),
    "image": ("58dff209cc1824bd03ae2f8689a2732a20a32be9582e4750335e722d6b6dfe32",
             "a7ceac56ae0efe0f9b9179dca6a9f5f75db4485396069ce07585482c386e4e8b"),
    "roi": ("fbd34dd9e9cc8dd9d333649735cbd25e043a0ae108f54a6dca05af9067a7c6db",
           "fbd34dd9e9cc8dd9d333649735cbd25e043a0ae108f54a6dca05af9067a7c6db"),
    "hrnetv2": ("f849e6b2b1233eb716942cba9c490987489f3d710be5661ac1876f99e2f66f0d",
               "ceca95ff9e552d1ef15d6e1a7021cfe08fe6d57f0b0a0eb9237f6676ee8a4eed"),
    "hrformer": ("2b4ebcc7a14e16b64740514f1f6f51913801856e874a01191b3b1e015ae151de",
                "1adfbbd8e078df73d1171f28931dad7a725be9cce836c3756c270eec443c4a5f"),
    "yolox": ("5be891eef2d63a5b2f2a55e7f442db6c1a13adfa80037a9e6b5af91ad705883b",
             "9c92af937042b0a2dd6b61e9942ef3d1ae9a8e558e7315d4ce2acc4d075d6a29"),
    "reid": ("24ad12666fc3b87a746804acad36dd1bf4be45ef03a2a5a7c12cad1ac6240646",
            "f3ec1a8d185f787e4c6243a79df57709d7e5a3d979fa89ff188fdcef552f41e2"),
    "vibe_backbone": ("12b1916e418778c5caad558c28730e21f75fae3b1f78eedbda490915e3c7e1b2",
                     "31071de3eeb7e9a044d7b66515f3a8489897f86a50c37e0fec1599e13545bcca"),
    "vibe_head": ("188167da8924f0ff7b11e46c4e49e222a2ae947726b9f33f3bf5ddba7fe05e81",
                 "188167da8924f0ff7b11e46c4e49e222a2ae947726b9f33f3bf5ddba7fe05e81"),
    "mars": ("020a1e86ce08317550dd2a200b4a8786284228b902d29d33e0865fef1781283a",
            "5886ef73948d0a7fa9bba2d3960cad734e4b1cd962543528a20d32e6b51bbef8"),
    "higherhrnet": ("775e4d6ccd057c19b671e7d886945375a414516cfe8a4fe4bcffaa16c4c22a49",
                   "9a17df757e673d8cdd95c76ff0c5c74e1710396d2e225909c4ac8ecc3a070099"),
    "vitpose": ("ec0adae3d137ee644480b6fbd1f0377ee2dcca5b7034970707782f4109ae2276",
               "ec0adae3d137ee644480b6fbd1f0377ee2dcca5b7034970707782f4109ae2276"),
    "dla34": ("aa2065b299a503429012b11a149104e4b385ebb97a3fea7cd683d01349a4d838",
             "dc920f9d025f2cee10ef7b3042ae64214f60d56adec4874315e612b981dc003c"),
    "gastnet": ("1a217e0fb77174ef8b3fdabdf77ee25b6e1a14db1aa6782442039d2a5b67318c",
               "1a217e0fb77174ef8b3fdabdf77ee25b6e1a14db1aa6782442039d2a5b67318c"),
    "trades_a": ("09c2ae31fd92850fd9e2524fdccb34c48ffa699e9282944fd719e7f4444c5156",
                "aba176e92c0acd1a6eaa40258e64e75b6b9cb7693441a3eca99c7bda7ca38456"),
    "trades_b": ("c8f8356a7fcc05d4de2aef0583dfddcad2a389d8eb506311ad4335b043b910fb",
                "c8f8356a7fcc05d4de2aef0583dfddcad2a389d8eb506311ad4335b043b910fb"),
    "poseformer": ("3a70ba7c4a6a84bce590e8de7cefe2b40557af9d81f0ecefd939082b712a90d6",
                  "3a70ba7c4a6a84bce590e8de7cefe2b40557af9d81f0ecefd939082b712a90d6"),
}


def digests_of(name, monkeypatch_env):
    out = []
    for halo in (None, "0"):
        monkeypatch_env(halo)
        out.append(program_digest(BUILDERS[name]()))
    return tuple(out)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_program_unchanged(name, monkeypatch):
    def set_halo(value):
        if value is None:
            monkeypatch.delenv("POSEPIPE_CONV_HALO", raising=False)
        else:
            monkeypatch.setenv("POSEPIPE_CONV_HALO", value)
    assert digests_of(name, set_halo) == DIGESTS[name]


def test_table_covers_every_builder():
    assert set(DIGESTS) == set(BUILDERS)


def test_emit_refuses_a_key_that_is_no_pp_op_field():
    b = ProgramBuilder()
    x = b.buf(8, 8, 4, name="input")
    with pytest.raises(AssertionError, match="pad_hh"):
        b._emit(0, x, b.buf(8, 8, 4), name="bad", cin=4, cout=4, pad_hh=1)
    assert b.vops == []


if __name__ == "__main__":
    import os

    def _set(value):
        os.environ.pop("POSEPIPE_CONV_HALO", None)
        if value is not None:
            os.environ["POSEPIPE_CONV_HALO"] = value
    for _name in BUILDERS:
        _a, _b = digests_of(_name, _set)
        print(f'    "{_name}": ("{_a}",\n{" " * (8 + len(_name))}"{_b}"),')
