"""HRFormer-B (`method="HRFormer_COCO"`, TopDownMethodLookup row 3) without a device: the spec against the values of the config
the reference vendors, the parameter inventory against the published size, the reference's two attention forms against each
other, the full-size program, checkpoint extras and the table routing."""
import datetime
import json
import os

import numpy as np
import pytest
import torch

from posepipeline_amd import _lib as L
from posepipeline_amd.models import hrformer as M
from tests import hrformer_ref as R

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "arch_config_hrformer.json")))


def test_spec_equals_vendored_config():
    spec = M.hrformer_base_384x288()
    ex = GOLD["extra"]
    assert GOLD["backbone_type"] == "HRFormer" and ex["with_rpe"] is True
    s1 = ex["stage1"]
    assert (s1["block"], tuple(s1["num_blocks"]), tuple(s1["num_channels"])) == ("BOTTLENECK", (spec.layer1_blocks,), (64,))
    for si, (n_mod, n_br) in enumerate(spec.stages):
        st = ex[f"stage{si + 2}"]
        assert st["block"] == "HRFORMERBLOCK"
        assert (st["num_modules"], st["num_branches"]) == (n_mod, n_br)
        assert tuple(st["num_channels"]) == spec.channels[:n_br]
        assert tuple(st["num_heads"]) == spec.heads[:n_br]
        assert tuple(st["mlp_ratios"]) == spec.mlp_ratios[:n_br]
        assert tuple(st["window_sizes"]) == spec.windows[:n_br]
        assert tuple(st["num_blocks"]) == (spec.blocks_per_branch,) * n_br
    assert all(c // h == 39 for c, h in zip(spec.channels, spec.heads))
    head = GOLD["head"]
    assert head["type"] == "TopdownHeatmapSimpleHead" and head["num_deconv_layers"] == 0 and head["extra"] == {"final_conv_kernel": 1}
    sh = M.hrformer_param_shapes(spec)
    assert sh["keypoint_head.final_layer.weight"] == (head["out_channels"], head["in_channels"], 1, 1) == (17, 78, 1, 1)
    assert GOLD["image_size"] == [spec.in_w, spec.in_h] and GOLD["heatmap_size"] == list(spec.heatmap_hw[::-1])
    # crop and normalisation are W48's: the oracle's (and the wrappers') constants
    from oracle import preprocess as opre
    assert np.array_equal(np.asarray(GOLD["mean"], np.float32), opre.MEAN) and np.array_equal(np.asarray(GOLD["std"], np.float32), opre.STD)
    assert GOLD["val_pipeline_types"] == ["LoadImageFromFile", "TopDownGetBboxCenterScale", "TopDownAffine", "ToTensor",
                                          "NormalizeTensor", "Collect"] and GOLD["test_pipeline_is_val_pipeline"]


def test_topdown_settings_equal_test_cfg():
    from posepipeline_amd.models import hrnet
    from posepipeline_amd.wrappers import mmpose as wmm
    tc = GOLD["test_cfg"]
    s = wmm.topdown_settings("HRFormer_COCO")
    assert tc["flip_test"] is True and np.array_equal(s["flip_perm"], hrnet.flip_perm(17, hrnet.COCO_FLIP_PAIRS))
    assert (s["post"], s["shift_heatmap"], s["blur_kernel"], s["num_joints"]) == \
        (tc["post_process"], tc["shift_heatmap"], tc["modulate_kernel"], 17) == ("default", True, 17, 17)
    assert wmm._METHODS["HRFormer_COCO"][1] == "mmpose/checkpoints/hrformer_base_coco_384x288-ecf0758d_20220316.pth"


def test_parameter_count_matches_published_size():
    n = M.param_count(M.hrformer_param_shapes(M.hrformer_base_384x288()))
    print(f"HRFormer-B parameters (without BN running statistics and buffers): {n} = {n / 1e6:.3f} M (published: 43.2 M)")
    assert abs(n - 43.2e6) <= 0.01 * 43.2e6, n


@pytest.mark.parametrize("hw", [(7, 7), (9, 10), (12, 9), (3, 2)])
def test_reference_attention_forms_agree(hw):
    """pad / view / permute (mmpose) == the per-pixel closed form the kernel implements, with a non-zero qkv bias: padding
    before the Linear makes a padded token's k and v the bias, not zero"""
    h, w = hw
    c, heads, n = 12, 2, 2
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    wqkv = torch.randn(3 * c, c, generator=g, dtype=torch.float64) / np.sqrt(c)
    bqkv = torch.randn(3 * c, generator=g, dtype=torch.float64)
    table = torch.randn(169, heads, generator=g, dtype=torch.float64)
    a = R.attn_windows_mmpose(x, wqkv, bqkv, table, heads)
    b = R.attn_closed_form(x @ wqkv.T + bqkv, bqkv, table, heads)
    assert a.shape == b.shape == (n, h, w, c)
    assert (a - b).abs().max() <= 1e-13 * max(1.0, a.abs().max().item())
    if (h, w) != (7, 7):      # the bias matters wherever there is padding: zero keys instead give another result
        z = R.attn_closed_form(x @ wqkv.T + bqkv, torch.zeros_like(bqkv), table, heads)
        assert (a - z).abs().max() > 1e-3


def test_reference_dwconv_numpy_equals_torch():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (2, 7, 9, 8)).astype(np.float32)
    w = rng.normal(0, 0.3, (8, 1, 3, 3)).astype(np.float32)
    b = rng.normal(0, 0.1, 8).astype(np.float32)
    for stride in (1, 2):
        got = R.dwconv3x3_np(x, w, b, stride=stride)
        ref = R.dwconv3x3_t(torch.from_numpy(x).double(), torch.from_numpy(w), torch.from_numpy(b), stride=stride).numpy()
        assert got.shape == ref.shape == (2, (7 - 1) // stride + 1, (9 - 1) // stride + 1, 8)
        assert np.abs(got - ref).max() <= 1e-5


def test_full_size_program_builds_without_a_device():
    spec = M.hrformer_base_384x288()
    sd = M.synth_params(spec, seed=1)
    prog = M.build_hrformer_program(spec, sd)
    blocks = sum(n_mod * n_br * spec.blocks_per_branch for n_mod, n_br in spec.stages)
    kinds = [op.type for op in prog.ops]
    assert kinds.count(L.PP_OP_WINDOW_ATTN) == blocks == kinds.count(L.PP_OP_GELU_ADD) == 44
    assert kinds.count(L.PP_OP_LAYERNORM) == 2 * blocks
    assert kinds.count(L.PP_OP_DWCONV3X3) > blocks                       # + the strided fuse chains
    assert prog.bufs[prog.named["input"]] == (384, 288, 4) and prog.bufs[prog.named["output"]] == (96, 72, 17)
    assert all(b[2] % 4 == 0 for i, b in enumerate(prog.bufs) if i != prog.named["output"])
    assert 45e9 < prog.flops < 70e9, prog.flops                        # published: 26.8 GMACs at 384x288
    gelu_in = [op for op in prog.ops if op.type == L.PP_OP_DWCONV3X3 and op.pad_end == L.PP_DW_GELU_IN]
    assert len(gelu_in) == blocks and all(op.relu == L.PP_ACT_GELU and op.stride == 1 for op in gelu_in)
    assert all(op.relu <= L.PP_ACT_SWISH for op in prog.ops if op.type == L.PP_OP_CONV)       # no GELU in the convolution kernels
    # the bias tables are non-zero and asymmetric, the LayerNorm gains not all ones
    t = sd["backbone.stage2.0.branches.0.0.attn.attn.relative_position_bias_table"]
    assert t.shape == (169, 2) and np.abs(t).min() > 0 and not np.allclose(t, t[::-1])
    assert np.ptp(sd["backbone.stage2.0.branches.0.0.norm1.weight"]) > 0.1


def test_state_dict_with_extra_keys_loads():
    spec = R.tiny_spec()
    sd = M.synth_params(spec, seed=2)
    ref = M.build_hrformer_program(spec, sd)
    extra = dict(sd)
    p = "backbone.stage2.0.branches.0.0."
    extra[p + "attn.attn.relative_position_index"] = np.zeros((49, 49), np.int64)
    extra["backbone.bn1.num_batches_tracked"] = np.array(7, np.int64)
    extra[p + "ffn.layers.0.weight"] = sd[p + "ffn.fc1.weight"]
    extra[p + "ffn.layers.0.bias"] = sd[p + "ffn.fc1.bias"]
    prog = M.build_hrformer_program(spec, extra)
    assert np.array_equal(prog.blob, ref.blob) and len(prog.ops) == len(ref.ops)
    missing = {k: v for k, v in sd.items() if not k.endswith("relative_position_bias_table")}
    with pytest.raises(KeyError, match="relative_position_bias_table"):
        M.build_hrformer_program(spec, missing)


def test_table_routes_row_3_to_hrformer(monkeypatch, tmp_path):
    from posepipeline_amd import djshim, pipeline as pl, video
    from posepipeline_amd.wrappers import mmpose as wmm
    djshim.reset()
    assert (pl.TopDownMethodLookup & {"top_down_method": 3}).fetch1("top_down_method_name") == "MMPoseHrformerCoco"
    path = str(tmp_path / "v.ppvid")
    video.write_ppvid(path, np.zeros((5, 32, 48, 3), np.uint8), 30.0)
    vkey = {"video_project": "p", "filename": "hrformer"}
    pl.Video().insert1({**vkey, "video": path, "start_time": datetime.datetime(2024, 5, 1)})
    tracks = [[{"track_id": 1, "tlbr": np.array([1.0, 2, 11, 22]), "tlhw": np.array([1.0, 2, 10, 20]), "confidence": 0.9}]] * 5
    tkey = {**vkey, "tracking_method": 5}
    pl.TrackingBboxMethod().insert1(tkey)
    pl.TrackingBbox().insert1({**tkey, "tracks": tracks, "num_tracks": 1})
    pl.PersonBboxValid().insert1({**tkey, "video_subject_id": 0, "keep_tracks": [1]})
    pl.PersonBbox().populate(tkey)
    calls = []

    def fake(key, method="HRNet_W48_COCO"):
        calls.append(method)
        return np.full((5, 17, 3), 2.0)

    monkeypatch.setattr(wmm, "mmpose_top_down_person", fake)
    pkey = {**tkey, "video_subject_id": 0, "top_down_method": 3}
    pl.TopDownMethod().insert1(pkey)
    pl.TopDownPerson().populate(pkey)
    assert calls == ["HRFormer_COCO"]
    assert (pl.TopDownPerson & pkey).fetch1("keypoints").shape == (5, 17, 3)
    djshim.reset()
