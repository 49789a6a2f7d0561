"""pp_net_create's per-op checker, op type by op type: the smallest valid program of every type is accepted, and each of its
malformed variants is refused with a message that names the op's index and, where the checker words it, the op's kind.

Every program here is written by hand as two pp_op records: op 0 is a PP_OP_COPY between buffers 0 and 1 that has nothing to do
with the op under test, which is op 1 -- so a message must say "op 1".  Nothing is launched: creation fails in the checker before
any allocation, or allocates a few kilobytes (the ViT encoder and the bf16 deconvolution convert their zero weights)."""
import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.program import Net, Program

pytestmark = pytest.mark.gpu

NEUTRAL = dict(res1=-1, res2=-1, kh=1, kw=1, stride=1, dil_h=1, dil_w=1)
COPY_BUFS = [(8, 8, 4), (8, 8, 4)]


def vit_floats(tokens, dim, depth, hidden):
    per_block = 2 * dim + 3 * dim * dim + 3 * dim + dim * dim + dim + 2 * dim + hidden * dim + hidden + dim * hidden + dim
    return tokens * dim + per_block * depth + 2 * dim


class Case:
    """bufs: the buffers behind the two of op 0 (ids 2, 3, ...: in_ is 2 and out is 3 everywhere); fields: op 1's record;
    kind: what the checker's own messages call the op (None: they do not name it); shape: a substring of the message for an
    out buffer of the wrong shape; no_res: the residual field the checker refuses for this type (None: it looks at neither)"""

    def __init__(self, type_, bufs, *, kind, shape=None, blob=64, takes=0, needs=0, no_res=None, params=None, **fields):
        self.type, self.bufs, self.kind, self.shape, self.blob = type_, bufs, kind, shape or kind, blob
        self.takes, self.needs, self.no_res, self.params = takes, needs, no_res, params
        self.fields = {**NEUTRAL, "in_": 2, "out": 3, **fields}

    def program(self, bufs=None, pads=None, **changed):
        ops = [L.pp_op(type=L.PP_OP_COPY, in_=0, out=1, cin=4, cout=4, **NEUTRAL), L.pp_op(type=self.type, **{**self.fields, **changed})]
        bufs = COPY_BUFS + list(self.bufs if bufs is None else bufs)
        return Program(ops=ops, bufs=bufs, buf_pad=pads or [0] * len(bufs), blob=np.zeros(self.blob, np.float32))


CASES = {
    "conv": Case(L.PP_OP_CONV, [(8, 8, 4), (8, 8, 8)], kind=None, shape="does not match out buffer", blob=1024, params="out of blob",
                 cin=4, cout=8, w_off=0, b_off=512),
    "maxpool": Case(L.PP_OP_MAXPOOL, [(8, 8, 4), (4, 4, 4)], kind="maxpool", cin=4, cout=4, kh=2, kw=2, stride=2),
    "avgpool": Case(L.PP_OP_AVGPOOL, [(8, 8, 4), (1, 1, 4)], kind="avgpool", cin=4, cout=4, kh=8, kw=8),
    "copy": Case(L.PP_OP_COPY, [(8, 8, 4), (8, 8, 4)], kind="copy", cin=4, cout=4),
    "depth_to_space": Case(L.PP_OP_DEPTH_TO_SPACE, [(8, 8, 16), (16, 16, 4)], kind="depth_to_space", cin=16, cout=4),
    "deconv_bf16": Case(L.PP_OP_DECONV_BF16, [(8, 8, 64), (16, 16, 8)], kind="deconv_bf16", blob=8192 + 8, params="parameters out of blob",
                        cin=64, cout=8, kh=4, kw=4, stride=2, pad_h=1, pad_w=1, w_off=0, b_off=8192),
    "upsample_add": Case(L.PP_OP_UPSAMPLE_ADD, [(4, 4, 4), (8, 8, 4), (8, 8, 4)], kind="upsample_add", takes=2, cin=4, cout=4, up_log2=1),
    "bilinear_add": Case(L.PP_OP_BILINEAR_ADD, [(4, 4, 4), (8, 8, 4), (8, 8, 4)], kind="bilinear_add", takes=2, no_res="res2",
                         cin=4, cout=4, up_log2=1),
    "dwconv3x3": Case(L.PP_OP_DWCONV3X3, [(8, 8, 4), (8, 8, 4), (8, 8, 4)], kind="dwconv3x3", no_res="res1", params="parameters out of blob",
                      cin=4, cout=4, kh=3, kw=3, pad_h=1, pad_w=1, w_off=0, b_off=36),
    "layernorm": Case(L.PP_OP_LAYERNORM, [(8, 8, 4), (8, 8, 4), (8, 8, 4)], kind="layernorm", no_res="res1", params="parameters out of blob",
                      cin=4, cout=4, w_off=0, b_off=4),
    "window_attn": Case(L.PP_OP_WINDOW_ATTN, [(7, 7, 12), (7, 7, 4), (7, 7, 4)], kind="window_attn", no_res="res1", blob=256,
                        params="parameters out of blob", cin=4, cout=4, kh=7, kw=7, w_off=0, b_off=172),
    "attention": Case(L.PP_OP_ATTENTION, [(8, 8, 12), (8, 8, 4), (8, 8, 4)], kind="attention", no_res="res1", cin=4, cout=4),
    "gelu_add": Case(L.PP_OP_GELU_ADD, [(8, 8, 4), (8, 8, 4), (8, 8, 4)], kind="gelu_add", no_res="res2", cin=4, cout=4),
    "dcn3x3": Case(L.PP_OP_DCN3X3, [(8, 8, 4), (8, 8, 4), (8, 8, 28)], kind="dcn3x3", takes=1, needs=1, no_res="res1", blob=9216 + 32,
                   params="parameters out of blob", cin=4, cout=4, kh=3, kw=3, pad_h=1, pad_w=1, in2=4, w_off=0, b_off=9216),
    "dwdeconv": Case(L.PP_OP_DWDECONV, [(4, 4, 4), (8, 8, 4), (8, 8, 4)], kind="dwdeconv", no_res="res2", params="parameters out of blob",
                     cin=4, cout=4, kh=4, kw=4, stride=2, pad_h=1, pad_w=1, w_off=0),
    # (the three elementwise ops of TraDeS share their messages, which name the kinds only where they differ)
    "sub_cat": Case(L.PP_OP_SUB_CAT, [(8, 8, 4), (8, 8, 8), (8, 8, 4), (8, 8, 1)], kind=None, shape="distinct out", takes=1, needs=1,
                    no_res="res2", cin=4, cout=8, res1=4, in2=5),
    "bcast_mul": Case(L.PP_OP_BCAST_MUL, [(8, 8, 4), (8, 8, 4), (8, 8, 4), (8, 8, 1)], kind=None, shape="distinct out", takes=1, needs=1,
                      no_res="res1", cin=4, cout=4, in2=5),
    "blend2": Case(L.PP_OP_BLEND2, [(8, 8, 4), (8, 8, 4), (8, 8, 4), (8, 8, 1), (8, 8, 1)], kind=None, shape="distinct out", takes=2,
                   needs=2, no_res="res2", cin=4, cout=4, res1=4, in2=5, in3=6),
    "graph_mix": Case(L.PP_OP_GRAPH_MIX, [(17, 8, 8), (17, 8, 4), (17, 8, 4)], kind="graph_mix", no_res="res1", blob=1156 + 24,
                      params="parameters out of blob", cin=8, cout=4, w_off=0, b_off=1156),
    "joint_attn": Case(L.PP_OP_JOINT_ATTN, [(17, 8, 12), (17, 8, 4), (17, 8, 4)], kind="joint_attn", no_res="res1", cin=4, cout=4),
    # (the encoder's attention kernel is built for 192 tokens: the smallest map pp_vit_encoder_create takes is 16x12 at dim 128)
    "vit_encoder": Case(L.PP_OP_VIT_ENCODER, [(16, 12, 128), (16, 12, 128)], kind="vit encoder", blob=(vit_floats(192, 128, 1, 128) + 3) // 4 * 4,
                        params="parameters out of blob", cin=128, cout=128, kh=1, kw=2, w_off=0),
}


def refused(ctx, prog, *substrings):
    with pytest.raises(L.PosePipeHipError) as e:
        Net(ctx, prog, max_batch=1).close()
    msg = str(e.value)
    assert "op 1:" in msg, msg
    for s in substrings:
        if s:
            assert s in msg, (s, msg)


def test_every_op_type_has_a_case():
    have = {c.type for c in CASES.values()}
    want = {v for k, v in vars(L).items() if k.startswith("PP_OP_")} - {L.PP_OP_ROIALIGN}      # (no layer-program op: the detector's own kernel)
    assert have == want


@pytest.mark.parametrize("name", sorted(CASES))
def test_valid_program_is_accepted(ctx, name):
    net = Net(ctx, CASES[name].program(), max_batch=1)
    assert net.handle
    net.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_out_buffer_of_the_wrong_shape(ctx, name):
    c = CASES[name]
    bufs = list(c.bufs)
    bufs[1] = (bufs[1][0] + 1, bufs[1][1], bufs[1][2])
    refused(ctx, c.program(bufs=bufs), c.kind, c.shape)


@pytest.mark.parametrize("name", sorted(CASES))
def test_in2_in3_only_where_the_op_takes_them(ctx, name):
    c = CASES[name]
    if c.takes == 0:
        refused(ctx, c.program(in2=2), "in2 / in3")
    if c.takes <= 1:
        refused(ctx, c.program(in3=2), "in2 / in3")
    if c.takes == 2 and c.needs == 0:       # the optional pair of the two fuse ops: in3 only behind in2
        refused(ctx, c.program(in2=-1, in3=2), "in3 without in2")


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.needs))
def test_missing_required_in2(ctx, name):
    c = CASES[name]
    refused(ctx, c.program(in2=-1), c.kind, "in2")
    if c.needs == 2:
        refused(ctx, c.program(in3=-1), "in3")


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.no_res))
def test_residual_on_an_op_that_has_none(ctx, name):
    c = CASES[name]
    refused(ctx, c.program(**{c.no_res: 4}), c.kind, "no " if c.kind else "res")


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.params))
def test_w_off_past_the_blob(ctx, name):
    c = CASES[name]
    refused(ctx, c.program(w_off=c.blob), c.kind, c.params)
    refused(ctx, c.program(w_off=-4), c.kind, c.params)


@pytest.mark.parametrize("name", sorted(set(CASES) - {"conv"}))
def test_only_convolutions_read_a_halo_buffer(ctx, name):
    c = CASES[name]
    pads = [0] * (2 + len(c.bufs))
    pads[2] = 1
    refused(ctx, c.program(pads=pads), "zero halo", "buffer 2")


def test_convolution_may_read_a_halo_buffer(ctx):
    c = CASES["conv"]
    Net(ctx, c.program(pads=[0, 0, 1, 0]), max_batch=1).close()


def test_unsupported_op_type(ctx):
    prog = CASES["copy"].program()
    prog.ops[1].type = 99
    refused(ctx, prog, "unsupported op type 99")
    prog.ops[1].type = L.PP_OP_ROIALIGN
    refused(ctx, prog, "unsupported op type")


@pytest.mark.parametrize("field", ["in_", "out", "res1", "res2", "in2", "in3"])
def test_buffer_id_out_of_range(ctx, field):
    c = CASES["upsample_add"]
    # (in2 / in3 share one condition, and one message, with the rule about which ops take them)
    refused(ctx, c.program(**{field: 2 + len(c.bufs)}), "in2 / in3" if field in ("in2", "in3") else "out of range")
    if field in ("in_", "out"):
        refused(ctx, c.program(**{field: -1}), "out of range")
