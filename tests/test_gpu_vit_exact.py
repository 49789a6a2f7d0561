"""ViTPose path (gemm_bf16.hip, vit_encoder.hip, deconv_bf16.hip): data movement settled with `==`, arithmetic with derived bounds.

Fragment mappings, swizzles, tile edges and scatter addresses are questions of WHICH value lands WHERE.  With integer-valued
operands whose partial sums are all exact in float32 (|sum| < 2^24) every summation order gives the same bits, so the
accumulation order of the bf16 MFMA (which the ISA does not architect) drops out and the kernels are compared with exact integer
arithmetic by `np.array_equal`: float32 outputs are the integer itself, bf16 outputs are one RNE rounding of it.

Where a result cannot be exact (GELU, LayerNorm, the whole encoder) the bound is derived from the kernel's stated contract or
measured from the reference alone inside the test -- never from what the kernel gives.  Every CPU precondition (score margins,
closed forms) is asserted before the GPU is used.

Sections: 1 GEMM (every epilogue x every tile configuration, in-place residual, M below one tile), 2 attention (one-hot,
uniform, half-and-half softmax), 3 the encoder alone (zero matrices, documented bit-identities, accuracy against the oracle),
4 LayerNorm edges, 5 PP_OP_DECONV_BF16, 6 pp_f32_to_bf16.
"""
import functools

import numpy as np
import pytest

from oracle import vit as OV
from posepipeline_amd import _lib as L
from posepipeline_amd.models import vitpose as MV
from posepipeline_amd.program import Net, ProgramBuilder
from tests.test_gpu_vit import Dev, _close_bf16

pytestmark = pytest.mark.gpu

F32 = np.float32
T = 192                                                      # tokens of the 256 x 192 crop: the attention kernels' only length


def _set_cfg(monkeypatch, cfg):
    if cfg:
        monkeypatch.setenv("POSEPIPE_GEMM_CFG", cfg)
    else:
        monkeypatch.delenv("POSEPIPE_GEMM_CFG", raising=False)


# ---- 1. bf16 GEMM, integer-exact --------------------------------------------------------------------------------------------
CFGS = ["", "0", "1", "2", "10"]                             # the default selection and every tile configuration
GEMM_M = [1, 7, 129, 192, 300, 576, 1100]                    # below one 128-row group, below one tile (192 = the encoder at batch 1), ragged
GEMM_NK = [(128, 64), (384, 192), (256, 128), (768, 256), (1280, 5120), (3840, 1280)]     # the last four take the ping-pong form
RES_KINDS = ["none", "sep", "mod192", "inplace"]
# (bias, residual form, bf16 output); in place (C == res) exists for float32 only: the residual stream is float32
EPILOGUES = [(ub, rk, ob) for ub in (1, 0) for rk in RES_KINDS for ob in (0, 1) if not (rk == "inplace" and ob)]
# the grid is pruned, not crossed: every epilogue once, the M and (N, K) values dealt round-robin ...
GEMM_CASES = [(GEMM_M[i % 7],) + GEMM_NK[i % 6] + EPILOGUES[i] for i in range(len(EPILOGUES))]
# ... plus, on EVERY M x (N, K), the two forms nothing ran before: a residual with a bf16 output (a branch of its own in the
# ping-pong epilogue) and the in-place residual stream (proj / fc2 of the encoder; 192 x 3840 x 1280 is its batch-1 shape) ...
GEMM_CASES += [(m, n, k, 1, rk, ob) for m in GEMM_M for n, k in GEMM_NK for rk, ob in (("sep", 1), ("inplace", 0))]
# ... and the row % 192 broadcast with a bf16 output / no bias on ping-pong shapes with a ragged last tile
GEMM_CASES += [(300, 768, 256, 1, "mod192", 1), (1100, 3840, 1280, 0, "mod192", 1), (1, 768, 256, 0, "sep", 1)]
GEMM_CASES = list(dict.fromkeys(GEMM_CASES))
# every value of every axis appears (and every case runs under every configuration)
assert {c[0] for c in GEMM_CASES} == set(GEMM_M) and {c[1:3] for c in GEMM_CASES} == set(GEMM_NK)
assert {c[3:] for c in GEMM_CASES} == set(EPILOGUES) and len(EPILOGUES) == 14


@functools.lru_cache(maxsize=4)                                 # the configurations of a case run back to back
def _gemm_operands(m, n, k, res_kind):
    """Seeded integer operands and the exact product.  |a w| <= 16 per term and K <= 5120: every partial sum, with the bias
    (<= 64) and the residual (<= 1000) added at any point, stays below 2^24 in magnitude -- exact in float32 in any order."""
    rng = np.random.default_rng([m, n, k, RES_KINDS.index(res_kind)])
    a = rng.integers(-4, 5, (m, k))
    w = rng.integers(-4, 5, (n, k))
    bias = rng.integers(-64, 65, n)
    res = rng.integers(-1000, 1001, (T if res_kind == "mod192" else m, n))
    # float64 holds these integers and all their sums exactly (16 K < 2^53), so the BLAS product IS the int64 product ...
    prod = a.astype(np.float64) @ w.astype(np.float64).T
    acc = prod.astype(np.int64)
    assert np.array_equal(acc, prod)
    rows = np.unique(np.array([0, m // 2, m - 1]))
    assert np.array_equal(acc[rows], a[rows].astype(np.int64) @ w.astype(np.int64).T)      # ... checked on three rows
    assert 16 * k + 64 + 1000 < 2 ** 24
    return a, w, bias, res, acc


def _run_gemm(ctx, a, w, bias, res, res_kind, act, out_bf16):
    """pp_gemm_bf16 on operand arrays that are exact in bf16; returns the raw output (float32 or bf16 bits)"""
    m, k = a.shape
    n = w.shape[0]
    for arr in (a, w):
        assert np.array_equal(OV.bf16_round(arr.astype(F32)), arr)
    da, dw = Dev(ctx, OV.bf16_bits(a.astype(F32))), Dev(ctx, OV.bf16_bits(w.astype(F32)))
    db = Dev(ctx, bias.astype(F32)) if bias is not None else None
    devs = [da, dw] + ([db] if db else [])
    if res_kind == "inplace":
        assert not out_bf16
        dc = Dev(ctx, res.astype(F32))                           # the residual IS the output buffer (C == res)
        res_ptr, res_mod = dc.ptr, 0
    else:
        dc = Dev(ctx, nbytes=m * n * (2 if out_bf16 else 4))
        ctx.h2d(dc.ptr, np.full(m * n * (1 if out_bf16 else 2), 0x7fc1, np.uint16))     # NaN fill: a row left unwritten shows
        dres = Dev(ctx, res.astype(F32)) if res_kind != "none" else None
        devs += [dres] if dres else []
        res_ptr, res_mod = (dres.ptr if dres else None), (T if res_kind == "mod192" else 0)
    devs.append(dc)
    L.check(ctx.lib.pp_gemm_bf16(ctx.handle, da.ptr, dw.ptr, db.ptr if db else None, res_ptr, res_mod, dc.ptr, m, n, k,
                                 act, out_bf16), "pp_gemm_bf16")
    ctx.synchronize()
    got = dc.get((m, n), np.uint16 if out_bf16 else F32)
    for d in devs:
        d.free()
    return got


def _res_rows(res, res_kind, m):
    return res[np.arange(m) % T] if res_kind == "mod192" else res


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("m,n,k,use_bias,res_kind,out_bf16", GEMM_CASES)
def test_gemm_bf16_integer_exact(ctx, monkeypatch, cfg, m, n, k, use_bias, res_kind, out_bf16):
    """C = A W^T (+ bias) (+ residual: separate, broadcast over row % 192, or in place) on integers: float32 outputs equal the
    int64 result, bf16 outputs equal its one RNE rounding, bit for bit, in every tile configuration."""
    _set_cfg(monkeypatch, cfg)
    a, w, bias, res, acc = _gemm_operands(m, n, k, res_kind)
    ref = acc.copy()
    if use_bias:
        ref += bias
    if res_kind != "none":
        ref += _res_rows(res, res_kind, m)
    assert np.abs(ref).max() < 2 ** 24
    ref32 = ref.astype(F32)
    assert np.array_equal(ref32.astype(np.int64), ref)
    got = _run_gemm(ctx, a, w, bias if use_bias else None, res, res_kind, 0, out_bf16)
    if out_bf16:
        want = OV.bf16_bits(ref32)
        assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    else:
        assert np.array_equal(got, ref32), (int((got != ref32).sum()), np.argwhere(got != ref32)[:4].tolist())


GELU_CASES = [(300, 768, 256, 1, "none"), (576, 1280, 5120, 0, "none"), (192, 384, 192, 1, "sep"), (129, 256, 128, 1, "sep")]


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("m,n,k,use_bias,res_kind", GELU_CASES)
def test_gemm_bf16_gelu_f32(ctx, monkeypatch, cfg, m, n, k, use_bias, res_kind):
    """GELU with a float32 output: the erf approximation seen directly, not through a bf16 rounding.  Same integer operands with
    W (and the bias) scaled by 2^-s, exact in bf16 / float32, so the pre-activation v is exact and the error is the activation's.

    Bound |got - ref| <= 0.5 |v| 3e-7 + 2^-22 |ref|, from the kernel's own contract: gelu = 0.5 v (1 + erf), the kernel documents
    |erf error| <= 1.5e-7 (Abramowitz-Stegun 7.1.26); the same again is allowed for its 1-ulp rcp and exp2; 2^-22 |ref| is
    four float32 half-ulps for the roundings of (1 + erf), of the product and of the residual add.  The reference is OV.gelu's
    formula kept in float64."""
    _set_cfg(monkeypatch, cfg)
    a, w, bias, res, acc = _gemm_operands(m, n, k, res_kind)
    s = int(round(np.log2((80.0 / 12.0) * np.sqrt(k) / 3.0)))                  # operand variance 80 / 12 each: std(v) ~ 3
    scale = 2.0 ** -s
    v = (acc + (bias if use_bias else 0)) * scale                              # exact: an integer < 2^24 times a power of two
    assert v.min() <= -8 and v.max() >= 8, (v.min(), v.max())                  # the pre-activations cover [-8, 8]
    ref = 0.5 * v * (1.0 + OV.erf(v / np.sqrt(2.0)))
    if res_kind != "none":
        ref = ref + _res_rows(res, res_kind, m)
    got = _run_gemm(ctx, a, w * scale, bias * scale if use_bias else None, res, res_kind, 1, 0).astype(np.float64)
    err = np.abs(got - ref)
    bound = 0.5 * np.abs(v) * 3e-7 + 2.0 ** -22 * np.abs(ref)
    i = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"gelu f32 cfg={cfg!r} {m}x{n}x{k}: max err {err.max():.3e}; worst err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f} "
          f"at v = {v[i]:.4f} (err {err[i]:.3e}, bound {bound[i]:.3e})")
    assert (err <= bound).all(), (int((err > bound).sum()), float(v[i]), float(err[i]), float(bound[i]))


# ---- 2. attention, exact cases ---------------------------------------------------------------------------------------------
ATT_SHAPES = [(8, 80), (4, 64), (16, 80), (1, 64)]
ATT_BATCH = [1, 3, 40]                                       # 40 x 16 heads = 640 workgroups: more than one wave of blocks on the chip


def _pack_qkv(q, k, v):
    """[b][h][t][hd] each -> the packed ABI layout [b * t][3][h][hd]"""
    b, h, t, hd = q.shape
    x = np.stack([q, k, v], 0).astype(F32)                   # [3][b][h][t][hd]
    x = np.ascontiguousarray(np.transpose(x, (1, 3, 0, 2, 4))).reshape(b * t, 3 * h * hd)
    assert np.array_equal(OV.bf16_round(x), x), "operands must be exact in bf16"
    return x


def _heads_first(o, b, h, hd):
    """[b * t][h * hd] -> [b][h][t][hd]"""
    return np.transpose(o.reshape(b, T, h, hd), (0, 2, 1, 3))


def _oracle_attention_bits(qkv, batch, heads):
    """OV.attention (float32 result) rounded to bf16, eight samples at a time"""
    o = np.concatenate([OV.attention(qkv[s * T:(s + 8) * T], min(8, batch - s), T, heads, True) for s in range(0, batch, 8)])
    return OV.bf16_bits(o)


def _gpu_attention_bits(ctx, qkv, batch, heads, hd):
    dq = Dev(ctx, OV.bf16_bits(qkv))
    do = Dev(ctx, nbytes=batch * T * heads * hd * 2)
    ctx.h2d(do.ptr, np.full(batch * T * heads * hd, 0x7fc1, np.uint16))
    L.check(ctx.lib.pp_attention_bf16(ctx.handle, dq.ptr, batch, T, heads, hd, do.ptr), "pp_attention_bf16")
    ctx.synchronize()
    got = do.get((batch * T, heads * hd), np.uint16)
    dq.free(); do.free()
    return got


def _mean_bits(sum_v, count):
    """the kernel's last step on an exact integer sum: bf16_rne(float32(sum) * (float32(1) / float32(count)))"""
    assert np.abs(sum_v).max() < 2 ** 24
    return OV.bf16_bits(sum_v.astype(F32) * (F32(1) / F32(count)))


@pytest.mark.parametrize("batch", ATT_BATCH)
@pytest.mark.parametrize("heads,hd", ATT_SHAPES)
def test_attention_one_hot(ctx, heads, hd, batch):
    """Keys are distinct +-1 vectors and query i is 64 x key pi(i), with a permutation pi of its own per (sample, head): the
    top score leads by > 110 after the 1 / sqrt(hd) scale, every other numerator underflows to 0 and out[i] == v[pi(i)] bit
    for bit.  A key slot that S^T and the V^T read disagree on, or a wrong (sample, head) address, moves a row."""
    rng = np.random.default_rng([1, heads, hd, batch])
    k = rng.choice(np.array([-1.0, 1.0], F32), (batch, heads, T, hd))
    pi = rng.permuted(np.tile(np.arange(T), (batch, heads, 1)), axis=-1)
    q = 64 * np.take_along_axis(k, pi[..., None], axis=2)
    v = OV.bf16_round(100 * rng.standard_normal((batch, heads, T, hd), dtype=F32))
    v[v == 0] = 1                                            # -0 + 0 = +0: a signed zero does not survive the sum over the keys
    s = q @ np.transpose(k, (0, 1, 3, 2))                    # integers <= 64 hd: exact in float32
    assert np.array_equal(s.argmax(-1), pi)
    top2 = np.partition(s, -2, axis=-1)[..., -2:]
    margin = (top2[..., 1] - top2[..., 0]).astype(np.float64) / np.sqrt(hd)
    assert margin.min() > 110, margin.min()                  # e^-110 < 2^-149: below the smallest float32 subnormal
    want = OV.bf16_bits(np.take_along_axis(v, pi[..., None], axis=2))
    qkv = _pack_qkv(q, k, v)
    assert np.array_equal(_heads_first(_oracle_attention_bits(qkv, batch, heads), batch, heads, hd), want)
    got = _heads_first(_gpu_attention_bits(ctx, qkv, batch, heads, hd), batch, heads, hd)
    assert np.array_equal(got, want), (int((got != want).any(-1).sum()), np.argwhere((got != want).any(-1))[:4].tolist())


@pytest.mark.parametrize("batch", ATT_BATCH)
@pytest.mark.parametrize("heads,hd", ATT_SHAPES)
def test_attention_uniform(ctx, heads, hd, batch):
    """q = 0: every numerator is exactly 1, the denominator 192, and with integer v the output is
    bf16_rne(float32(sum_v) * (float32(1) / float32(192))) -- the kernel's own last step (no fast-math, no contraction), so
    bit-equal: each of the 192 keys counts exactly once."""
    rng = np.random.default_rng([2, heads, hd, batch])
    q = np.zeros((batch, heads, T, hd), F32)
    k = OV.bf16_round(rng.standard_normal((batch, heads, T, hd), dtype=F32))
    v = rng.integers(-8, 9, (batch, heads, T, hd))
    want = np.broadcast_to(_mean_bits(v.sum(2), T)[:, :, None, :], v.shape)
    qkv = _pack_qkv(q, k, v)
    assert np.array_equal(_heads_first(_oracle_attention_bits(qkv, batch, heads), batch, heads, hd), want)
    got = _heads_first(_gpu_attention_bits(ctx, qkv, batch, heads, hd), batch, heads, hd)
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("batch", ATT_BATCH)
@pytest.mark.parametrize("heads,hd", ATT_SHAPES)
def test_attention_half_and_half(ctx, heads, hd, batch):
    """k_j = +a for tokens j < 96 and -a for the rest (one +-1 vector a per (sample, head)), q_i = 16 k_i: a query sees exactly
    the 96 keys of its own half (score margin 32 sqrt(hd) >= 256, the other numerators are 0), so the output is the exact mean
    of its half's integer v.  A kb step that is skipped or counted twice, or a numerator paired with a v of the other half,
    changes a sum; a permutation of keys inside one 32-key step does not (96 = 3 x 32) -- the one-hot case sees that."""
    rng = np.random.default_rng([3, heads, hd, batch])
    a = rng.choice(np.array([-1.0, 1.0], F32), (batch, heads, 1, hd))
    sign = np.where(np.arange(T) < T // 2, F32(1), F32(-1))
    k = a * sign[None, None, :, None]
    q = 16 * k
    v = rng.integers(-8, 9, (batch, heads, T, hd))
    s = q @ np.transpose(k, (0, 1, 3, 2))
    own = np.broadcast_to(sign[:, None] * sign[None, :] > 0, s.shape)           # query and key in the same half
    assert (s[own] == 16 * hd).all() and (s[~own] == -16 * hd).all()
    assert 32 * hd / np.sqrt(hd) >= 256
    half = np.stack([v[:, :, :T // 2].sum(2), v[:, :, T // 2:].sum(2)], 2)      # [b][h][2][hd]
    want = np.repeat(_mean_bits(half, T // 2), T // 2, axis=2)
    qkv = _pack_qkv(q, k, v)
    assert np.array_equal(_heads_first(_oracle_attention_bits(qkv, batch, heads), batch, heads, hd), want)
    got = _heads_first(_gpu_attention_bits(ctx, qkv, batch, heads, hd), batch, heads, hd)
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


# ---- 3. the encoder alone ------------------------------------------------------------------------------------------------
ENC_SPECS = {
    # hd 64; every GEMM, the qkv GEMM included, is eligible for the ping-pong form (N % 256 == 0, K % 128 == 0)
    "dim256": MV.VitPoseSpec(dim=256, depth=2, heads=4, mlp_ratio=4, deconv=(64, 64)),
    # hd 80; qkv (N = 1920), proj and fc2 (K or N = 640) take configurations 0 .. 2, fc1 (N = 2560, K = 640) the ping-pong form
    "dim640": MV.VitPoseSpec(dim=640, depth=2, heads=8, mlp_ratio=4, deconv=(64, 64)),
}
ENC_BATCHES = (1, 3, 5)                                      # M = 192, 576, 960: rows cross sample boundaries inside 128-row groups


class _Encoder:
    """a program of one [16][12][dim] input buffer and the encoder op"""

    def __init__(self, ctx, spec, p, max_batch=5):
        b = ProgramBuilder()
        gh, gw = spec.grid
        assert gh * gw == T
        x = b.buf(gh, gw, spec.dim, name="input")
        b.vit_encoder(x, MV.encoder_param_block(p, spec), depth=spec.depth, heads=spec.heads, mlp_ratio=spec.mlp_ratio)
        self.ctx, self.spec, self.prog = ctx, spec, b.build()
        self.net = Net(ctx, self.prog, max_batch)

    def __call__(self, tok):
        n = tok.shape[0]
        dptr, nbytes, _ = self.net.buffer("input")
        assert nbytes == T * self.spec.dim * 4 and tok.shape[1:] == (T, self.spec.dim) and tok.dtype == F32
        self.ctx.h2d(dptr, tok)
        self.net.run(n)
        self.ctx.synchronize()
        return self.net.read(self.prog.ops[0].out, n).reshape(n, T, self.spec.dim)

    def close(self):
        self.net.close()


def _tokens(spec, n, seed):
    return np.random.default_rng(seed).standard_normal((n, T, spec.dim), dtype=F32)        # every sample different


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("name", list(ENC_SPECS))
def test_encoder_zero_matrices(ctx, monkeypatch, name, cfg):
    """All four weight matrices of every block are zero: every GEMM returns its bias and the residual stream before the last
    LayerNorm is (((tok + pos) + bproj_0) + b2_0) + ..., every addition in float32 -- known bit for bit, so the output is checked
    against the float64 LayerNorm of that array at float32 precision (test_layernorm's rtol 1e-5 / atol 2e-5).  This sees the
    row % pos_mod broadcast of the position embedding, the x_out write-back, the in-place residual of every GEMM configuration
    and the ping-pong form's "bias first" at 1e-5 instead of through 5e-3 of a heat-map."""
    spec = ENC_SPECS[name]
    p = MV.synth_params(spec, seed=21)
    for i in range(spec.depth):
        for w in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"):
            p[f"backbone.blocks.{i}.{w}.weight"][...] = 0
    pos = p["backbone.pos_embed"][0]
    pos = (pos[1:] + pos[:1]).astype(F32)
    tok = _tokens(spec, 5, 31)
    x = tok + pos[None]
    for i in range(spec.depth):
        x = x + p[f"backbone.blocks.{i}.attn.proj.bias"]
        x = x + p[f"backbone.blocks.{i}.mlp.fc2.bias"]
    assert x.dtype == F32
    ref = OV.layernorm(x, p["backbone.last_norm.weight"], p["backbone.last_norm.bias"])
    assert np.array_equal(OV.encoder(tok[:3], p, spec, True), ref[:3])          # the oracle agrees with the closed form exactly
    assert not np.array_equal(ref[0], ref[1])
    _set_cfg(monkeypatch, cfg)
    enc = _Encoder(ctx, spec, p)
    for n in ENC_BATCHES:
        np.testing.assert_allclose(enc(tok[:n]), ref[:n], rtol=1e-5, atol=2e-5)
    enc.close()


@pytest.mark.parametrize("name", list(ENC_SPECS))
def test_encoder_documented_bit_identities(ctx, monkeypatch, name):
    """What the code documents as the same arithmetic on the same values, on random parameters, batch 1 / 3 / 5:
      * POSEPIPE_VIT_HEAD_MAJOR=1 equals 0 under each of POSEPIPE_GEMM_CFG "", "0", "2", "10" -- on dim 256 the qkv GEMM takes
        the ping-pong form's head-major epilogue, rows crossing a sample boundary inside a 128-row group included;
      * tile configurations 0, 1 and 2 equal each other (gemm_bf16.hip, "0 .. 2 are bit-identical");
      * sample i of a batch of 5 equals the same sample run alone, in a batch of 3 and at another batch position."""
    spec = ENC_SPECS[name]
    p = MV.synth_params(spec, seed=22)
    tok = _tokens(spec, 5, 32)
    out = {}
    for hm in ("0", "1"):
        monkeypatch.setenv("POSEPIPE_VIT_HEAD_MAJOR", hm)    # read when the encoder is created
        enc = _Encoder(ctx, spec, p)
        for cfg in ("", "0", "1", "2", "10"):
            _set_cfg(monkeypatch, cfg)
            for n in ENC_BATCHES:
                out[hm, cfg, n] = enc(tok[:n])
        _set_cfg(monkeypatch, "")
        out[hm, "alone"] = np.concatenate([enc(tok[i:i + 1]) for i in range(5)])
        out[hm, "reversed"] = enc(np.ascontiguousarray(tok[::-1]))[::-1]
        enc.close()
    assert np.isfinite(out["0", "", 5]).all() and out["0", "", 5].std() > 0.1
    assert not np.array_equal(out["0", "", 5][0], out["0", "", 5][1])
    for cfg in ("", "0", "2", "10"):
        for n in ENC_BATCHES:
            assert np.array_equal(out["1", cfg, n], out["0", cfg, n]), ("head-major", cfg, n)
    for n in ENC_BATCHES:
        assert np.array_equal(out["0", "1", n], out["0", "0", n]), ("cfg 1 vs 0", n)
        assert np.array_equal(out["0", "2", n], out["0", "0", n]), ("cfg 2 vs 0", n)
    for hm in ("0", "1"):
        full = out[hm, "", 5]
        assert np.array_equal(out[hm, "alone"], full), ("alone", hm)
        assert np.array_equal(out[hm, "reversed"], full), ("batch position", hm)
        assert np.array_equal(out[hm, "", 3], full[:3]) and np.array_equal(out[hm, "", 1], full[:1]), ("batch size", hm)


def _linear_f32(x, w, b, q):
    """OV.linear with a float32-accumulating matmul: another valid float32 evaluation of the same bf16-rounded operands"""
    y = OV._q(x, q) @ OV._q(w, q).T
    if b is not None:
        y = y + b.astype(F32)
    return y.astype(F32)


@pytest.mark.parametrize("name", list(ENC_SPECS))
def test_encoder_accuracy_against_oracle(ctx, monkeypatch, name):
    """The encoder against OV.encoder(q=True) (bf16 rounding at the same points, float64 accumulation), batch 3.  The tolerance
    is measured from the reference alone: the control is the same oracle with OV.linear swapped for a float32-accumulating
    matmul, a second valid float32 evaluation, which also triggers the downstream 1-ulp bf16 flips.  GPU max deviation <= 4 x
    the control's and GPU rms <= 2 x the control's: the maximum over ~1e5 outputs fluctuates from case to case, the rms is the
    robust statistic (the reasoning of check_layer in tests/test_gpu_split.py).

    Measured on an MI355X (deviation from the oracle, GPU against the float32 control; both pairs are printed on every run):
      dim 256 (output range 4.66)  GPU max 7.62e-3, rms 1.31e-3   control max 6.64e-3, rms 9.94e-4
      dim 640 (output range 5.25)  GPU max 8.44e-3, rms 1.35e-3   control max 8.56e-3, rms 1.23e-3"""
    spec = ENC_SPECS[name]
    p = MV.synth_params(spec, seed=23)
    tok = _tokens(spec, 3, 33)
    ref = OV.encoder(tok, p, spec, True).astype(np.float64)
    with monkeypatch.context() as mp:
        mp.setattr(OV, "linear", _linear_f32)
        control = OV.encoder(tok, p, spec, True).astype(np.float64)
    assert not np.array_equal(control, ref)
    c_max, c_rms = np.abs(control - ref).max(), np.sqrt(np.mean((control - ref) ** 2))
    monkeypatch.delenv("POSEPIPE_GEMM_CFG", raising=False)
    monkeypatch.delenv("POSEPIPE_VIT_HEAD_MAJOR", raising=False)
    enc = _Encoder(ctx, spec, p, max_batch=3)
    got = enc(tok).astype(np.float64)
    enc.close()
    g_max, g_rms = np.abs(got - ref).max(), np.sqrt(np.mean((got - ref) ** 2))
    print(f"encoder {name} batch 3, output range {np.abs(ref).max():.2f}: GPU max {g_max:.3e} rms {g_rms:.3e}; "
          f"float32 control max {c_max:.3e} rms {c_rms:.3e}")
    assert g_max <= 4 * c_max, (g_max, c_max)
    assert g_rms <= 2 * c_rms, (g_rms, c_rms)


# ---- 4. LayerNorm edges (standalone ABI) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 252, 256, 260, 1280, 1792, 2048])       # NV = 1 .. 8, partially filled last vectors
@pytest.mark.parametrize("rows", [1, 2, 3, 5, 1025])                        # 4 rows per block: partial and many blocks
def test_layernorm_edges(ctx, rows, dim):
    """Three kinds of rows against float64: the benign ones of test_layernorm (std 3 around 1), mean 50 with std 1 (the mean
    is 50 x the deviations: cancellation in x - mean), std 1e-3 around 0 (variance at the size of eps).

    Per-row bound from the kernel's two-pass form.  The mean is a sum of at most 4 NV + 6 float32 additions (NV x (3 + 1) per
    lane, 6 shuffle steps) and one division, so |mean error| <= (4 NV + 7) 2^-24 max|x_row|, amplified by 1 / sigma_row; the
    deviations, the variance, rstd and the affine step add 8 half-ulps of |y|, the last add one of |beta|:
        |err| <= ((4 NV + 7) 2^-24 max|x_row| / sigma_row + 8 2^-24 |y|) |gamma| + 2^-24 |beta|
    with y the normalised value and sigma_row = sqrt(var + eps).  Rows without the large mean also keep rtol 1e-5 / atol 2e-5;
    bf16 outputs are within one bf16 ulp."""
    nv = (dim // 4 + 63) // 64
    rng = np.random.default_rng([4, rows, dim])
    g = rng.uniform(0.5, 1.5, dim).astype(F32)
    b = rng.standard_normal(dim, dtype=F32)
    z = rng.standard_normal((3, rows, dim), dtype=F32)
    kinds = {"benign": (z[0] * 3 + 1).astype(F32), "mean50": (z[1] + 50).astype(F32), "std1e-3": (z[2] * F32(1e-3)).astype(F32)}
    dg, db = Dev(ctx, g), Dev(ctx, b)
    for kind, x in kinds.items():
        x64 = x.astype(np.float64)
        mu = x64.mean(-1, keepdims=True)
        sigma = np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + OV.LN_EPS)
        y = (x64 - mu) / sigma
        ref = y * g.astype(np.float64) + b.astype(np.float64)
        bound = ((4 * nv + 7) * 2.0 ** -24 * np.abs(x64).max(-1, keepdims=True) / sigma + 8 * 2.0 ** -24 * np.abs(y)) * np.abs(g) \
            + 2.0 ** -24 * np.abs(b)
        dx = Dev(ctx, x)
        dy = Dev(ctx, nbytes=rows * dim * 4)
        ctx.h2d(dy.ptr, np.full(rows * dim * 2, 0x7fc1, np.uint16))
        L.check(ctx.lib.pp_layernorm(ctx.handle, dx.ptr, dg.ptr, db.ptr, rows, dim, OV.LN_EPS, dy.ptr, 0), "pp_layernorm")
        ctx.synchronize()
        got = dy.get((rows, dim), F32)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"layernorm {rows}x{dim} {kind}: max err {err.max():.3e}, worst err/bound {np.max(err / bound):.3f}")
        assert (err <= bound).all(), (kind, int((err > bound).sum()), float(np.max(err / bound)))
        if kind != "mean50":
            np.testing.assert_allclose(got, OV.layernorm(x, g, b), rtol=1e-5, atol=2e-5)
        L.check(ctx.lib.pp_layernorm(ctx.handle, dx.ptr, dg.ptr, db.ptr, rows, dim, OV.LN_EPS, dy.ptr, 1), "pp_layernorm")
        ctx.synchronize()
        got16 = dy.get((rows, dim), np.uint16)
        if kind != "mean50":
            _close_bf16(got16, ref.astype(F32))
        else:
            # the bf16 output is the RNE rounding of the float32 one, whose error may be `bound` here (up to ~1e-4, more than
            # _close_bf16's 1e-5 of slack): a value that close to a rounding boundary may land on the other neighbour, which
            # is half a bf16 ulp (<= 2^-8 |ref|) plus that error away -- still within one bf16 ulp
            err16 = np.abs(OV.bf16_from_bits(got16).astype(np.float64) - ref)
            tol16 = 2.0 ** -8 * np.abs(ref) + 1e-5 + bound
            assert (err16 <= tol16).all(), (kind, int((err16 > tol16).sum()), float(np.max(err16 - tol16)))
        dx.free(); dy.free()
    dg.free(); db.free()


# ---- 5. PP_OP_DECONV_BF16, integer-exact ---------------------------------------------------------------------------------------
DECONV_SHAPES = [(2, 16, 12, 1280, 256),                     # the ViT-H head
                 (3, 5, 7, 64, 8), (1, 1, 1, 128, 24), (2, 1, 9, 64, 16), (2, 8, 1, 192, 40)]
assert any(h > 1 and w > 1 for _, h, w, _, _ in DECONV_SHAPES)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n,h,w,cin,cout", DECONV_SHAPES)
def test_deconv_bf16_integer_exact(ctx, n, h, w, cin, cout, relu):
    """ConvTranspose2d(4, 2, 1) + bias (+ ReLU) as one bf16 GEMM over the 16 kernel taps + gather, on integers (|sum| <= 4 taps x
    cin x 8 < 2^24): equal to the float64 definition.  Border outputs (1 or 2 taps present) and, where the map has them, interior
    outputs (all 4 taps) are both compared; one-pixel-wide maps have border outputs only."""
    rng = np.random.default_rng([5, n, h, w, cin, cout])
    x = rng.integers(-4, 5, (n, h, w, cin)).astype(F32)
    wt = rng.integers(-2, 3, (cin, cout, 4, 4)).astype(F32)
    bias = rng.integers(-16, 17, cout).astype(F32)
    assert 4 * cin * 8 + 16 < 2 ** 24
    ref = OV.conv_transpose_4s2p1(x, wt) + bias.astype(np.float64)
    if relu:
        ref = np.maximum(ref, 0.0)
    taps = OV.conv_transpose_4s2p1(np.ones((1, h, w, 1), F32), np.ones((1, 1, 4, 4), F32))[0, :, :, 0]     # taps present per output pixel
    assert (taps < 4).any() and (taps == 4).any() == (h > 1 and w > 1) and taps.min() >= 1
    b = ProgramBuilder()
    xin = b.buf(h, w, cin, name="input")
    b.deconv4x4s2_bf16(xin, wt, bias, relu=L.PP_RELU_LAST if relu else L.PP_RELU_NONE)
    prog = b.build()
    net = Net(ctx, prog, n)
    dptr, nbytes, _ = net.buffer("input")
    assert nbytes == h * w * cin * 4
    ctx.h2d(dptr, x)
    net.run(n)
    ctx.synchronize()
    got = net.read(prog.ops[0].out, n)
    net.close()
    assert got.shape == ref.shape
    assert np.array_equal(got.astype(np.float64), ref), (int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
    if relu:
        assert (got == 0).any() and (got > 0).any()
    else:
        assert (got < 0).any()


# ---- 6. pp_f32_to_bf16 --------------------------------------------------------------------------------------------------------
def _f32_patterns():
    """all 65 536 upper halves x the lower halves that decide the rounding: exact, just above, just below a tie, the tie, just
    above the tie, all ones -- ties to even on both parities, float32 subnormals, +-0, +-inf, 0x7f7fffff -> inf, every NaN form"""
    hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
    lo = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], np.uint32)[None, :]
    return (hi | lo).reshape(-1)


@pytest.mark.parametrize("n", [1, 255, 257, 2 ** 24 + 3])    # one partial block, block edges, the grid-stride loop beyond 65 536 blocks
def test_f32_to_bf16_all_patterns(ctx, n):
    """pp_f32_to_bf16 converts every encoder weight: bits equal OV.bf16_bits (RNE) on every non-NaN pattern; a NaN stays a NaN
    (payload not compared)."""
    pat = _f32_patterns()
    if n < pat.size:
        # 0x3f818000, a tie that RNE rounds UP to the even 0x3f82; around the largest finite / inf / NaN; subnormals
        start = {1: 0x3f81 * 6 + 3, 255: 0x7f7f * 6 - 100, 257: 0}[n]
        bits = pat[start:start + n].copy()
    else:
        bits = np.resize(pat, n)
    assert bits.size == n
    x = bits.view(F32)
    dx, dy = Dev(ctx, x), Dev(ctx, nbytes=n * 2 + 2)
    ctx.h2d(dy.ptr, np.full(n + 1, 0x1234, np.uint16))
    L.check(ctx.lib.pp_f32_to_bf16(ctx.handle, dx.ptr, dy.ptr, n), "pp_f32_to_bf16")
    ctx.synchronize()
    got = dy.get((n + 1,), np.uint16)
    dx.free(); dy.free()
    assert got[n] == 0x1234                                   # nothing written past the end
    got = got[:n]
    nan = (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    with np.errstate(all="ignore"):
        want = OV.bf16_bits(x)
    bad = ~nan & (got != want)
    assert not bad.any(), (int(bad.sum()), [hex(v) for v in bits[bad][:6]], [hex(v) for v in got[bad][:6]])
    assert ((got[nan] & 0x7fff) > 0x7f80).all()
    if n > 2 ** 24:
        assert nan.any() and want[bits == 0x7f7fffff][0] == 0x7f80 and want[bits == 0x3f808000][0] == 0x3f80
