"""The split-conv kernels, bit for bit: a guard for structural changes to posepipeline_amd/csrc/conv_split*.

A sha256 over the output bytes of every kernel family (tap kernel in tile / stream mode with one to four channel blocks per wave and
with 4 / 8 waves, the 48-channel kernel, the one-tap and tap-gather products, the product kernel under both of its epilogues and with
a folded shortcut, the strided-patch form, the stem) and of every epilogue path (no residual, res1 with ReLU last / first, res1 + res2,
an activation, a shifted residual), under both split forms where the form exists.  Inputs are seeded and heavy-tailed, so that the low
planes of the operand splits matter.  There is no reference: the table below was recorded on the commit BEFORE the kernels were
split into one file per family with shared device pieces (conv_split_dev.h), by running `python -m tests.test_gpu_split_digests`
there, and a refactor of these files must reproduce it.  A digest that differs after a structural change is a bug in that change; the
table is not regenerated for it.  A change that alters a summation order ON PURPOSE runs the same command, pastes its output over the
table and says so.

Not reached by any case: the 16 instances of the tap kernel's 4-wave form with per-wave weight loads (conv_split_tap_nw4.hip, 3x3).
The launcher takes them only where the weight ring does not fit or with POSEPIPE_SPLIT_RING4=0, which is read once per process;
tools/kernel_isa_diff.py (the compiler's output per kernel, old tree against new) is what guards them.

The form each case takes (launcher tag, channel blocks per wave, waves, patch slots per thread) is written beside it; it was read
from a build of the launcher that prints them."""
import hashlib
import zlib

import numpy as np
import pytest

from posepipeline_amd import _lib as L
from posepipeline_amd.program import Net, ProgramBuilder
from tests.helpers import hip_conv_op
from tests.test_gpu_split_fold import _pair_program

pytestmark = pytest.mark.gpu
LAST, FIRST = L.PP_RELU_LAST, L.PP_RELU_FIRST


def _heavy(rng, shape):
    """activations spanning ~6 orders of magnitude (as test_split_3x3_is_as_accurate_as_the_float32_chain)"""
    return (rng.standard_normal(shape) * np.exp(2 * rng.standard_normal(shape))).astype(np.float32)


def _layer(rng, n, h, w, cin, cout, k=3, stride=1):
    pad = k // 2 if k == 3 else 0
    x = _heavy(rng, (n, h, w, cin))
    wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    r1, r2 = (rng.standard_normal((n, ho, wo, cout)).astype(np.float32) for _ in range(2))
    return x, wt, b, pad, r1, r2


def conv_case(n, h, w, cin, cout, k=3, stride=1, variants="all"):
    """one conv layer through pp_conv2d: no residual; res1 + ReLU last; res1 + ReLU first; res1 + res2 + ReLU last"""
    def run(ctx, rng):
        x, wt, b, pad, r1, r2 = _layer(rng, n, h, w, cin, cout, k, stride)
        todo = {"all": ((0, None, None), (LAST, r1, None), (FIRST, r1, None), (LAST, r1, r2)), "res1": ((LAST, r1, None),),
                "mish": ((L.PP_ACT_MISH, r1, None),), "plain": ((0, None, None), (LAST, r1, None))}[variants]
        return [hip_conv_op(ctx, x, wt, b, stride=stride, pad=(pad, pad), relu=relu, res1=ra, res2=rb) for relu, ra, rb in todo]
    return run


def chain_case(h, w, c, n):
    """conv -> conv on zero-halo buffers: the second conv's activation scale (fp16 form) is what the first one's epilogue stored"""
    def run(ctx, rng):
        pb = ProgramBuilder()
        x = pb.buf(h, w, c, name="input")
        wts = [(rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32) for _ in range(2)]
        bs = [rng.standard_normal(c).astype(np.float32) for _ in range(2)]
        y1 = pb.conv(x, wts[0], bs[0], pad=1, relu=LAST)
        pb.conv(y1, wts[1], bs[1], pad=1, relu=LAST, res1=y1, out=pb.buf(h, w, c, name="output"))
        prog = pb.build()
        assert max(prog.buf_pad) > 0
        net = Net(ctx, prog, max_batch=n)
        assert (net.conv_kinds() == 2).all()
        y = net.forward(_heavy(rng, (n, h, w, c)))
        net.close()
        return [y]
    return run


def both_epilogues(fn):
    """a product-kernel case under the register epilogue and the one transposed through LDS: the same bytes"""
    def run(ctx, rng):
        state = rng.bit_generator.state
        out = []
        for epi in (0, 1):
            rng.bit_generator.state = state
            L.check(ctx.lib.pp_debug_knob(b"split_gemm_epilogue", epi), "pp_debug_knob")
            try:
                out.append(fn(ctx, rng))
            finally:
                L.check(ctx.lib.pp_debug_knob(b"split_gemm_epilogue", -1), "pp_debug_knob")
        assert all(np.array_equal(a, b) for a, b in zip(*out)), "the product kernel's two epilogues differ"
        return out[0]
    return run


def shifted_case(ctx, rng):
    """FPN lateral: 1x1 + the coarser map read at (y >> 1, x >> 1), odd fine map"""
    x = _heavy(rng, (3, 21, 35, 512))
    wt = (rng.standard_normal((256, 512, 1, 1)) / np.sqrt(512)).astype(np.float32)
    b = rng.standard_normal(256).astype(np.float32)
    r = rng.standard_normal((3, 11, 18, 256)).astype(np.float32)
    return [hip_conv_op(ctx, x, wt, b, res1=r, res1_shift=1)]


def fold_case(ctx, rng):
    """tests/test_gpu_split_fold.py's smallest case: the projection shortcut as the product's second K segment"""
    n, h, w, cx, ch, cout, stride = 2, 20, 13, 64, 64, 256, 1
    prog, _ = _pair_program(h, w, cx, ch, cout, stride, rng)
    net = Net(ctx, prog, max_batch=n, numerics="split_f16")
    assert int((net.folded_into() >= 0).sum()) == 1
    y = net.forward(_heavy(rng, (n, h, w, cx + ch)) * (10.0 ** np.linspace(-3, 2, n)).reshape(-1, 1, 1, 1).astype(np.float32))
    net.close()
    return [y]


def stem_case(n, h, w):
    def run(ctx, rng):
        wt = (rng.standard_normal((64, 4, 7, 7)) / np.sqrt(147)).astype(np.float32)
        wt[:, 3] = 0
        x = _heavy(rng, (n, h, w, 4))
        x[..., 3] = 0
        b = rng.standard_normal(64).astype(np.float32)
        return [hip_conv_op(ctx, x, wt, b, stride=2, pad=(3, 3), relu=relu) for relu in (LAST, 0)]
    return run


F16, BF16 = "f16", "bf16"
# name -> (the split forms it runs under, case).  Shapes are (n, h, w, cin, cout).  Behind each case, the form it was seen to take:
# launcher tag (ring4 / nw4 / nw8: tap kernel with the weights through the 4-wave ring / per-wave loads / the 8-wave ring; gemm4: the tap
# kernel's product form; c48 / c48ring; g256x128: product kernel; s2p; stem7), channel blocks per wave, patch slots per thread -- for
# the fp16 form | the bf16 form where they differ
CASES = {
    # tap kernel, tile mode: the four tile shapes and two ragged maps, four epilogue variants each
    "tile_8x32": ((F16, BF16), conv_case(1, 8, 32, 32, 64)),            # ring4, 2 blocks, 6 slots
    "tile_4x64": ((F16, BF16), conv_case(2, 4, 64, 16, 32)),            # ring4, 1 block, 7 slots
    "tile_32x8": ((F16, BF16), conv_case(1, 32, 8, 64, 96)),            # ring4, 1 block (three columns), 7 slots
    "tile_16x16": ((F16, BF16), conv_case(2, 16, 16, 32, 64)),          # ring4, 2 blocks, 6 slots
    "ragged_33x29": ((F16, BF16), conv_case(1, 33, 29, 128, 100)),      # ring4, 2 blocks, 6 slots
    "ragged_7x100": ((F16, BF16), conv_case(1, 7, 100, 32, 20)),        # ring4, 1 block, 6 slots
    "mish_res1": ((F16, BF16), conv_case(2, 26, 26, 64, 128, variants="mish")),     # ring4, 2 blocks, 6 slots
    # three and four channel blocks per wave (fp16 form, 432 workgroups; bf16: one / two)
    "cob3": ((F16, BF16), conv_case(12, 96, 96, 32, 96, variants="res1")),          # ring4, 3 blocks | 1 block, 6 slots
    "cob4": ((F16, BF16), conv_case(12, 96, 96, 32, 128, variants="res1")),         # ring4, 4 blocks | 2 blocks, 6 slots
    # 8-wave form (bf16; the fp16 form takes the 4-wave ring form)
    "nw8_256": ((F16, BF16), conv_case(8, 96, 96, 256, 256, variants="res1")),      # ring4, 4 blocks, 6 slots | nw8, 2 blocks, 5 slots
    "nw8_96": ((F16, BF16), conv_case(10, 96, 96, 256, 96, variants="res1")),       # ring4, 1 block, 6 slots | nw8, 1 block, 5 slots
    # two convs on zero-halo buffers; the first reads the program's input (no halo) in tile mode.  Second conv in stream mode (a tile
    # across samples; under the fp16 form it scales by the maxima the first one's epilogue stored) ...
    "stream_27x36": ((F16, BF16), chain_case(27, 36, 32, 3)),           # ring4 tile, 7 slots, then ring4 STREAM, 6 slots; 1 block
    "chain_20x34": ((F16, BF16), chain_case(20, 34, 32, 3)),            # the same forms: the stream wastes fewer positions here, too
    # ... and in tile mode between halo buffers (two whole 8x32 tiles per sample beat the stream's 512 of 612 positions)
    "chain_16x32": ((F16, BF16), chain_case(16, 32, 32, 3)),            # ring4 tile, 6 slots, both convs; 1 block
    # 48-channel kernel (fp16 form: weights through the ring; bf16: per-wave loads)
    "c48_16x16": ((F16, BF16), conv_case(2, 16, 16, 48, 48)),           # c48ring | c48, 6 slots
    "c48_9x40": ((F16, BF16), conv_case(2, 9, 40, 256, 40)),            # c48ring | c48, 6 slots
    "c48_64x48": ((F16, BF16), conv_case(1, 64, 48, 16, 36)),           # c48ring | c48, 6 slots
    # one-tap form of the tap kernel
    "onetap_s1": ((F16, BF16), conv_case(2, 12, 20, 1024, 96, k=1, variants="plain")),              # gemm4, 1 block
    "onetap_s2": ((F16, BF16), conv_case(2, 12, 20, 1024, 96, k=1, stride=2, variants="plain")),    # gemm4, 1 block
    "onetap_column": ((F16,), conv_case(1, 64, 64, 256, 64, k=1, variants="plain")),                # gemm4, 2 blocks (one column)
    # product kernel (g256x128), each under both epilogues
    "product_1024": ((F16, BF16), both_epilogues(conv_case(2, 12, 20, 1024, 256, k=1, variants="all"))),
    "product_64": ((F16, BF16), both_epilogues(conv_case(1, 20, 34, 64, 128, k=1, variants="all"))),     # ragged last tile
    "product_roi": ((F16, BF16), both_epilogues(conv_case(300, 7, 7, 64, 128, k=7, variants="plain"))),  # a sample per pixel
    "product_shifted": ((F16, BF16), both_epilogues(shifted_case)),
    "product_fold": ((F16,), both_epilogues(fold_case)),                                                 # second K segment
    # 3x3 stride 2, strided-patch form (fp16): one to four channel blocks per wave; 16x8 tiles (13 slots) and 8x16 tiles (10 slots)
    "s2p_cob1": ((F16,), conv_case(2, 60, 100, 16, 32, stride=2, variants="plain")),        # s2p, 1 block, 13 slots
    "s2p_cob2": ((F16,), conv_case(2, 95, 71, 64, 64, stride=2, variants="plain")),         # s2p, 2 blocks, 13 slots
    "s2p_cob3": ((F16,), conv_case(2, 96, 72, 48, 96, stride=2, variants="plain")),         # s2p, 3 blocks, 13 slots
    "s2p_cob4": ((F16,), conv_case(1, 80, 136, 256, 256, stride=2, variants="plain")),      # s2p, 4 blocks, 10 slots
    "s2p_tall": ((F16,), conv_case(1, 131, 33, 32, 160, stride=2, variants="plain")),       # s2p, 1 block (five columns), 13 slots
    # 3x3 stride 2, tap-gather product: where the strided-patch map rule says no (fp16), from 128 channels with even blocks (bf16)
    "gather_f16": ((F16,), conv_case(2, 24, 18, 96, 384, stride=2, variants="plain")),      # gemm4, 2 blocks
    "gather_128": ((F16, BF16), conv_case(2, 21, 33, 128, 128, stride=2, variants="plain")),    # gemm4, 2 blocks
    # stem (fp16 form only): stem7
    "stem_21x37": ((F16,), stem_case(1, 21, 37)),
    "stem_64x128": ((F16,), stem_case(2, 64, 128)),
}

# name -> {split form: digest}
DIGESTS = {
    "tile_8x32": {"f16": "660c5722c6d02af373b6338e3788210d5e6308cfb8186fadc72158f399592400",
                 "bf16": "b7ba6a6aab474bfdf08ff053567252eed9308b03cf785684c4ecb72c21427a0c"},
    "tile_4x64": {"f16": "b450c1da2bfa43e96dc46fc05111ca18e08e44338c467765606e9c9fa761b9e8",
                 "bf16": "501c962b073ad63ab34732667dc0e6bdf6b0dd10072b378f433a68df7a0ffa06"},
    "tile_32x8": {"f16": "cab08ad11d5de29973dcb9a113628836ef0029bc3d29e24ed6a6700499b796a8",
                 "bf16": "5de58862a7a33f7d4ad5e3c20c29212a2d1c210d0c96cac017a4787f599f3123"},
    "tile_16x16": {"f16": "e74e08c150788203da624a2da2a6591f7a411a9412033c3fa551e43a0a6da33c",
                  "bf16": "5abba25ce29425e96f6e4f22b9533aaa5e9d51fd053679cb0856f45517b286d7"},
    "ragged_33x29": {"f16": "9c9ec009f85c04842cc3b600f29017e29d538d0fa49d7bdcbb4dcb621a501151",
                    "bf16": "2107db5501277f26e5e0eb0f358e04a1c27534fd8d3177a98c6cf800667ae8e1"},
    "ragged_7x100": {"f16": "ab82844ac85d97d198d9a4ddd1a08a149c0ee3bbd4a3a55030e9c7d0b2272c08",
                    "bf16": "fec6f4fc60e8c4df0b95d7250630ea5c357e562f1eac79b6c7b0e9b2990978f8"},
    "mish_res1": {"f16": "b10a2952fe4b99908fcae72796e98abe360d55cb0037c3c16c037199abc09fb9",
                 "bf16": "f7a836458bcd952110882debd57f317085c9c695eca8a0fe193641dd467a4863"},
    "cob3": {"f16": "141c14c19a4e903de7ba14943483b751ef329ae7406071bc99d0d8a2bb65afb2",
            "bf16": "e81d125a0549ff61889b156f8b4bfde21744e82fefad45df7b8fa50d51b5d152"},
    "cob4": {"f16": "ce723a7ce4ae67a35926ecf635db9baf2e4a5dd9ebcf534a54653dba64cd57a0",
            "bf16": "32fcd25973b675175a76ad189e09f4069a4ee6b11b82f719d3c95bac8bce9414"},
    "nw8_256": {"f16": "1810f2a549e2281b2338555c0351286176b454a179d02fbd5550b49b858b88f8",
               "bf16": "547e65951794dedf0f8b89597f249e8dee7293fe64f56f30f8fd805af0979b5f"},
    "nw8_96": {"f16": "5b01fddf56f13dede311d41ef9ff786b7a00e61c1ca5a059037b3e2f919c70e9",
              "bf16": "f704209d28e128af8288c08259b120c2bbae7616095bbb2d6e0cd2737dce92f6"},
    "stream_27x36": {"f16": "792d3486061eac0505adbccf359d18f5659e0b07f91fddfb4036c8f8722b16ba",
                    "bf16": "356c34428dfc2f74f83b988034441d01c525f0e803b3045f0b1b081c19cad13f"},
    "chain_20x34": {"f16": "fd232d88c3f4a68e963c49fe136b2094674c0b9d325dbe33d45a8452508a30ce",
                   "bf16": "561193b20929a01b164f4f21cc482289ac113135b62e70d4f61833fc5b7ea1b2"},
    "chain_16x32": {"f16": "89f78da68af656c0976ea2a402b5df39003197523bfce1661159c58f57c8c0d0",
                   "bf16": "0a76db9c45c28c11436dd800666181642c77cb12663c47e0d45f92e03600199c"},
    "c48_16x16": {"f16": "0d807372aabcc31a892f9c09d1fe679cc2203c99490aac1f47305f084b453ddd",
                 "bf16": "72eb3b918ec25e9d65e1bbbe245ce93db74c4a85b443b5c27f92cf5b28f6ebe8"},
    "c48_9x40": {"f16": "ffb2a00cba75849978aac18690e7ce660e7d45d89437e826b15a11e7ce21a5ce",
                "bf16": "1c1771972dc8982f5483ff67f9d02cd7e08a97737783b300245deb89f9e88f34"},
    "c48_64x48": {"f16": "e1d0a228aa9c5d7032ca8d31c08f0a8b2d30204da6c4c6e6563ef9485cb9cb28",
                 "bf16": "43bbb91cfa22d0923971d3427ea1f81a83057e48e9cdc6905d48d45f1b7d41ae"},
    "onetap_s1": {"f16": "324d22ad97c5f8951795e88dee0cb1d5236cca6cb5990ac5957e192a76ad71bb",
                 "bf16": "0ce8e8fedd46f21e008c36bcd2c39d986e082d5b2cb0374801a420a732f25462"},
    "onetap_s2": {"f16": "eea6d78635842eca48ab3e5b52fcb155eca88ee277f7a9f2347f31a1e400d4d2",
                 "bf16": "141ed1eb238ac9a9d905cede90daf25012ae8e19a8f78dbe9c7191eb93ac57a3"},
    "onetap_column": {"f16": "3b6c25aef843323a6ca0d486f7f31113ecc334568eb5018d54183f6197a076ae"},
    "product_1024": {"f16": "8419694a86edcaffcdea5b0a3a13b61115b970e7bddbd661ea767e8f357b6b36",
                    "bf16": "e394d41ec757558754a4ce88117cbfdd47bc4007cd0180d394ede761a7512b71"},
    "product_64": {"f16": "8fbe9a401bb30f38f060767057f5607fb1ed6e00ac39e6e2d8cecb9b65e74f96",
                  "bf16": "6c3a94f56d93224db40e152a6eab66142f25025ef0ffef9b802df4e796731ce4"},
    "product_roi": {"f16": "f92fe64ed4def079bdf892277cf061c60924fcb8d4a67b89e30289ea34b82fd0",
                   "bf16": "bfaeac06fd9d91dd0242d6aaa1592395d7bb6cb0c059d38f2ca2ec7b39433733"},
    "product_shifted": {"f16": "2d21f7bd7f020fe624d6fa68eada85b99d88bbb7bbe3b039e650ecce157b4c97",
                       "bf16": "1db20ab4038b647e7604db678480ff613cfdb93272390737fbf790de33051fa8"},
    "product_fold": {"f16": "7d11fba3d2dd6a86dc9e8613272ab9ec9d2b18d8c349b70888a8cac258ff488f"},
    "s2p_cob1": {"f16": "ba29bf2903a23210e8908ac498d74388410b9efec8538175e36c176744fa3786"},
    "s2p_cob2": {"f16": "fafdec4613ace6b8ef581009ab275d64eb94f81a801dbe389df67ec5c007e4e3"},
    "s2p_cob3": {"f16": "c16159af322251e661ac29e88d5966364f9d0264740e53dbcc1476b3b6d40dcc"},
    "s2p_cob4": {"f16": "299dfa4bf110bded6979078a983d09cd7343bb139765c4bdd6f91d525d8744bc"},
    "s2p_tall": {"f16": "4073de525638ccf15949e99a19663d1a46a5b2a9d40ce24a72da2ed56bfeec62"},
    "gather_f16": {"f16": "b0342f2e53a33e530525d71cb9012d86f37f495885750c218671724fce7308e1"},
    "gather_128": {"f16": "72fa77b5081498c059e719297f7fe34ba2f8cdf1982be73e221164b87de69728",
                  "bf16": "32f3cda7a842944c2402f1cb0c99bc6cebf5108d0ed6422cc87290840de19f4f"},
    "stem_21x37": {"f16": "d4e94fd10ac8fec479105bab1f61b502fafc7037ef60f48710890753e34de02b"},
    "stem_64x128": {"f16": "efc48387e58f4b5dda794f24d5252bb1e0945c166917099a50bdbdbfafde3285"},
}


def digest_of(ctx, name, form):
    fn = CASES[name][1]
    L.check(ctx.lib.pp_conv_split_kind(1 if form == F16 else 0), "pp_conv_split_kind")
    L.check(ctx.lib.pp_conv_exact(0), "pp_conv_exact")
    try:
        outs = fn(ctx, np.random.default_rng(zlib.crc32(name.encode())))
    finally:
        L.check(ctx.lib.pp_conv_split_kind(-1), "pp_conv_split_kind")
        L.check(ctx.lib.pp_conv_exact(1), "pp_conv_exact")
    h = hashlib.sha256()
    for y in outs:
        assert np.isfinite(y).all()
        h.update(np.ascontiguousarray(y, np.float32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name,form", [(n, f) for n in CASES for f in CASES[n][0]])
def test_split_kernel_output_unchanged(ctx, name, form):
    assert digest_of(ctx, name, form) == DIGESTS[name][form]


def test_table_covers_every_case():
    assert {(n, f) for n in DIGESTS for f in DIGESTS[n]} == {(n, f) for n in CASES for f in CASES[n][0]}


if __name__ == "__main__":
    import sys
    import time

    _ctx = L.Context(0)
    print("DIGESTS = {")
    for _name in CASES:
        _t = time.time()
        print(f"case {_name}", file=sys.stderr, flush=True)
        _d = {_f: digest_of(_ctx, _name, _f) for _f in CASES[_name][0]}
        print(f'    "{_name}": {{' + ",\n".join(f'{" " * (8 + len(_name)) if _i else ""}"{_f}": "{_v}"' for _i, (_f, _v) in enumerate(_d.items())) + "},")
        print(f"{_name}: {time.time() - _t:.1f} s", file=sys.stderr, flush=True)
    print("}")
    _ctx.close()
