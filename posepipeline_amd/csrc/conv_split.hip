// fp32 convolution on the bf16 matrix cores: three-way operand split, six MFMA products per term, fp32 accumulation.
//
// Why: v_mfma_f32_16x16x4_f32 peaks at 256 FLOP/clk/CU (157 TFLOP/s at 2.4 GHz); conv_igemm(_p3).hip sustain 0.76-0.85 of it and
// the detector / HRNet chunks are bound by exactly that (profiles/r02_conv_ablation.txt).  v_mfma_f32_32x32x16_bf16 runs 16x
// that rate.  A float32 value is the EXACT sum of three bfloat16 values (24 significand bits = 8 + 8 + 8, same exponent range):
//     a = a0 + a1 + a2,   a0 = bf16(a),  a1 = bf16(a - a0),  a2 = a - a0 - a1   (round to nearest even; every residual is exact)
// so a*b = sum_{i,j} ai*bj, every ai*bj exact in the MFMA's fp32 product.  Keeping the six terms with i + j <= 2 drops
// a1*b2 + a2*b1 + a2*b2 ~ 2^-26 |a*b| with random signs (|a1| <= 2^-9 |a|, |a2| <= 2^-17 |a|) -- a sixth of ONE float32
// rounding of the product, which a float32 FMA chain commits at every step anyway.  The sums are accumulated in the MFMA's float32 accumulators.  Cost: 6 bf16 MFMAs of 16 k for what
// takes 4 fp32 MFMAs of 4 k = 2.67x the arithmetic peak (419 TFLOP/s fp32-equivalent).
// Results are NOT bit-identical to oracle/conv_ref.c (different summation order and the dropped 2^-23 terms): the measured
// deviation is that of a reordered float32 sum (tests/test_gpu_split.py: same error against a float64 convolution as the
// exact kernel, and a control with the bit-exact kernels on the transposed network).  POSEPIPE_CONV_EXACT=1 / pp_conv_variant(3) selects the bit-exact fp32-MFMA kernels instead.
//
// Files: this one holds the plan (pp_conv_split_plan) and the dispatch (pp_launch_conv_split); conv_split_dev.h the device pieces the
// kernels share, conv_split_internal.h the declarations between these files; one translation unit per kernel family --
// conv_split_tap.h (the tap kernel's template; instances in conv_split_tap_ring4 / _nw4 / _nw8.hip), conv_split_c48.hip,
// conv_split_gemm.hip, conv_split_stem.hip -- and conv_split_weights.hip (weight splits, pp_launch_amax, and the tap kernel's
// strided-patch instances: see there).
// Kernels: conv_split_kernel (3x3, stride 1, pad 1 -- 52 % of the detector's and ~85 % of HRNet's time; 4 waves with per-wave
// weight loads, or 8 waves with the weights through an LDS ring for long-K layers; also a one-tap form) and
// conv_split_gemm_kernel (1x1 layers from 256 input channels with Cout % 128 == 0, the RoI head's fc6 / fc7).
// Structure of conv_split_kernel:
// An implicit GEMM that gathers per tap re-reads every input element nine times through L1/L2; at 2.67x the MFMA rate that
// feed (87 GB/s per CU for a 128 x 64 tile) is over what the vector memory path delivers.  Instead a workgroup stages the
// input PATCH of its output tile once per 16 input channels:
//   * output tile: 8 pixel blocks of 32 pixels (one MFMA N tile each) arranged as a rectangle, x 64 output channels
//     (2 MFMA M tiles): 4 waves x (2 pixel blocks x 2 channel blocks) = 4 accumulators of 16 registers per wave;
//   * patch: (TH + 2) x (TW + 2) pixels x 16 channels, loaded as float32 (coalesced 64 B per pixel), split into the three
//     bf16 planes in registers (5.5 VALU ops per element, once per element per block) and written to LDS as
//     [plane][k half][pixel] 16-byte slots: the B fragment of tap (dy, dx) for a pixel block is ONE ds_read_b128 per plane
//     at slot (pixel + dy * pitch + dx) -- the nine taps are nine address offsets into the same patch;
//   * weights: pre-split on the device at net creation into MFMA A-fragment order ([16-channel chunk][tap][32 couts][plane]
//     [lane] x 16 B), read straight from global memory into registers, 1 KB contiguous per wave instruction, one tap ahead;
//   * one barrier per 16-channel chunk (9 taps x 24 MFMAs = 6912 matrix-pipe cycles per wave); the patch is double-buffered,
//     the float32 loads of chunk c + 1 are in flight during chunk c and split / written half-way through it.
// Traffic per 16-channel chunk and block: patch 340 x 64 B + weights 9 x 6 KB (L1 / L2 resident) = 11 B / matrix-pipe cycle.
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>
#include <cstring>
#include <cstdio>


#include "conv_split_internal.h"

// {m, sh} for pp_udiv (device): n / d for every 32-bit n; d == 1 is flagged by sh = 32
void pp_split_make_magic(unsigned d, unsigned (&dv)[2]) {
    if (d <= 1) { dv[0] = 0; dv[1] = 32; return; }
    unsigned k = 0;
    while ((1ull << k) < d) ++k;                                   // k = ceil(log2 d), 1 <= k <= 32
    dv[0] = (unsigned)((((1ull << k) - d) << 32) / d + 1);
    dv[1] = k - 1;
}

namespace {

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// the 256-pixel tile shape (8 blocks of 32 pixels) that wastes the fewest pixels on this map
TileGeom pick_tile(int H, int W, int max_np, int pxb) {
    static const int force = env_int("POSEPIPE_SPLIT_TILE", -1);
    TileGeom best{};
    best.eff = -1.0;
    // (bw_log2, gx_log2): 8x32, 4x64, 16x16, 32x8 pixel tiles (pxb = 2, 4 waves); 16x32, 8x64, 32x16, 64x8 (pxb = 4: 8 waves)
    const int cand[4][2] = {{0, 0}, {0, 1}, {1, 0}, {2, 0}};
    const int nblk = 4 * pxb;
    for (int i = 0; i < 4; ++i) {
        if (force >= 0 && i != force) continue;
        TileGeom g{};
        g.bw_log2 = cand[i][0];
        g.gx_log2 = cand[i][1];
        const int BW = 32 >> g.bw_log2, BH = 1 << g.bw_log2, GX = 1 << g.gx_log2, GY = nblk / GX;
        g.TW = GX * BW;
        g.TH = GY * BH;
        g.PWp = g.TW + 2;
        if (g.bw_log2 == 2)
            while (g.PWp % 8 != 4) ++g.PWp;
        g.NP = (g.TH + 2) * g.PWp;
        g.NPp = g.NP;
        while (g.NPp % 8 != 4) ++g.NPp;       // half planes 64 B apart mod 128: conflict-free ds_write_b64
        g.tiles_x = (W + g.TW - 1) / g.TW;
        g.tiles_y = (H + g.TH - 1) / g.TH;
        if (g.NP > max_np) continue;
        g.eff = (double)H * W / ((double)g.tiles_x * g.tiles_y * 128.0 * pxb) - 1e-4 * g.NP / 256.0;
        if (g.eff > best.eff) best = g;
    }
    return best;
}

// strided-patch form: the 128-pixel output tile (4 blocks of 32 pixels, one per wave) whose de-interleaved patch -- four phase maps of
// (TH + 1) x PWp slots -- serves the map best: pixels wasted at the edges against slots staged per tile
TileGeom pick_tile_s2(int H, int W, int max_np) {
    static const int force = env_int("POSEPIPE_SPLIT_TILE_S2", -1);
    TileGeom best{};
    best.eff = -1.0;
    // (bw_log2, gx_log2): 4x32 (1x32 blocks stacked), 8x16 (2x16 blocks stacked), 16x8 (4x8 blocks stacked), 4x32 as 2x2 blocks of 2x16
    const int cand[4][2] = {{0, 0}, {1, 0}, {2, 0}, {1, 1}};
    for (int i = 0; i < 4; ++i) {
        if (force >= 0 && i != force) continue;
        TileGeom g{};
        g.bw_log2 = cand[i][0];
        g.gx_log2 = cand[i][1];
        const int BW = 32 >> g.bw_log2, BH = 1 << g.bw_log2, GX = 1 << g.gx_log2, GY = 4 / GX;
        g.TW = GX * BW;
        g.TH = GY * BH;
        g.PWp = g.TW + 1;
        if (g.bw_log2 == 2)
            while (g.PWp % 8 != 4) ++g.PWp;       // two rows of a 4x8 block per lane group: 128 B apart mod 256
        g.NP = 4 * (g.TH + 1) * g.PWp;
        g.NPp = g.NP;
        while (g.NPp % 8 != 4) ++g.NPp;
        g.tiles_x = (W + g.TW - 1) / g.TW;
        g.tiles_y = (H + g.TH - 1) / g.TH;
        if (g.NP > max_np) continue;
        g.eff = (double)H * W / ((double)g.tiles_x * g.tiles_y * 128.0) - 0.05 * g.NP / 612.0;
        if (g.eff > best.eff) best = g;
    }
    return best;
}

}  // namespace

// ---- the split plan: whether a layer runs on a split kernel, on which, and with what weight layout (pp_internal.h, SplitPlan) ----------

// the 3x3 tap kernel's tiling of the map for `nw` waves (512-pixel tiles with 8, 256 with 4): the pixel tile that wastes the fewest
// pixels, or the padded input as one stream where that wastes fewer positions
static TileGeom tap_tiling(const ConvArgs& a, int nw, int stream_env) {
    const int max_np = nw == 8 ? 768 : 512, xp_h = a.Hin + a.x_pad, xp_w = a.Win + a.x_pad;
    TileGeom g = pick_tile(a.Hout, a.Wout, max_np, nw / 2);
    g.mode = MODE_TILE;
    const int snp = 64 * nw + 2 + 2 * xp_w;
    const double stream_eff = (double)a.Hout * a.Wout / ((double)xp_h * xp_w);
    bool use_stream = a.x_pad >= 1 && snp <= max_np && (g.eff < 0 || stream_eff > g.eff + 0.02);
    if (stream_env == 0 && g.eff >= 0) use_stream = false;
    if (stream_env == 1 && a.x_pad >= 1 && snp <= max_np) use_stream = true;
    if (use_stream) {
        g.mode = MODE_STREAM;
        g.PWp = xp_w;
        g.NP = g.NPp = snp;
        while (g.NPp % 8 != 4) ++g.NPp;
    }
    return g;
}

SplitPlan pp_conv_split_plan(const ConvArgs& a) {
    // selection knobs, read once per process -- except POSEPIPE_SPLIT_S2_MIN_CIN, read per plan: tests set it to run the tap-gather
    // form on every shape it supports, whatever the selection rule would pick
    static const int stem7_on = env_int("POSEPIPE_SPLIT_STEM7", 1);
    static const int s2_on = env_int("POSEPIPE_SPLIT_S2", 1), s2p_on = env_int("POSEPIPE_SPLIT_S2P", 1);
    static const int gemm8_on = env_int("POSEPIPE_SPLIT_GEMM8", 1), gemm4_min_c = env_int("POSEPIPE_SPLIT_GEMM4_MIN_C", 64);
    static const int gemm_min_cin = env_int("POSEPIPE_SPLIT_GEMM_MIN_CIN", 1024);
    static const int c48_on = env_int("POSEPIPE_SPLIT_C48", 1), c48_mult = env_int("POSEPIPE_SPLIT_C48_MULT", 0);
    static const int stream_env = env_int("POSEPIPE_SPLIT_STREAM", -1);
    const char* s2_env = getenv("POSEPIPE_SPLIT_S2_MIN_CIN");
    SplitPlan p;
    p.f16 = a.split_f16 != 0;
    const size_t wpl = p.f16 ? 2 : 3;                   // weight planes: (g0, g1) of the fp16 form, three bf16 planes
    p.ncb = (a.Cout + 31) / 32;                         // odd: one block per workgroup (COB = 1), else two
    p.nout = p.ncb * 32;
    // ResNet-50's stem on conv_split_stem7_kernel (fp16 form only: the six-product form keeps the float32 kernels there)
    if (stem7_on && p.f16 && a.KH == 7 && a.KW == 7 && a.stride == 2 && a.pad_h == 3 && a.pad_w == 3 && a.dil_h == 1 && a.dil_w == 1 &&
        a.Cin == 4 && a.Cout == 64 && a.CoutPad >= 64 && a.up_log2 == 0 && !a.out_nchw && !a.res1 && !a.res2 &&
        (a.relu == PP_RELU_NONE || a.relu == PP_RELU_FIRST || a.relu == PP_RELU_LAST) && (a.y_stride == 0 || a.y_stride == a.Cout) &&
        a.y_coff == 0 && a.Hout == (a.Hin - 1) / 2 + 1 && a.Wout == (a.Win - 1) / 2 + 1) {
        p.kernel = SPLIT_STEM7;
        p.cin = a.Cin;
        p.frag_bytes = STEM_WBYTES;
        p.bytes = p.frag_bytes + (size_t)2 * p.nout * sizeof(float);
        return p;
    }
    // how the split kernel sees the layer: taps (9 / 1) and channels per tap (a full-cover 'valid' conv is a 1x1 over KH*KW*Cin)
    const bool k3 = a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad_h == 1 && a.pad_w == 1 && a.dil_h == 1 && a.dil_w == 1 &&
                    a.Hout == a.Hin && a.Wout == a.Win;
    const bool k1 = a.KH == 1 && a.KW == 1 && a.pad_h == 0 && a.pad_w == 0;
    const bool full = a.KH == a.Hin && a.KW == a.Win && a.pad_h == 0 && a.pad_w == 0 && a.dil_h == 1 && a.dil_w == 1 &&
                      a.x_pad == 0 && a.Hout == 1 && a.Wout == 1 && !k1;
    // 3x3 stride 2 (HRNet's transition / fuse layers, ResNet's strided blocks): the product form with one step per (chunk, tap)
    // Measured (gpurun r3c, per-op profiles): it is bound by the same L2 feed as the one-tap form on 1x1 layers (~140 TFLOP/s): ResNet's
    // 128 / 256 / 512-channel strided 3x3 122 -> 132, 132 -> 139, 135 -> 140 TFLOP/s, HRNet 192 -> 384 98 -> 104; with 48 / 96 input
    // channels or ONE channel block per workgroup (Cout 96) it LOSES to the fp32 kernels (48 -> 96: 95 -> 58), so: from 128 input
    // channels, two channel blocks.  (What these layers want is the patch form with a strided patch: 4x the LDS per tile.)
    // Round 5 (fp16 form: half the products of the form the rule above was measured on; same-box per-op tables, W48, 128 samples): 96 -> 192
    // 1.26 -> 1.09 ms, 96 -> 96 0.19 -> 0.16, 96 -> 384 0.18 -> 0.15, 256 -> 96 (three blocks) 0.85 -> 0.67, 48 -> 192 0.55 -> 0.44, 48 -> 384
    // 0.10 -> 0.08; it still LOSES on 48 -> 96 (1.34 -> 2.10) and 48 -> 48 (0.80 -> 0.89): from 96 input channels, or from 48 with >= 6 blocks.
    const bool s2_pick = s2_env ? a.Cin >= atoi(s2_env) : p.f16 ? (a.Cin >= 96 || (a.Cin >= 48 && p.ncb >= 6)) : (a.Cin >= 128 && (p.ncb & 1) == 0);
    // Round 6 (fp16 form): the STRIDED-PATCH form (conv_split_kernel<.., S2>) takes every 3x3 / stride-2 / pad-1 layer -- it stages each input
    // element once and has no padding products, so the break-even rules above do not apply to it.  Same weight fragments ([chunk][tap]
    // order) as the tap-gather product, which stays the bf16 form's (and POSEPIPE_SPLIT_S2P=0's) kernel.
    const bool s2_shape = a.KH == 3 && a.KW == 3 && a.stride == 2 && a.pad_h == 1 && a.pad_w == 1 && a.dil_h == 1 && a.dil_w == 1 && !full;
    // Same-box per-op tables (profile_net w48 128 / det 64, S2P on / off): 48 -> 96 at 96x72 1.37 -> 0.91 ms (float32 kernel before), 256 -> 96
    // 0.66 -> 0.39, 64 -> 64 at 192x144 0.55 -> 0.37, 96 -> 192 1.07 -> 0.97, 48 -> 48 0.81 -> 0.76; ResNet-50 128 -> 128 at 160x272 1.07 -> 0.88,
    // 256 -> 256 1.01 -> 0.72, 512 -> 512 1.00 -> 0.93.  It LOSES where a 128-pixel tile does not fit the output map: 12x9 outputs (192 -> 384
    // 0.39 -> 0.43, 96 -> 384 0.15 -> 0.16, 48 -> 384 0.09 -> 0.11) and 48 -> 48 onto 24x18 (0.07 -> 0.08) -- those keep their former kernels.
    const bool s2p_map = a.Hout * a.Wout >= 1500 || (a.Hout * a.Wout >= 400 && a.Cout >= 96);
    const bool s2p = s2p_on && p.f16 && s2_shape && s2p_map;
    const bool k3s2 = s2_on && s2_shape && (s2_pick || s2p);
    if (!(k3 || k1 || full || k3s2)) return p;
    p.taps = (k3 || k3s2) ? 9 : 1;
    p.cin = full ? a.K : a.Cin;
    // product kernel (conv_split_gemm_kernel) for 1x1 / full-cover layers: 256 x 128 tile, 4 waves, two workgroups per CU.
    // Round 4: ONE form.  The per-workgroup timeline (tools/split_timeline.py) showed these layers bound by the CU's memory path, with the
    // epilogue as long as the K loop (256 -> 1024 at 40x68: 64k cycles of loop, 57k of epilogue) -- the 8-wave forms (256 x 256, 512 x 128: one
    // workgroup per CU) had nothing to run beside it.  With the residual lines of the epilogue requested back to back, the two-per-CU
    // form wins on EVERY layer of the detector (per 64 frames, 8-wave form -> this one): 512 -> 2048 1.76 -> 1.48 ms, 512 -> 128 1.74 -> 1.52,
    // 512 -> 256 2.00 -> 1.88, 1024 -> 256 2.88 -> 2.76, 2048 -> 512 1.13 -> 0.90, fc6 (K = 12544) 6.41 -> 6.24 (264 TFLOP/s), and
    // 128 -> 512 leaves the fp32 kernels for it (4.06 -> 3.74); 64 -> 256 stayed there in round 4 (5.59 vs 5.91: profiles/r04_product_kernel_forms.txt).
    // Round 5, after the rewrite of this kernel (pixels by DMA, three stages): 64 -> 256 at 160x272 5.60 -> 4.74 ms per 64 frames (4.08 -> 4.81 TB/s
    // algorithmic), HRNet's 64 -> 256 at 96x72 2.34 -> 2.01 ms per 128 samples, same box -- the floor is 64 input channels now.
    const bool product = gemm8_on && p.taps == 1 && p.cin >= gemm4_min_c && a.Cout % 128 == 0;
    // 1x1 layers with Cout % 128 == 0: the product kernel.  Others: the tap kernel's one-tap form wins from ~1024 input
    // channels only (its 256 x 64 tile re-reads X Cout / 64 times; below, the fp32 kernel's smaller tiles do as well or better).
    // Round 5 (fp16 form): ONE 64-channel column reads X once, and then the one-tap form beats the float32 kernel from 256 input
    // channels on large maps -- 256 -> 64 at 160x272 1.88 -> 1.62 ms per 64 frames, at 96x72 0.92 -> 0.83 per 128 samples; 12x9 maps
    // (384 -> 48: 0.05 -> 0.11) and the 16-channel RPN maps lose and stay where they were.
    const bool one_column = p.f16 && p.cin >= 256 && a.Cout > 32 && a.Cout <= 64 && a.HWout >= 4096;   // (per SAMPLE: the choice must not depend on the batch)
    if (p.taps == 1 && p.cin < gemm_min_cin && !one_column && !product) return p;
    // res1: the output's own shape, or a coarser map read with >> shift (FPN's lat[i-1] += up(lat[i]), fused as a shifted read)
    const bool res1_plain = !a.res1 || (a.res1_off_w == 0 && a.res1_shift >= 0 && a.res1_shift <= 4 &&
                                        ((a.Hout - 1) >> a.res1_shift) < a.res1_H && ((a.Wout - 1) >> a.res1_shift) < a.res1_W &&
                                        (a.res1_shift > 0 || (a.res1_H == a.Hout && a.res1_W == a.Wout)));
    if (!(p.cin % 16 == 0 && a.Cout % 4 == 0 && a.up_log2 == 0 && !a.out_nchw && res1_plain && a.relu <= PP_ACT_SWISH &&
          (a.y_stride == 0 || a.y_stride == a.Cout) && a.y_coff == 0))
        return p;
    // 3x3 stride 1 with 33 .. 48 output channels: conv_split48_kernel (three 16-channel blocks, K = two taps x 16 channels)
    const bool c48 = c48_on && k3 && ((a.Cout > 32 && a.Cout <= 48) || (c48_mult == 1 && a.Cout % 48 == 0) || (c48_mult == 2 && a.Cout == 192));
    // a folded shortcut (ConvArgs::Cin2): only as the second K segment of a plain 1x1 / stride-1 product in the fp16 form
    if (a.Cin2 > 0) {
        if (!(product && p.f16 && k1 && a.stride == 1 && !a.res1 && a.Cin2 % 16 == 0 && a.stride2 >= 1 && a.x_pad == 0 && a.x2_pad == 0 &&
              (a.Hout - 1) * a.stride2 < a.Hin2 && (a.Wout - 1) * a.stride2 < a.Win2))
            return SplitPlan();
        p.cin2 = a.Cin2;
    }
    size_t steps = (size_t)((p.cin + p.cin2) / 16) * p.taps;
    if (product) {
        p.kernel = SPLIT_PRODUCT;
    } else if (!k3 && !s2p) {
        p.kernel = p.taps > 1 ? SPLIT_TAP_GATHER : SPLIT_ONE_TAP;
        p.tile[0].mode = MODE_GEMM;
        p.tile[0].NP = 256;
        p.tile[0].NPp = 260;
    } else if (s2p) {
        p.kernel = SPLIT_S2P;
        p.tile[0] = pick_tile_s2(a.Hout, a.Wout, 13 * 64);
        p.tile[0].mode = MODE_TILE;
    } else if (c48) {
        p.kernel = SPLIT_C48;
        p.ncb = (a.Cout + 47) / 48 * 3;                 // 16-channel blocks, whole columns of 3
        p.nout = p.ncb * 16;
        steps = (size_t)(p.cin / 16) * 5;
        p.tile[0] = tap_tiling(a, 4, stream_env);
    } else {
        p.kernel = SPLIT_TAP3;
        p.tile[0] = tap_tiling(a, 4, stream_env);
        p.tile[1] = tap_tiling(a, 8, stream_env);
    }
    p.frag_bytes = (steps + 1) * p.ncb * wpl * 64 * sizeof(uint4);      // + one spare step: the kernel fetches one step ahead
    p.bytes = p.frag_bytes + (p.f16 ? (size_t)2 * p.nout * sizeof(float) : 0);   // fp16 form: 1 / c, then max |w| per output channel
    if (p.cin2 > 0) {                                   // ... then the summed bias of the two segments
        p.bias_off = (p.bytes + 15) / 16 * 16;
        p.bytes = p.bias_off + (size_t)a.CoutPad * sizeof(float);
    }
    return p;
}

#ifdef PP_SPLIT_TIMELINE
// diagnosis builds: one record buffer, sized for the largest grid; tl_begin hands it to the launch, tl_end synchronises and appends
// "launch header + records" to the file named by $POSEPIPE_SPLIT_TIMELINE (only layers with Cin == $POSEPIPE_SPLIT_TIMELINE_CIN if set)
static unsigned long long* tl_buf = nullptr;
static const size_t TL_MAX_WG = 1 << 19;
static unsigned long long* tl_begin(const ConvArgs& a, hipStream_t stream) {
    static const char* path = getenv("POSEPIPE_SPLIT_TIMELINE");
    static const int only_cin = env_int("POSEPIPE_SPLIT_TIMELINE_CIN", 0);
    static const int max_launches = env_int("POSEPIPE_SPLIT_TIMELINE_MAX", 300);
    static int recorded = 0;
    if (!path || (only_cin && a.Cin != only_cin) || recorded >= max_launches) return nullptr;
    ++recorded;
    if (!tl_buf && hipMalloc(&tl_buf, TL_MAX_WG * 128) != hipSuccess) return nullptr;
    (void)hipMemsetAsync(tl_buf, 0, TL_MAX_WG * 128, stream);
    return tl_buf;
}
static void tl_end(const ConvArgs& a, const SplitArgs& s, const char* kernel, unsigned nwg, hipStream_t stream) {
    if (!s.dbg) return;
    (void)hipStreamSynchronize(stream);
    nwg = std::min<unsigned>(nwg, TL_MAX_WG);
    std::vector<unsigned long long> h((size_t)nwg * 16);
    (void)hipMemcpy(h.data(), tl_buf, h.size() * 8, hipMemcpyDeviceToHost);
    static int launch = 0;
    FILE* f = fopen(getenv("POSEPIPE_SPLIT_TIMELINE"), "ab");
    if (!f) return;
    long long hdr[16] = {0x54494d454c494e45ll, launch++, (long long)nwg, a.N, a.Hout, a.Wout, a.Cin, a.Cout, s.mode, s.nchunks, s.gx, s.gy,
                         a.res1 != nullptr, a.res2 != nullptr, 0, 0};
    memcpy(&hdr[14], kernel, std::min<size_t>(strlen(kernel), 15));
    fwrite(hdr, 8, 16, f);
    fwrite(h.data(), 8, h.size(), f);
    fclose(f);
}
#define PP_TL_BEGIN() s.dbg = tl_begin(a, stream)
#define PP_TL_END(name, nwg) tl_end(a, s, name, nwg, stream)
#else
#define PP_TL_BEGIN()
#define PP_TL_END(name, nwg)
#endif

// the reciprocals the kernels divide by (pp_udiv), from the launch's final geometry
static void fill_divisors(SplitArgs& s) {
    const bool stream_mode = s.mode == MODE_STREAM;
    pp_split_make_magic(stream_mode ? (unsigned)(s.xp_h * s.PWp) : (unsigned)(s.H * s.W), s.dv_per);
    pp_split_make_magic(stream_mode ? (unsigned)s.PWp : (unsigned)s.W, s.dv_row);
    pp_split_make_magic((unsigned)std::max(s.tiles_x, 1), s.dv_tx);
    pp_split_make_magic((unsigned)std::max(s.tiles_y, 1), s.dv_ty);
    pp_split_make_magic((unsigned)std::max(s.PWp, 1), s.dv_pw);
    pp_split_make_magic((unsigned)std::max(s.gy, 1), s.dv_ncol);
    pp_split_make_magic((unsigned)std::max(s.gx >> 3, 1), s.dv_run0);
    pp_split_make_magic((unsigned)((s.gx >> 3) + 1), s.dv_run1);
    pp_split_make_magic((unsigned)std::max(s.ktaps, 1), s.dv_ktaps);
    pp_split_make_magic((unsigned)std::max(s.KW, 1), s.dv_kw);
}

// the plan's pixel tiling (TileGeom) in the launch arguments, and the workgroups it takes for this batch
static unsigned apply_tiling(SplitArgs& s, const TileGeom& g, const ConvArgs& a, int nw) {
    s.mode = g.mode;
    s.NP = g.NP;
    s.NPp = g.NPp;
    if (g.mode == MODE_GEMM) {
        s.S = (long long)a.M;
        return (unsigned)((a.M + 255) / 256);
    }
    s.PWp = g.PWp;
    if (g.mode == MODE_STREAM) {
        s.S = (long long)a.N * s.xp_h * s.xp_w;
        return (unsigned)((s.S + 64 * nw - 1) / (64 * nw));
    }
    s.tiles_x = g.tiles_x; s.tiles_y = g.tiles_y; s.TH = g.TH; s.TW = g.TW; s.bw_log2 = g.bw_log2; s.gx_log2 = g.gx_log2;
    return (unsigned)(g.tiles_x * g.tiles_y * a.N);
}

// the launch's final geometry -- gx pixel tiles x gy channel columns -- in the arguments, with its reciprocals; returns the grid: 2-D, or
// under xcd_remap the 1-D launch of 8 * ceil(gx / 8) * gy ids that xcd_tile_column decodes
static dim3 set_grid(SplitArgs& s, unsigned gx, unsigned gy) {
    s.gx = (int)gx; s.gy = (int)gy;
    fill_divisors(s);
    return s.xcd_remap ? dim3((unsigned)((s.gx + 7) / 8 * 8 * s.gy), 1) : dim3(gx, gy);
}

int pp_launch_conv_split(const SplitPlan& p, const ConvArgs& a, hipStream_t stream) {
    if (a.wsplit && p.kernel == SPLIT_STEM7) return split_launch_stem7(a, stream);
    if (!a.wsplit || p.kernel == SPLIT_NONE) {
        pp_set_error("conv_split: layer not eligible");
        return PP_ERR_ARG;
    }
    // launch-time knobs, read once per process (the product kernel's epilogue also follows pp_debug_knob, per launch)
    static const int colmaj_mb = env_int("POSEPIPE_SPLIT_COLMAJOR_MB", 256), gemm_remap = env_int("POSEPIPE_SPLIT_GEMM_REMAP", 1);
    static const int epi_env = env_int("POSEPIPE_SPLIT_GEMM_EPI", 1), tile_env = env_int("POSEPIPE_SPLIT_GEMM_TILE", 1);
    static const int cob2_env = env_int("POSEPIPE_SPLIT_S2_COB", 0), cob_env = env_int("POSEPIPE_SPLIT_COB", 0);
    static const int nw8_f16 = env_int("POSEPIPE_SPLIT_NW8_F16", 0);
    static const int nw8_min_blocks = env_int("POSEPIPE_SPLIT_NW8_MIN_BLOCKS", 512), nw8_min_chunks = env_int("POSEPIPE_SPLIT_NW8_MIN_CHUNKS", 16);
    static const int ring4_env = env_int("POSEPIPE_SPLIT_RING4", 1), ring48_env = env_int("POSEPIPE_SPLIT_RING48", 1);
    const bool full = p.cin != a.Cin;          // (a folded shortcut's channels are SplitPlan::cin2, not part of p.cin)
    SplitArgs s{};
    s.x = a.x; s.w = (const uint4*)a.wsplit; s.bias = a.bias; s.res1 = a.res1; s.res2 = a.res2; s.y = a.y;
    s.N = a.N; s.H = a.Hout; s.W = a.Wout; s.Cin = p.cin; s.Cout = a.Cout;
    s.ncb = p.ncb;
    s.xp_h = full ? 1 : a.Hin + a.x_pad;
    s.xp_w = full ? 1 : a.Win + a.x_pad;
    s.stride = a.stride;
    s.y_pad = a.y_pad; s.r1_pad = a.r1_pad; s.r2_pad = a.r2_pad; s.relu = a.relu;
    s.r1_shift = a.res1 ? a.res1_shift : 0;
    s.r1_H = a.res1 ? a.res1_H : a.Hout;
    s.r1_W = a.res1 ? a.res1_W : a.Wout;
    s.nchunks = (p.cin + p.cin2) / 16;
    s.seg1 = p.cin / 16;
    if (p.cin2 > 0) {
        if (p.cin2 != a.Cin2 || !a.x2 || !a.x2_amax || p.kernel != SPLIT_PRODUCT || !p.f16 || a.res1) {
            pp_set_error("conv_split: the plan has a folded shortcut of %d channels, the launch does not match it", p.cin2);
            return PP_ERR_STATE;
        }
        s.x2 = a.x2; s.x2_amax = a.x2_amax; s.Cin2 = a.Cin2; s.stride2 = a.stride2;
        s.xp2_h = a.Hin2 + a.x2_pad; s.xp2_w = a.Win2 + a.x2_pad;
    }
    s.ktaps = 1; s.KW = a.KW; s.pad = a.pad_h; s.Hin = a.Hin; s.Win = a.Win;
    if (p.kernel == SPLIT_TAP_GATHER) {     // a step per (chunk, tap), weights in the same [chunk][tap] order
        s.ktaps = p.taps;
        s.nchunks = (p.cin / 16) * p.taps;
    }
    s.x_bytes = a.x_bytes;
    s.xcd_remap = a.xcd_remap;
    const bool f16 = p.f16 != 0;
    const int xp = f16 ? 2 : 3;              // activation planes in LDS
    const int wpl = f16 ? 2 : 3;             // weight planes per fragment set
    s.wscale = f16 ? reinterpret_cast<const float*>(static_cast<const unsigned char*>(a.wsplit) + p.frag_bytes) : nullptr;
    s.x_amax = a.x_amax;
    s.y_amax = a.y_amax;
    if (f16 && !a.x_amax) {
        pp_set_error("conv_split: the fp16 form needs the per-sample maximum of its input (ConvArgs::x_amax)");
        return PP_ERR_STATE;
    }
    PP_TL_BEGIN();
    // inputs beyond the Infinity Cache (256 MB): the columns of a tile back to back; smaller ones: column by column
    s.col_major = (size_t)a.x_bytes <= (size_t)colmaj_mb << 20;
    const char* tag;
    dim3 grid;
    if (p.kernel == SPLIT_PRODUCT) {
        s.mode = MODE_GEMM;
        s.S = (long long)a.M;
        s.col_major = 0;                     // the product kernel walks tile by tile, all columns of a tile back to back
        const int BM = 256, BN = 128;
        s.xcd_remap = gemm_remap && a.Cout / BN > 1;
        grid = set_grid(s, (unsigned)((a.M + BM - 1) / BM), (unsigned)(a.Cout / BN));
        // 1 = epilogue transposed through LDS (18 KiB per wave), 0 = from registers: two store orders of the SAME values (bit-identical,
        // tests/test_gpu_split.py A/Bs them in one process through pp_debug_knob("split_gemm_epilogue", ..)); POSEPIPE_SPLIT_GEMM_EPI is
        // read ONCE per process -- no environment scan per launch
        const int epi_knob = g_split_gemm_epi.load(std::memory_order_relaxed);
        s.epi_lds = epi_knob >= 0 ? epi_knob : epi_env;
        const int nwave = 4;
        // fp16 form: three raw float32 pixel stages of BM x 64 B + three weight stages; six-product form: two stages of split planes + weights
        const size_t lds_loop = f16 ? (size_t)3 * BM * 64 + (size_t)3 * BN * 2 * wpl * 16 : (size_t)2 * (xp * 2 * (BM + 4) * 16 + BN * 2 * wpl * 16);
        const size_t lds = std::max<size_t>(lds_loop, s.epi_lds ? (size_t)nwave * (16384 + 2048) : 0);
        // fp16 form: 1 = the four waves 4 x 1 with 64 x 128 wave tiles (each activation converted once per workgroup), 0 = 2 x 2 with
        // 128 x 64: two arrangements of the SAME sums (bit-identical, tests/test_gpu_split_gemm_tile.py; pp_debug_knob("split_gemm_wave_tile", ..))
        const int tile_knob = g_split_gemm_tile.load(std::memory_order_relaxed);
        split_launch_gemm(f16, p.cin2 > 0, (tile_knob >= 0 ? tile_knob : tile_env) != 0, grid, lds, stream, s);
        tag = "g256x128";
    } else if (p.kernel == SPLIT_S2P) {
        // strided-patch form: 128-pixel tiles, one pixel block per wave, 1 .. 4 channel blocks per wave (the widest the block count and
        // the LDS budget allow: every column stages the patch again)
        if (p.tile[0].eff < 0) {
            pp_set_error("conv_split: no strided-patch tile for a %dx%d map", a.Hout, a.Wout);
            return PP_ERR_STATE;
        }
        const unsigned gx = apply_tiling(s, p.tile[0], a, 4);
        s.SP = (s.TH + 1) * s.PWp;
        int cob = 1;
        for (int c : {4, 3, 2})
            if (s.ncb % c == 0 && (size_t)2 * 2 * s.NPp * 16 + (size_t)4 * c * 2 * 1024 <= 80 * 1024 && (cob2_env == 0 || cob2_env == c)) {
                cob = c;
                break;
            }
        grid = set_grid(s, gx, (unsigned)(s.ncb / cob));
        pp_split_make_magic((unsigned)s.SP, s.dv_row);          // (this form decodes a patch slot into (phase, row, column): dv_row = 1 / SP)
        const size_t lds = (size_t)2 * 2 * s.NPp * 16 + (size_t)4 * cob * 2 * 1024;
        split_launch_tap_s2p((s.NP + 63) / 64, cob, grid, lds, stream, s);
        tag = "s2p";
    } else if (p.kernel == SPLIT_C48) {
        // three 16-channel blocks per workgroup on v_mfma_f32_16x16x32_bf16; Cout / 48 channel columns
        const unsigned gx = apply_tiling(s, p.tile[0], a, 4);
        grid = set_grid(s, gx, (unsigned)(s.ncb / 3));
        // fp16 form: weights through a 4-slot LDS ring (3 blocks x 2 planes = 6 KB per pair-step) where patch + ring leave two workgroups per CU
        const size_t patch48 = (size_t)2 * xp * 2 * s.NPp * 16;
        const bool ring48 = f16 && ring48_env && patch48 + (size_t)4 * 3 * wpl * 1024 <= 80 * 1024;
        const size_t lds = patch48 + (ring48 ? (size_t)4 * 3 * wpl * 1024 : 0);
        split_launch_c48((s.NP + 63) / 64, f16, ring48, grid, lds, stream, s);
        tag = "c48";
    } else {
        // the tap kernel: 3x3 stride 1 (tile or stream), or its product form (one-tap, tap-gather).  Channel blocks (32 output channels)
        // per wave = per workgroup column.  fp16 form, 4-wave ring kernels: THREE where the block count allows and enough workgroups
        // remain (96 / 192 channels of HRNet-W48): 10 fragment reads per 18 MFMAs and wave instead of 6 per 6 (96 channels ran with ONE
        // block per workgroup: three columns, each staging the patch again) or 8 per 12.  Same-box A/B (profile_net w48 128): 96 -> 96 at
        // 48x36 292 -> 315 TFLOP/s, 192 -> 192 at 24x18 328 -> 349; 384 -> 384 at 12x9 LOSES (296 -> 227: 308 workgroups on 512 slots) --
        // hence the workgroup floor below.  FOUR blocks (128, 256, 512 channels: the detector's 3x3 layers; 12 reads per 24 MFMAs, half
        // the patch staging per output): 128 accumulator registers leave room for ONE weight register set (WSETS; with two the K loop
        // spilled: 442 -> 215 TFLOP/s) -- 256 -> 256 at 160x272 429 -> 455 TFLOP/s, 80x136 409 -> 426, 40x68 386 -> 394.
        const bool tap3 = p.kernel == SPLIT_TAP3;
        int cob = (s.ncb & 1) ? 1 : 2;
        if (tap3 && f16 && s.ncb % 3 == 0 && (cob_env == 0 || cob_env == 3)) cob = 3;
        else if (tap3 && f16 && s.ncb % 4 == 0 && (cob_env == 0 || cob_env == 4)) cob = 4;
        // fp16 form: the 4-wave ring form everywhere.  With half the matrix work per tap both forms sit at the same ~420 TFLOP/s on the
        // long-K layers (LDS bandwidth: 8 b128 fragment reads per 12 MFMAs and wave), and two workgroups per CU hide each other's per-tap
        // barrier: same-box A/B (profile_net det 64) 256 -> 256 at 160x272 414.7 -> 418.9, 80x136 366 -> 400, 40x68 354 -> 371 TFLOP/s.
        // The 8-wave form (512-pixel tiles, one workgroup per CU) where it gives ~2 workgroups per CU, else the 4-wave form (256-pixel
        // tiles, two per CU).  Measured on real activations (zeros clock ~15 % higher and mislead): 256 -> 256 at 160x272 207 -> 227
        // TFLOP/s, at 40x68 186 -> 199; but 128 -> 128 189 -> 182 and HRNet's 48 / 96-channel layers -8 %: the per-tap barrier and the
        // three-DMA start-up want >= 16 chunks to pay off
        int nw = tap3 && (!f16 || nw8_f16) ? 8 : 4;
        unsigned gx = apply_tiling(s, p.tile[nw == 8], a, nw);
        if (nw == 8 && !((long)gx * (s.ncb / cob) >= nw8_min_blocks && s.nchunks >= nw8_min_chunks)) {
            nw = 4;
            gx = apply_tiling(s, p.tile[0], a, nw);
        }
        const int nslot = (s.NP + 16 * nw - 1) / (16 * nw);     // exactly: only the last patch slot of a thread can be partly outside
        // 4 waves, 3x3: weights through the LDS ring with a single-buffered patch (RING4), two workgroups per CU; three / four blocks per
        // wave exist for the ring kernels only: back to one / two where that form does not apply
        const auto ring_fits = [&](int c) {
            return ring4_env && nw == 4 && s.mode != MODE_GEMM && (size_t)xp * 2 * s.NPp * 16 + (size_t)4 * c * wpl * 1024 <= 80 * 1024;
        };
        if (cob >= 3 && !(ring_fits(cob) && (cob_env >= 3 || (long)gx * (s.ncb / cob) >= 400))) cob = (s.ncb & 1) ? 1 : 2;
        const bool ring = ring_fits(cob);
        grid = set_grid(s, gx, (unsigned)(s.ncb / cob));
        const size_t lds = (size_t)(ring ? 1 : 2) * xp * 2 * s.NPp * 16 + ((nw == 8 || ring) ? (size_t)4 * cob * wpl * 1024 : 0);
        if (s.mode == MODE_GEMM) split_launch_tap_gemm(cob, f16, grid, lds, stream, s);
        else if (nw == 8) split_launch_tap_nw8(nslot, cob, f16, grid, lds, stream, s);
        else if (ring) split_launch_tap_ring4(nslot, cob, f16, grid, lds, stream, s);
        else split_launch_tap_nw4(nslot, cob, f16, grid, lds, stream, s);
        tag = s.mode == MODE_GEMM ? "gemm4" : nw == 8 ? "nw8" : ring ? "ring4" : "nw4";
    }
    PP_TL_END(tag, grid.x * grid.y);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        pp_set_error("conv_split (%s) launch failed: %s", tag, hipGetErrorString(e));
        return PP_ERR_HIP;
    }
    return PP_OK;
}
