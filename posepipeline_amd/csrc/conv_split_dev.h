// Device pieces shared by the split-conv kernels (conv_split_tap.h, conv_split_c48.hip, conv_split_gemm.hip, conv_split_stem.hip):
// the launch arguments (SplitArgs), the timeline macros, pp_udiv / xcd_tile_column, the operand splits (split4, split2h, split4h),
// split_activate, the lane -> pixel maps, the four-component epilogue steps (relu4, act4, add4) with epi_value / epi_finish built from
// them, the index pieces out_pixels, decode_pos, wg_samples and tile_origin, the chunk request of the patch loader (patch_request) and
// of the weight ring the DMA statement (dma_fragment), ring_read and ring_wait.  Where a kernel keeps its own copy of one of these
// pieces (the compiler's output changed through the shared form), the copy is marked there.  The design narrative is in conv_split.hip.
#pragma once
#include "pp_internal.h"
#include "pp_amax.h"

// timing experiments only (tools/build_variant.sh; WRONG results): 1 no weight loads, 2 no patch staging, 4 no barrier,
// 8 no fragment reads from LDS, 16 no MFMAs in the K loop of conv_split_kernel, 32 no epilogue (one store per lane)
#ifndef PP_SPLIT_ABLATE
#define PP_SPLIT_ABLATE 0
#endif

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

struct SplitArgs {
    const float* x;
    const uint4* w;          // split weights, fragment order
    const float* bias;
    const float* res1;
    const float* res2;
    float* y;
    int N, H, W, Cin, Cout, ncb;          // ncb: 32-channel blocks of the split weights
    int xp_h, xp_w;                       // stored rows per image / pixels per row of the input (dims + halo)
    int y_pad, r1_pad, r2_pad, relu;
    int nchunks;                          // Cin / 16
    int tiles_x, tiles_y, TH, TW, bw_log2, gx_log2;   // MODE_TILE
    int PWp;                              // patch pitch (TILE) / stored row pitch of the input (STREAM), in pixels
    int NP, NPp;                          // patch pixels, padded so that the two k halves are 64 B apart mod 128
    int mode, stride;
    int r1_shift, r1_H, r1_W;             // res1 is read at (y >> r1_shift, x >> r1_shift) of an r1_H x r1_W map (FPN top-down add)
    int ktaps, KW, pad, Hin, Win;         // GEMM with ktaps > 1: a KH x KW (strided) convolution as one product per (channel chunk, tap)
    long long S;                          // STREAM: positions of the padded input stream, GEMM: output pixels
    unsigned x_bytes;
    int xcd_remap;
    int SP;                               // strided-patch form: slots per phase map ((TH + 1) x PWp)
    int gx, gy;                           // xcd_remap: logical grid (pixel tiles, channel columns) of the 1-D launch
    int col_major;                        // xcd_remap: an XCD walks its tiles column by column (small inputs) instead of tile by tile
    int epi_lds;                          // conv_split_gemm_kernel: epilogue transposed through LDS (whole 128-byte lines per store)
    // host-made reciprocals (pp_split_make_magic / pp_udiv) of the divisors of the tap kernels' index arithmetic: round 4's timeline showed
    // the ~700 instructions of a workgroup's set-up -- ten 32 / 64-bit division sequences among them -- taking 3.5 - 5k cycles
    // before the first load was even requested (profiles/r04_w48_timeline_before.txt)
    unsigned dv_per[2], dv_row[2];        // positions per image / per row of the output-coordinate decode (STREAM: the padded input stream)
    unsigned dv_tx[2], dv_ty[2], dv_pw[2];   // MODE_TILE: tiles_x, tiles_y, patch pitch
    unsigned dv_ncol[2], dv_run0[2], dv_run1[2];   // xcd_tile_column: gy, ntiles / 8, ntiles / 8 + 1
    unsigned dv_ktaps[2], dv_kw[2];       // tap-gather product: ktaps, KW
    // fp16 form (H kernels): per-output-channel 1 / c of the weight normalisation (behind the fragments of the split copy) and the
    // running maximum of |x| PER SAMPLE (bit pattern of a non-negative float, pp_amax.h) that the activation scale follows
    const float* wscale;
    const unsigned* x_amax;
    // any form: where to fold max |y| per sample of what this launch stores (null: the output feeds no fp16-form convolution)
    unsigned* y_amax;
    // conv_split_gemm_kernel<.., H, SEG2>: the second K segment (a folded projection shortcut, ConvArgs::x2).  Stages [0, seg1) read x
    // (Cin channels), stages [seg1, nchunks) read x2 (Cin2 channels at stride2 of an xp2_h x xp2_w map); the weight fragments of the
    // two segments follow each other in stage order
    const float* x2;
    const unsigned* x2_amax;
    int Cin2, stride2, xp2_h, xp2_w, seg1;
#ifdef PP_SPLIT_TIMELINE
    unsigned long long* dbg;              // diagnosis builds only (tools/build_variant.sh tl -DPP_SPLIT_TIMELINE): 16 x u64 per workgroup
#endif
};

// Diagnosis builds (-DPP_SPLIT_TIMELINE, never the shipped library): every workgroup of the tap kernels records s_memtime at entry,
// after its prologue, after its K loop and at its end, plus where it ran (HW_ID / XCC_ID); the launcher synchronises after each
// launch and appends the records to $POSEPIPE_SPLIT_TIMELINE (tools/split_timeline.py reads them).
#ifdef PP_SPLIT_TIMELINE
#define PP_TL_DECL unsigned long long tl_t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PP_TL_MARK(i) do { if (a.dbg) tl_t[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define PP_TL_FLUSH()                                                                                                    \
    do {                                                                                                                 \
        if (a.dbg && threadIdx.x == 0) {                                                                                 \
            unsigned hw, xcc;                                                                                            \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                            \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                                          \
            unsigned long long* r = a.dbg + (size_t)blockIdx.x * 16;                                                     \
            r[0] = blockIdx.x; r[1] = ((unsigned long long)xcc << 32) | hw;                                              \
            r[2] = tl_t[0]; r[3] = tl_t[1]; r[4] = tl_t[2]; r[5] = tl_t[3]; r[6] = L; r[7] = col;                       \
            for (int i_ = 4; i_ < 10; ++i_) r[4 + i_] = tl_t[i_];                                                        \
        }                                                                                                                \
    } while (0)
#else
#define PP_TL_DECL
#define PP_TL_MARK(i)
#define PP_TL_FLUSH()
#endif

// n / d for any 32-bit n through the host-made pair {m, sh} = pp_split_make_magic(d) (Granlund - Montgomery: k = ceil(log2 d),
// m = floor(2^32 (2^k - d) / d) + 1, q = (t + ((n - t) >> 1)) >> (k - 1) with t = mulhi(m, n); d == 1 is flagged by sh >= 32):
// five integer instructions instead of the ~40 of a 32-bit and the ~150 of a 64-bit division sequence
__device__ __forceinline__ unsigned pp_udiv(unsigned n, const unsigned (&dv)[2]) {
    const unsigned t = __umulhi(n, dv[0]);
    const unsigned q = (t + ((n - t) >> 1)) >> (dv[1] & 31u);
    return dv[1] >= 32u ? n : q;
}

// Workgroup id -> (tile, channel column) of a 1-D launch of 8 * ceil(ntiles / 8) * ncol ids.  Consecutive ids go round-robin over
// the 8 XCDs (each with its own L2).  XCD x owns a CONTIGUOUS run of tiles (neighbouring tiles share their halo rows in its L2)
// and walks it tile by tile, all channel columns of a tile one after the other: the columns read the same input tile, which
// then comes from HBM once instead of once per column (256 -> 1024 at 40x68 has 8 columns, 512 -> 2048 16).  false: idle id.
// col_major != 0 (small maps: the whole input sits in the Infinity Cache anyway, and what an XCD's L2 should keep is ONE column's
// split weights): the XCD walks its run once per column instead -- measured on HRNet's 192 -> 192 at 24x18: 187 vs 166 TFLOP/s.
__device__ __forceinline__ bool xcd_tile_column(unsigned L, const SplitArgs& a, unsigned& tile, unsigned& col) {
    const unsigned ntiles = (unsigned)a.gx, ncol = (unsigned)a.gy;
    const unsigned xcd = L & 7u, j = L >> 3;
    const unsigned q = ntiles >> 3, r = ntiles & 7u;
    const unsigned run = xcd < r ? q + 1 : q;
    unsigned tj;
    if (a.col_major) {
        if (run == 0) return false;
        col = xcd < r ? pp_udiv(j, a.dv_run1) : pp_udiv(j, a.dv_run0);
        tj = j - col * run;
        if (col >= ncol) return false;
    } else {
        tj = pp_udiv(j, a.dv_ncol);
        col = j - tj * ncol;
        if (tj >= run) return false;
    }
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + tj;
    return true;
}

// Round-to-nearest-even split of four floats into the three bf16 planes (4 x 16 bit each): p0 = bf16(a), p1 = bf16(a - p0),
// p2 = a - p0 - p1.  The residuals are exact float32 values (a - p0 has at most 16 significant bits, a - p0 - p1 at most 8), so
// a = p0 + p1 + p2 EXACTLY, as with a truncating split -- but the planes below the first are SIGNED with half the magnitude
// (|p1| <= 2^-9 |a|, |p2| <= 2^-17 |a|): the three dropped products p1*q2 + p2*q1 + p2*q2 are ~2^-26 |a q| with random signs.
// Round 2's truncating split kept every plane the sign of a, so on same-sign data (ReLU activations x positive kernels) the
// dropped terms, 2^-22 |a q| on average, all pushed the same way: -2e-7 per layer, -1.3e-5 over HRNet-W48's ~70 layers
// (tests/test_gpu_parity_modes.py found it as a uniform score deficit).  v_cvt_pk_bf16_f32 converts and packs two values per
// instruction: 4.5 vector instructions per element (5.5 with masks and v_perm).  Values within 2^-8 of FLT_MAX would round to
// infinity; activations and weights are nowhere near.
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
__device__ __forceinline__ void split4(const float4 v, uint2& p0, uint2& p1, uint2& p2) {
    const f32x2_t a = {v.x, v.y}, b = {v.z, v.w};
    const bf16x2_t a0 = __builtin_convertvector(a, bf16x2_t), b0 = __builtin_convertvector(b, bf16x2_t);
    const f32x2_t ra = a - __builtin_convertvector(a0, f32x2_t), rb = b - __builtin_convertvector(b0, f32x2_t);          // exact
    const bf16x2_t a1 = __builtin_convertvector(ra, bf16x2_t), b1 = __builtin_convertvector(rb, bf16x2_t);
    const f32x2_t sa = ra - __builtin_convertvector(a1, f32x2_t), sb = rb - __builtin_convertvector(b1, f32x2_t);        // exact, <= 8 bits
    const bf16x2_t a2 = __builtin_convertvector(sa, bf16x2_t), b2 = __builtin_convertvector(sb, bf16x2_t);              // exact
    // a bf16x2 register = (element 2i+1) << 16 | element 2i
    p0 = make_uint2(__builtin_bit_cast(unsigned, a0), __builtin_bit_cast(unsigned, b0));
    p1 = make_uint2(__builtin_bit_cast(unsigned, a1), __builtin_bit_cast(unsigned, b1));
    p2 = make_uint2(__builtin_bit_cast(unsigned, a2), __builtin_bit_cast(unsigned, b2));
}

// ---- fp16 form (round 5): two-term operand split, THREE products per term ------------------------------------------------------
// The six-product form's ceiling is 2500 / 6 = 417 TFLOP/s fp32-equivalent, and two rounds of tuning put the kernels at 0.46 of it
// with the long-K layers at the chip's power limit.  float16 carries 11 significand bits: two terms carry 22,
//     x s = h0 + h1,   h0 = f16(x s),  h1 = f16(x s - h0)     (s: power of two PER SAMPLE, max |x| s in [2^14, 2^15), exact)
//     w c = g0 + g1,   g0 = f16(w c),  g1 = f16(w c - g0)     (c: power of two PER OUTPUT CHANNEL, max |w| c in [2^14, 2^15))
//     (x s)(w c) ~ h0 g0 + h1 g0 + h0 g1                      (dropped: h1 g1 ~ 2^-22 |x w|, random sign)
// -- three v_mfma_f32_32x32x16_f16 (same rate as bf16) into ONE float32 accumulator set, TWO planes per operand (the weight planes
// are a third smaller than the bf16 form's: LDS reads per tap 10 -> 8, weight bytes through L2 / the DMA ring -33 %); the epilogue
// multiplies by 1 / (s c) (exact) inside the bias add's fma.  Representation error: |x s - h0 - h1| <= 2^-22 |x s| wherever the
// residual is a normal float16 (|x s| >= 2^-2, i.e. down to 2^-17 of the sample's maximum) and <= 2^-25 absolutely = 2^-39 of the
// sample's maximum below that -- far under what ONE float32 rounding of the running sum costs (2^-24 of the sum); the weights
// likewise per channel.  Per product that is ~2^-23.7 rms with
// random sign against the ~2^-24 EVERY step of a float32 FMA chain commits on the running sum: over K >= 144 terms the chain's own
// rounding dominates (tests/test_gpu_split.py holds the same yardstick as for the six-product form: error against float64 <= the
// float32 kernel's).  Range of activations: s = 2^k is chosen PER SAMPLE from the running maximum of the tensor (pp_amax.h: the kernel
// that stores a tensor folds max |v| into amax[sample]; max |x| s lies in [2^14, 2^15)), so nothing can leave the format upwards,
// values down to 2^-17 of the sample's maximum keep their 22 bits and smaller ones are off by <= 2^-39 of it -- whatever the
// magnitude of the data (1e-30 .. 1e30 alike).  Non-finite inputs stay non-finite (inf s = inf in float16, NaN stays NaN).
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
// (round 6) two elements -> their (h0, h1) register pair in FOUR instructions: v_fma_mixlo / mixhi_f16 evaluate fma(x, s, c) in float32
// with c read as float16 and round the result into one half of the destination -- h0 = f16(x s + 0), h1 = f16(x s - h0) -- where the
// plain sequence takes six (v_pk_mul, v_cvt_pk_f16_f32, two v_cvt_f32_f16, v_pk_add, v_cvt_pk_f16_f32).  x s is exact (s a power of two)
// and so is the difference: the same bits as before, except the sign of an exact zero (tools/dbg/mix_test.hip: 4M random bit patterns,
// four scales, 0 mismatches).  The split is the VALU work of every fp16-form kernel: the product kernel converts at each fragment read
// (ablation: 3.3 ms of a 105 ms step go into it), the strided-patch kernel stages four input pixels per output (3.6 VALU per MFMA).
__device__ __forceinline__ void split2h(const float x0, const float x1, const float s, unsigned& h0, unsigned& h1) {
    unsigned d, e;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(d) : "v"(x0), "v"(s));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(d) : "v"(x1), "v"(s));
    asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(e) : "v"(x0), "v"(s), "v"(d));
    asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(e) : "v"(x1), "v"(s), "v"(d));
    h0 = d;
    h1 = e;
}
__device__ __forceinline__ void split4h(const float4 v, const float s, uint2& p0, uint2& p1) {
    split2h(v.x, v.y, s, p0.x, p1.x);
    split2h(v.z, v.w, s, p0.y, p1.y);
}

// Activations of the DeepSortYOLOv4 / YOLOX programs, as conv_igemm_p3.hip: every transcendental is evaluated in double precision
// and rounded to float once (what oracle/yolo.py restates); applied like PP_RELU_FIRST: y = res + act(conv + bias).
__device__ __forceinline__ float split_activate(float x, int act) {
    if (act == PP_ACT_LEAKY) return x >= 0.f ? x : 0.1f * x;
    if (act == PP_ACT_MISH) {
        if (x > 20.f) return x;
        const double n = exp((double)x);
        const double t = n * (n + 2.0);
        return x * (float)(t / (t + 2.0));
    }
    if (act == PP_ACT_ELU) return x > 0.f ? x : (float)expm1((double)x);
    if (act == PP_ACT_SWISH) return x * (float)(1.0 / (1.0 + exp(-(double)x)));
    return x;
}

// ds_read_b128 is serviced in the lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (+32): lane -> q such that each
// group is 16 consecutive q.  Pixel blocks narrower than 32 pixels give every group whole rows of the block.
__device__ __forceinline__ int lane_q(int r) {
    const int g1 = ((r >= 4 && r < 12) || (r >= 16 && r < 20) || r >= 28) ? 1 : 0;
    int idx;
    if (!g1) idx = r < 4 ? r : r < 16 ? r - 8 : r - 12;              // 0-3 -> 0-3, 12-15 -> 4-7, 20-27 -> 8-15
    else idx = r < 12 ? r - 4 : r < 20 ? r - 8 : r - 16;             // 4-11 -> 0-7, 16-19 -> 8-11, 28-31 -> 12-15
    return g1 * 16 + idx;
}
// position of block pixel q inside a block of width 32 >> bw_log2 ... (bw_log2: 0 = 1 x 32, 1 = 2 x 16, 2 = 4 x 8 pixels)
__device__ __forceinline__ void block_pixel(int r, int bw_log2, int& iy, int& ix) {
    if (bw_log2 == 0) {
        iy = 0;
        ix = r;
        return;
    }
    const int q = lane_q(r);
    if (bw_log2 == 1) {
        iy = q >> 4;
        ix = q & 15;
    } else {            // rows 0, 2 in the first lane group, 1, 3 in the second (patch pitch = 4 mod 8: conflict-free)
        iy = ((q >> 3) & 1) * 2 + (q >> 4);
        ix = q & 7;
    }
}

// MODE_TILE   3x3 / stride 1 / pad 1 on any buffer: rectangular output tile, patch = tile + 1-pixel frame (bounds-tested loads)
// MODE_STREAM 3x3 / stride 1 / pad 1 on a zero-halo input (pp_buf.pad >= 1): the padded tensor is ONE pixel stream in which tap
//             (dy, dx) of position s is position s + dy * pitch + dx (the halo supplies every out-of-image zero), so a tile is
//             256 CONSECUTIVE stream positions whatever the map's width -- no tile quantisation on HRNet's 36 / 18 / 9-pixel rows;
//             patch = the 256 + 2 pitch + 2 positions around it, loaded without any test; halo positions are not stored
// MODE_GEMM   1x1 (any stride), and 'valid' convs whose kernel covers the whole input (the RoI head's 7x7 fc6, rewritten by
//             the launcher as 1x1 over 49 x 256 channels): tile = 256 consecutive output pixels, one "tap".
//             ktaps > 1 (round 3: 3x3 stride 2): the same product form, one step per (16-channel chunk, tap) -- the operand of a
//             step is the tile's 256 input pixels AT THAT TAP (gathered with the stride, out-of-image taps read as zero through
//             a per-slot validity mask).  No patch reuse between taps (a strided patch is 4x the tile: 117 KB of LDS per stage),
//             so every input element is staged 2.25 times instead of once; at 16 KB per step that is ~17 % of the vector
//             memory path, and the layers leave the fp32 MFMA kernels (95 - 130 TFLOP/s) for this kernel's one-tap rate.
enum { MODE_TILE = 0, MODE_STREAM = 1, MODE_GEMM = 2 };


// ---- four-component steps of the epilogues (in place: the statements the kernels spelled out) ---------------------------------------
__device__ __forceinline__ void relu4(float4& v) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
__device__ __forceinline__ void act4(float4& v, int act) {
    v.x = split_activate(v.x, act); v.y = split_activate(v.y, act); v.z = split_activate(v.z, act); v.w = split_activate(v.w, act);
}
__device__ __forceinline__ void add4(float4& v, const float4& r) { v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }

// The epilogue of four consecutive output channels of one pixel, in two steps (kernels that request their res2 lines in one batch add
// them with add4 between the two).  epi_value: v = accumulators + bias -- fp16 form (H): fma(acc, sc * xi, bias) with sc = 1 / c of the
// channels (SplitArgs::wscale) and xi = 1 / s of the pixel's sample (the products with powers of two are exact: the fma rounds once, like
// the add) --, then PP_RELU_FIRST or the activation `relu` names, then + res1 (has_r1; r1, like sc and xi, is not read otherwise)
template <bool H>
__device__ __forceinline__ void epi_value(float4& v, float c0, float c1, float c2, float c3, const float4& b, const float4& sc, const float& xi,
                                          int relu, bool has_r1, const float4& r1) {
    if constexpr (H) v = make_float4(__builtin_fmaf(c0, sc.x * xi, b.x), __builtin_fmaf(c1, sc.y * xi, b.y), __builtin_fmaf(c2, sc.z * xi, b.z),
                                     __builtin_fmaf(c3, sc.w * xi, b.w));
    else v = make_float4(c0 + b.x, c1 + b.y, c2 + b.z, c3 + b.w);
    if (relu == PP_RELU_FIRST) relu4(v);
    else if (relu >= PP_ACT_LEAKY) act4(v, relu);
    if (has_r1) add4(v, r1);
}
// epi_finish: + res2 (has_r2 / r2 as above), then PP_RELU_LAST: v is what is stored.  NO_R2: what callers without that residual pass
static constexpr float4 NO_R2 = {0.f, 0.f, 0.f, 0.f};
__device__ __forceinline__ void epi_finish(float4& v, int relu, bool has_r2, const float4& r2) {
    if (has_r2) add4(v, r2);
    if (relu == PP_RELU_LAST) relu4(v);
}

// ---- pieces of the kernels' index arithmetic, written once --------------------------------------------------------------------------

// output pixel (sample n, row y, column x) -> its pixel index in y, in res1 (a map of r1_H x r1_W read at (y >> r1_shift, x >> r1_shift))
// and in res2, each buffer with its own halo
__device__ __forceinline__ void out_pixels(const SplitArgs& a, int n, int y, int x, size_t& ypix, size_t& r1pix, size_t& r2pix) {
    ypix = ((size_t)n * (a.H + a.y_pad) + y) * (a.W + a.y_pad) + x;
    r1pix = ((size_t)n * (a.r1_H + a.r1_pad) + (y >> a.r1_shift)) * (a.r1_W + a.r1_pad) + (x >> a.r1_shift);
    r2pix = ((size_t)n * (a.H + a.r2_pad) + y) * (a.W + a.r2_pad) + x;
}

// first and last sample of the `n` positions from s0 on (clamped to the tensor's S): pp_amax_commit_wg's range for a workgroup
__device__ __forceinline__ void wg_samples(const SplitArgs& a, unsigned s0, int n, int& first, int& last) {
    const unsigned l = (unsigned)min((long long)s0 + n - 1, a.S - 1);
    first = (int)pp_udiv(min(s0, l), a.dv_per);
    last = (int)pp_udiv(l, a.dv_per);
}

// position m of the padded input stream (MODE_STREAM) or output pixel m (MODE_GEMM) -> (sample, row, column).  per / row: the
// positions per sample / per row of that mode, whose reciprocals dv_per / dv_row hold; m < S (the callers clamp)
__device__ __forceinline__ void decode_pos(const SplitArgs& a, unsigned m, unsigned per, unsigned row, int& img, int& y, int& x) {
    const unsigned i = pp_udiv(m, a.dv_per), rem = m - i * per;
    const unsigned yy = pp_udiv(rem, a.dv_row);
    img = (int)i;
    y = (int)yy;
    x = (int)(rem - yy * row);
}

// workgroup tile L -> its origin: sample n and corner (x0, y0) in MODE_TILE, else the first of its `tile` stream positions / output
// pixels s0 (32-bit throughout: one launch addresses < 4 GiB of input, so positions and pixels stay below 2^30)
__device__ __forceinline__ void tile_origin(const SplitArgs& a, unsigned L, unsigned tile, int& n, int& x0, int& y0, unsigned& s0) {
    n = x0 = y0 = 0;
    s0 = 0;
    if (a.mode == MODE_TILE) {
        const unsigned L2 = pp_udiv(L, a.dv_tx);
        const int tx = (int)(L - L2 * (unsigned)a.tiles_x);
        n = (int)pp_udiv(L2, a.dv_ty);
        const int ty = (int)(L2 - (unsigned)n * (unsigned)a.tiles_y);
        x0 = tx * a.TW;
        y0 = ty * a.TH;
    } else {
        s0 = L * tile;
    }
}

// ---- the patch loader: only the request of a chunk is shared (48-channel kernel, product kernel's six-product form).  The slot
// offsets of the tile / stream modes and the split-and-write are written out in conv_split_kernel and conv_split48_kernel: as
// functions (stream slots, tile offset, slot split-and-write; parameters by reference) they reordered 4 - 10 of each unit's instances.
// the request of a chunk: 16 bytes per slot at goff[j] + add, masked slots read as zero
template <int NSLOT>
__device__ __forceinline__ void patch_request(const __amdgpu_buffer_rsrc_t& rsrc, const unsigned (&goff)[NSLOT], const unsigned& add, float4 (&xr)[NSLOT]) {
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
        const unsigned off = goff[j] == 0xffffffffu ? 0xffffffffu : goff[j] + add;
        xr[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, 0, 0));
    }
}
// ---- the weight ring: a step's 1 KB weight fragments global -> LDS by the DMA path, slot (step & 3) of four (the kernels issue) -------------------------
// One fragment (64 lanes x 16 B at g) to LDS address dst.  Raw instruction: through the builtin the compiler treats the DMA as a
// possible alias of EVERY later LDS read and orders them behind s_waitcnt vmcnt(0); completion is awaited by the counted waits below.
__device__ __forceinline__ void dma_fragment(const uint4* g, unsigned dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(dst) : "memory", "m0");
}
// ... with a workgroup-uniform base and a 32-bit lane offset (one address register per DMA)
__device__ __forceinline__ void dma_fragment(unsigned voff, const void* sbase, unsigned dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(dst) : "memory", "m0");
}
// a slot's fragments into a register set
template <int CB, int WPL>
__device__ __forceinline__ void ring_read(const unsigned char* smem, unsigned wring, int lane, int step, uint4 (&dst)[CB][WPL]) {
    const unsigned char* base = smem + wring + (step & 3) * (CB * WPL * 1024) + lane * 16;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int pl = 0; pl < WPL; ++pl) dst[cb][pl] = *reinterpret_cast<const uint4*>(base + (cb * WPL + pl) * 1024);
}
// allow `n` (0, NDMA, NSLOT, NSLOT + NDMA) of the youngest vector-memory operations to stay in flight; LGKM: also wait for every LDS
// operation of the wave
template <int NSLOT, int NDMA, bool LGKM>
__device__ __forceinline__ void ring_wait(int n) {
    if constexpr (LGKM) {
        if (n == NSLOT + NDMA) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NSLOT + NDMA) : "memory");
        else if (n == NSLOT) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NSLOT) : "memory");
        else if (n == NDMA) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NDMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    } else {
        if (n == NSLOT + NDMA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSLOT + NDMA) : "memory");
        else if (n == NSLOT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSLOT) : "memory");
        else if (n == NDMA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}
