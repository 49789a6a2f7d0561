// Weight side of the split convolutions: the kernels that write a layer's weights in fragment order (pp_conv_split_weights), and the
// stand-alone per-sample maximum (pp_launch_amax).  Layouts are described with the kernels that read them (conv_split*.hip).
// Also the strided-patch instances of the tap kernel (at the end), which the compiler translates as it always did only beside amax_kernel.
#include <algorithm>
#include <vector>

#include "conv_split_tap.h"

namespace {

// fp16 form: the two weight planes of one value under its channel's normalisation c = 2^e (g0 = f16(w c), g1 = f16(w c - g0));
// cmax = max |w| of the output channel (0: an all-zero channel, c = 1)
__device__ __forceinline__ float channel_scale(float cmax) {
    if (!(cmax > 0.f) || !(cmax < 3.0e38f)) return 1.f;
    int e;
    (void)frexpf(cmax, &e);                    // cmax = m 2^e, m in [0.5, 1)  ->  cmax 2^(15 - e) in [2^14, 2^15)
    return ldexpf(1.f, 15 - e);
}
__device__ __forceinline__ void split_weight_h(float v, float c, unsigned short& q0, unsigned short& q1, unsigned short& q2) {
    const float vs = v * c;                    // exact (power of two; |vs| < 2^15)
    const _Float16 g0 = (_Float16)vs;
    const float r = vs - (float)g0;            // exact
    const _Float16 g1 = (_Float16)r;
    q0 = __builtin_bit_cast(unsigned short, g0);
    q1 = __builtin_bit_cast(unsigned short, g1);
    q2 = 0;                                    // (no third plane in this form)
}
// max |w| per output channel of a packed conv weight ([K / 32][CoutPad][32]); one wave per channel; also writes 1 / c
__global__ __launch_bounds__(64) void weight_channel_max_kernel(const float* w, int kchunks, int CoutPad, int nout, float* cmax, float* inv_scale) {
    const int cout = blockIdx.x, lane = threadIdx.x;
    float m = 0.f;
    if (cout < CoutPad)
        for (int c = lane >> 5; c < kchunks; c += 2) m = fmaxf(m, fabsf(w[((size_t)c * CoutPad + cout) * 32 + (lane & 31)]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0 && cout < nout) {
        cmax[cout] = m;
        inv_scale[cout] = 1.f / channel_scale(m);
    }
}

// split weights of the 48-channel form: [chunk][pair][16-channel block][plane][lane] x 16 B; lane = (k group g = lane >> 4: tap
// 2 * pair + (g >> 1), channels 8 (g & 1) .. + 7 of the chunk; channel block row lane & 15); tap 9 (the odd half of pair 4) is zero
template <bool H>
__global__ __launch_bounds__(256) void split_weights48_kernel(const float* w, uint4* out, int Cin, int CoutPad, int ncb16, size_t total, const float* cmax) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;       // (chunk, pair, cb, lane)
    if (i >= total) return;
    const int lane = (int)(i & 63);
    size_t r = i >> 6;
    const int cb = (int)(r % ncb16);
    r /= ncb16;
    const int pair = (int)(r % 5);
    const int c = (int)(r / 5);
    const int g = lane >> 4;
    const int t = 2 * pair + (g >> 1);
    const int cout = cb * 16 + (lane & 15);
    unsigned short h[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int cin = c * 16 + (g & 1) * 8 + j;
        const int k = t * Cin + cin;
        float v = 0.f;
        if (t < 9 && cout < CoutPad) v = w[((size_t)(k >> 5) * CoutPad + cout) * 32 + 8 * (k & 3) + ((k & 31) >> 2)];
        if constexpr (H) {
            split_weight_h(v, channel_scale(cmax[cout]), h[0][j], h[1][j], h[2][j]);
            continue;
        }
        const __bf16 q0 = (__bf16)v;
        const float r1 = v - (float)q0;
        const __bf16 q1 = (__bf16)r1;
        const float r2 = r1 - (float)q1;
        const __bf16 q2 = (__bf16)r2;
        h[0][j] = __builtin_bit_cast(unsigned short, q0);
        h[1][j] = __builtin_bit_cast(unsigned short, q1);
        h[2][j] = __builtin_bit_cast(unsigned short, q2);
    }
    constexpr int WPL = H ? 2 : 3;
    const size_t frag = (i >> 6) * WPL;
#pragma unroll
    for (int pl = 0; pl < WPL; ++pl) {
        uint4 o;
        o.x = h[pl][0] | ((unsigned)h[pl][1] << 16);
        o.y = h[pl][2] | ((unsigned)h[pl][3] << 16);
        o.z = h[pl][4] | ((unsigned)h[pl][5] << 16);
        o.w = h[pl][6] | ((unsigned)h[pl][7] << 16);
        out[(frag + pl) * 64 + lane] = o;
    }
}

// ---- weight split: float32 blob rows ([K / 32][CoutPad][32], pack_conv order) -> fragment order, three bf16 planes ---------
template <bool H>
__global__ __launch_bounds__(256) void split_weights_kernel(const float* w, uint4* out, int Cin, int taps, int CoutPad, int ncb,
                                                            size_t total, const float* cmax) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;       // (chunk, tap, cb, lane)
    if (i >= total) return;
    const int lane = (int)(i & 63);
    size_t r = i >> 6;
    const int cb = (int)(r % ncb);
    r /= ncb;
    const int t = (int)(r % taps);
    const int c = (int)(r / taps);
    const int cout = cb * 32 + (lane & 31);
    unsigned short h[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int cin = c * 16 + (lane >> 5) * 8 + j;
        const int k = t * Cin + cin;
        float v = 0.f;
        if (cout < CoutPad) v = w[((size_t)(k >> 5) * CoutPad + cout) * 32 + 8 * (k & 3) + ((k & 31) >> 2)];
        if constexpr (H) {
            split_weight_h(v, channel_scale(cmax[cout]), h[0][j], h[1][j], h[2][j]);
            continue;
        }
        // round-to-nearest-even split (see split4): planes 1 and 2 are signed residuals
        const __bf16 q0 = (__bf16)v;
        const float r1 = v - (float)q0;                                      // exact
        const __bf16 q1 = (__bf16)r1;
        const float r2 = r1 - (float)q1;                                     // exact, <= 8 significant bits
        const __bf16 q2 = (__bf16)r2;                                        // exact
        h[0][j] = __builtin_bit_cast(unsigned short, q0);
        h[1][j] = __builtin_bit_cast(unsigned short, q1);
        h[2][j] = __builtin_bit_cast(unsigned short, q2);
    }
    constexpr int WPL = H ? 2 : 3;
    const size_t frag = (i >> 6) * WPL;
#pragma unroll
    for (int pl = 0; pl < WPL; ++pl) {
        uint4 o;
        o.x = h[pl][0] | ((unsigned)h[pl][1] << 16);
        o.y = h[pl][2] | ((unsigned)h[pl][3] << 16);
        o.z = h[pl][4] | ((unsigned)h[pl][5] << 16);
        o.w = h[pl][6] | ((unsigned)h[pl][7] << 16);
        out[(frag + pl) * 64 + lane] = o;
    }
}

// the packed weights ([K / 32][CoutPad][32], pack_conv order) of two 1x1 layers onto the same output channels as ONE layer over the
// concatenated input channels (a folded shortcut: w over cin0 channels, then w2 over cin1); rows past cin0 + cin1 are zero
__global__ __launch_bounds__(256) void concat_weights_kernel(const float* w, const float* w2, float* out, int cin0, int cin1, int CoutPad, size_t total) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;       // element of the output blob
    if (i >= total) return;
    const int e = (int)(i & 31), cout = (int)((i >> 5) % CoutPad);
    const int k = (int)((i >> 5) / CoutPad) * 32 + (e & 7) * 4 + (e >> 3);          // inverse of 8 * (k & 3) + ((k & 31) >> 2)
    auto at = [&](const float* src, int kk) { return src[((size_t)(kk >> 5) * CoutPad + cout) * 32 + 8 * (kk & 3) + ((kk & 31) >> 2)]; };
    out[i] = k < cin0 ? at(w, k) : k < cin0 + cin1 ? at(w2, k - cin0) : 0.f;
}

// split weights of the stem: fragment (step s, channel block cb, plane) at ((s * 2 + cb) * 2 + plane) * 64 + lane; lane = (channel
// cb * 32 + (lane & 31), k half lane >> 5); its 8 values: k = 16 s + 8 half + j -> dy = s >> 1, dx = 4 (s & 1) + 2 half + (j >> 2), c = j & 3
__global__ __launch_bounds__(256) void split_weights_stem7_kernel(const float* w, uint4* out, int CoutPad, const float* cmax) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // (s, cb, lane)
    if (i >= STEM_STEPS * 2 * 64) return;
    const int lane = i & 63, cb = (i >> 6) & 1, s = i >> 7;
    const int cout = cb * 32 + (lane & 31);
    unsigned short h[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int dy = s >> 1, dx = 4 * (s & 1) + 2 * (lane >> 5) + (j >> 2), c = j & 3;
        float v = 0.f;
        if (dx < 7) {
            const int k = (dy * 7 + dx) * 4 + c;
            v = w[((size_t)(k >> 5) * CoutPad + cout) * 32 + 8 * (k & 3) + ((k & 31) >> 2)];
        }
        unsigned short q2;
        split_weight_h(v, channel_scale(cmax[cout]), h[0][j], h[1][j], q2);
    }
#pragma unroll
    for (int pn = 0; pn < 2; ++pn) {
        uint4 o;
        o.x = h[pn][0] | ((unsigned)h[pn][1] << 16);
        o.y = h[pn][2] | ((unsigned)h[pn][3] << 16);
        o.z = h[pn][4] | ((unsigned)h[pn][5] << 16);
        o.w = h[pn][6] | ((unsigned)h[pn][7] << 16);
        out[(size_t)(((s * 2 + cb) * 2 + pn) * 64 + lane)] = o;
    }
}

}  // namespace

// a folded shortcut (SplitPlan::cin2): the two layers' weights are concatenated along K into a temporary blob and split as ONE layer
// -- one scale per output channel over both segments, fragments in stage order -- and the biases are added in float32 on the host
static int split_weights_folded(const SplitPlan& p, const ConvArgs& a, void* out, hipStream_t stream) {
    const int kcat = p.cin + p.cin2, kpad = (kcat + 31) / 32 * 32;
    const size_t total = (size_t)kpad * a.CoutPad;
    float* cat = nullptr;
    PP_HIP_CHECK(hipMalloc((void**)&cat, total * sizeof(float)));
    hipLaunchKernelGGL(concat_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a.w, a.w2, cat, p.cin, p.cin2, a.CoutPad, total);
    SplitPlan q = p;
    q.cin = kcat;
    q.cin2 = 0;
    ConvArgs b = a;
    b.w = cat;
    b.Cin = kcat; b.K = kcat; b.Kpad = kpad;
    int rc = pp_conv_split_weights(q, b, out, stream);
    std::vector<float> b0(a.CoutPad), b1(a.CoutPad);
    hipError_t e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipMemcpy(b0.data(), a.bias, b0.size() * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(b1.data(), a.bias2, b1.size() * sizeof(float), hipMemcpyDeviceToHost);
    for (size_t i = 0; i < b0.size(); ++i) b0[i] += b1[i];
    if (e == hipSuccess) e = hipMemcpy(static_cast<unsigned char*>(out) + p.bias_off, b0.data(), b0.size() * sizeof(float), hipMemcpyHostToDevice);
    (void)hipFree(cat);
    if (rc == PP_OK && e != hipSuccess) {
        pp_set_error("split_weights (folded shortcut) failed: %s", hipGetErrorString(e));
        rc = PP_ERR_HIP;
    }
    return rc;
}

int pp_conv_split_weights(const SplitPlan& p, const ConvArgs& a, void* out, hipStream_t stream) {
    if (p.cin2 > 0) return split_weights_folded(p, a, out, stream);
    float* cmax = nullptr;
    if (p.f16) {
        float* inv_scale = reinterpret_cast<float*>(static_cast<unsigned char*>(out) + p.frag_bytes);
        cmax = inv_scale + p.nout;
        hipLaunchKernelGGL(weight_channel_max_kernel, dim3((unsigned)p.nout), dim3(64), 0, stream, a.w, a.Kpad / 32, a.CoutPad, p.nout, cmax, inv_scale);
    }
    const char* what = "split_weights";
    if (p.kernel == SPLIT_STEM7) {
        what = "split_weights_stem7";
        hipLaunchKernelGGL(split_weights_stem7_kernel, dim3((STEM_STEPS * 2 * 64 + 255) / 256), dim3(256), 0, stream, a.w, (uint4*)out, a.CoutPad, cmax);
    } else if (p.kernel == SPLIT_C48) {
        what = "split_weights48";
        const size_t total = (size_t)(p.cin / 16) * 5 * p.ncb * 64;
        const dim3 grid((unsigned)((total + 255) / 256));
        if (p.f16) hipLaunchKernelGGL(split_weights48_kernel<true>, grid, dim3(256), 0, stream, a.w, (uint4*)out, p.cin, a.CoutPad, p.ncb, total, cmax);
        else hipLaunchKernelGGL(split_weights48_kernel<false>, grid, dim3(256), 0, stream, a.w, (uint4*)out, p.cin, a.CoutPad, p.ncb, total, cmax);
    } else {
        const size_t total = (size_t)(p.cin / 16) * p.taps * p.ncb * 64;
        const dim3 grid((unsigned)((total + 255) / 256));
        if (p.f16) hipLaunchKernelGGL(split_weights_kernel<true>, grid, dim3(256), 0, stream, a.w, (uint4*)out, p.cin, p.taps, a.CoutPad, p.ncb, total, cmax);
        else hipLaunchKernelGGL(split_weights_kernel<false>, grid, dim3(256), 0, stream, a.w, (uint4*)out, p.cin, p.taps, a.CoutPad, p.ncb, total, cmax);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        pp_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return PP_ERR_HIP;
    }
    return PP_OK;
}

// ---- stand-alone running maximum (pp_amax.h): tensors whose producer has no fused epilogue (program inputs, pools, ...) -----------
__global__ __launch_bounds__(256) void amax_kernel(const float4* x, size_t quads, unsigned per, unsigned* amax) {
    const unsigned n = blockIdx.x / per, part = blockIdx.x - n * per;      // 1-D grid: the RoI head has 64 000 samples
    const float4* xs = x + (size_t)n * quads;
    float m = 0.f;
    for (size_t i = (size_t)part * 256 + threadIdx.x; i < quads; i += (size_t)per * 256) m = fmaxf(m, pp_abs4max(xs[i]));
    __shared__ float red[16];
    const int im[1] = {(int)n};
    const float mm[1] = {m};
    pp_amax_commit_wg<4, 1>(amax, im, mm, (int)n, (int)n, red);
}

int pp_launch_amax(const float* x, int n, size_t elems, unsigned* amax, hipStream_t stream) {
    if (n <= 0 || elems == 0) return PP_OK;
    if (elems % 4 != 0) {
        pp_set_error("amax: %zu floats per sample (a multiple of 4 is required)", elems);
        return PP_ERR_ARG;
    }
    const size_t quads = elems / 4;
    // ~16 KB per workgroup pass; enough workgroups to fill the chip even for a single large sample
    const unsigned per = (unsigned)std::min<size_t>(std::max<size_t>((quads + 1023) / 1024, 1), std::max<size_t>(2048 / (size_t)n, 1));
    hipLaunchKernelGGL(amax_kernel, dim3(per * (unsigned)n), dim3(256), 0, stream, (const float4*)x, quads, per, amax);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        pp_set_error("amax launch failed: %s", hipGetErrorString(e));
        return PP_ERR_HIP;
    }
    return PP_OK;
}

// ---- instances of conv_split_kernel (conv_split_tap.h): the strided-patch forms (3x3 / stride 2, fp16 form, one pixel block per wave) ----
// They are compiled HERE because they and amax_kernel are the two users of pp_amax_commit_wg<4, 1>: in a translation unit without
// amax_kernel one instruction of their epilogue is scheduled into another slot (tools/kernel_isa_diff.py; DESIGN_LOG.md 5t).
// After ANY edit to this file run tools/kernel_isa_diff.py against the tree before it: a change to amax_kernel or to a weight kernel
// can move these 12 kernels.
void split_launch_tap_s2p(int nslot, int cob, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s) {
    with_nslot<10, 11, 13>(nslot, [&](auto ns) { launch_tap<9, 4, true, decltype(ns)::value, true>(cob, true, grid, lds, stream, s); });
}
