// The ops an HRFormer block adds to the layer programs (models/hrformer.py; mmpose 0.x backbones/hrformer.py):
//   PP_OP_DWCONV3X3    depthwise 3x3 convolution (CrossFFN's dw3x3, the strided fuse chains), bit-reproducible
//   PP_OP_LAYERNORM    LayerNorm over the channels of an NHWC map whose buffer may be wider than the real channel count
//   PP_OP_WINDOW_ATTN  7x7 local-window multi-head self-attention with a relative-position bias (LocalWindowSelfAttention)
//   PP_OP_GELU_ADD     out = res1 + gelu(in): the last GELU of the FFN and the residual add
// All float32 on the vector ALU.  Transcendentals (erf, exp) are evaluated in double and rounded once (the header's convention).
// GELU lives only here: the convolution kernels are untouched, so the other networks compile to the code they had.
#include "pp_internal.h"

namespace {

__device__ __forceinline__ float gelu1(float x) {
    const double d = (double)x;
    return (float)(0.5 * d * (1.0 + erf(d * 0.70710678118654752440)));
}
__device__ __forceinline__ float4 gelu4(const float4 v) { return make_float4(gelu1(v.x), gelu1(v.y), gelu1(v.z), gelu1(v.w)); }
__device__ __forceinline__ float4 relu4(const float4 v) {
    return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}
// acc = acc + x * w, the product and the sum each rounded to float32 (no FMA): what tests/hrformer_ref.py restates in numpy
__device__ __forceinline__ void mac4_rn(float4& acc, const float4 x, const float4 w) {
    acc.x = __fadd_rn(acc.x, __fmul_rn(x.x, w.x));
    acc.y = __fadd_rn(acc.y, __fmul_rn(x.y, w.y));
    acc.z = __fadd_rn(acc.z, __fmul_rn(x.z, w.z));
    acc.w = __fadd_rn(acc.w, __fmul_rn(x.w, w.w));
}
__device__ __forceinline__ float4 dw_act(float4 v, int act) {
    if (act == PP_RELU_LAST) return relu4(v);
    if (act == PP_ACT_GELU) return gelu4(v);
    return v;
}

// ---- PP_OP_DWCONV3X3 ---------------------------------------------------------------------------------------------------------
// out[n][oy][ox][c] = act(bias[c] + sum over (ky, kx) in order of x[n][oy * s - 1 + ky][ox * s - 1 + kx][c] * w[ky * 3 + kx][c]);
// taps outside the map are skipped.  One float4 of channels per thread, consecutive threads on consecutive channels.
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const float4* __restrict__ x, const float4* __restrict__ w,
                                                        const float4* __restrict__ bias, float4* __restrict__ y, size_t total,
                                                        int Hin, int Win, int Hout, int Wout, int c4, int stride, int act) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int cc = (int)(i % c4);
    size_t p = i / c4;
    const int ox = (int)(p % Wout);
    p /= Wout;
    const int oy = (int)(p % Hout);
    const size_t n = p / Hout;
    float4 acc = bias[cc];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - 1 + ky;
        if (iy < 0 || iy >= Hin) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * stride - 1 + kx;
            if (ix < 0 || ix >= Win) continue;
            mac4_rn(acc, x[((n * Hin + iy) * Win + ix) * c4 + cc], w[(ky * 3 + kx) * c4 + cc]);
        }
    }
    y[i] = dw_act(acc, act);
}

// the FFN's form: GELU on every input value (fc1's activation) and stride 1.  A workgroup computes 8 x 8 pixels of 4 float4 channel
// groups; the 10 x 10 input patch goes through GELU once on its way into LDS (1.6 double-precision erf per output instead of 9).
// Same arithmetic per output as dwconv3x3_kernel.
constexpr int DW_T = 8, DW_P = DW_T + 2, DW_C = 4;
__global__ __launch_bounds__(256) void dwconv3x3_gelu_in_kernel(const float4* __restrict__ x, const float4* __restrict__ w,
                                                                const float4* __restrict__ bias, float4* __restrict__ y, int H, int W,
                                                                int c4, int tiles_x, int tiles_y, int act) {
    __shared__ float4 tile[DW_P * DW_P * DW_C];
    int t = blockIdx.x;
    const int tx0 = (t % tiles_x) * DW_T;
    t /= tiles_x;
    const int ty0 = (t % tiles_y) * DW_T;
    const size_t n = t / tiles_y;
    const int c0 = blockIdx.y * DW_C;
    for (int idx = threadIdx.x; idx < DW_P * DW_P * DW_C; idx += 256) {
        const int cc = c0 + idx % DW_C, pp = idx / DW_C;
        const int iy = ty0 + pp / DW_P - 1, ix = tx0 + pp % DW_P - 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy >= 0 && iy < H && ix >= 0 && ix < W && cc < c4) v = gelu4(x[((n * H + iy) * W + ix) * c4 + cc]);
        tile[idx] = v;
    }
    __syncthreads();
    const int ci = threadIdx.x % DW_C, cc = c0 + ci, pix = threadIdx.x / DW_C;
    const int py = pix / DW_T, px = pix % DW_T, oy = ty0 + py, ox = tx0 + px;
    if (oy >= H || ox >= W || cc >= c4) return;
    float4 acc = bias[cc];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy - 1 + ky;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            mac4_rn(acc, tile[((py + ky) * DW_P + (px + kx)) * DW_C + ci], w[(ky * 3 + kx) * c4 + cc]);
        }
    }
    y[((n * H + oy) * W + ox) * c4 + cc] = dw_act(acc, act);
}

// ---- PP_OP_LAYERNORM ---------------------------------------------------------------------------------------------------------
// One wave per pixel: the row of c_buf floats stays in registers (up to LN_V float4 per lane), mean and the biased variance of the
// first c_real channels are taken in two passes (sum, then sum of squared deviations), channels >= c_real are written as zeros.
constexpr int LN_V = 4;   // c_buf <= 64 lanes * 4 float4 * 4 = 1024
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
    return v;
}
__global__ __launch_bounds__(256) void layernorm_nhwc_kernel(const float4* __restrict__ x, const float4* __restrict__ gamma,
                                                             const float4* __restrict__ beta, float4* __restrict__ y,
                                                             size_t rows, int c_real, int c4) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                          // (whole waves leave: no barrier below)
    const int lane = threadIdx.x & 63;
    const float eps = reinterpret_cast<const float*>(beta)[4 * c4];      // the float behind beta[c_buf]
    float4 v[LN_V];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < LN_V; ++k) {
        const int q = lane + 64 * k;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < c4) {
            v[k] = x[row * c4 + q];
            const int c = 4 * q;                      // channels >= c_real take no part in the statistics, whatever they hold
            if (c + 0 >= c_real) v[k].x = 0.f;
            if (c + 1 >= c_real) v[k].y = 0.f;
            if (c + 2 >= c_real) v[k].z = 0.f;
            if (c + 3 >= c_real) v[k].w = 0.f;
            s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
        }
    }
    const float mean = wave_sum(s) / (float)c_real;
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < LN_V; ++k) {
        const int c = 4 * (lane + 64 * k);
        const float a = v[k].x - mean, b = v[k].y - mean, cz = v[k].z - mean, d = v[k].w - mean;
        float t = 0.f;
        if (c + 0 < c_real) t += a * a;
        if (c + 1 < c_real) t += b * b;
        if (c + 2 < c_real) t += cz * cz;
        if (c + 3 < c_real) t += d * d;
        d2 += t;
    }
    const float rstd = 1.f / sqrtf(wave_sum(d2) / (float)c_real + eps);
#pragma unroll
    for (int k = 0; k < LN_V; ++k) {
        const int q = lane + 64 * k;
        if (q >= c4) continue;
        const int c = 4 * q;
        const float4 g = gamma[q], b = beta[q];
        float4 o;
        o.x = c + 0 < c_real ? (v[k].x - mean) * rstd * g.x + b.x : 0.f;
        o.y = c + 1 < c_real ? (v[k].y - mean) * rstd * g.y + b.y : 0.f;
        o.z = c + 2 < c_real ? (v[k].z - mean) * rstd * g.z + b.z : 0.f;
        o.w = c + 3 < c_real ? (v[k].w - mean) * rstd * g.w + b.w : 0.f;
        y[row * c4 + q] = o;
    }
}

// ---- PP_OP_GELU_ADD ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gelu_add_kernel(const float4* __restrict__ x, const float4* __restrict__ r, float4* __restrict__ y,
                                                       size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float4 v = gelu4(x[i]);
    if (r) {
        const float4 a = r[i];
        v = make_float4(__fadd_rn(a.x, v.x), __fadd_rn(a.y, v.y), __fadd_rn(a.z, v.z), __fadd_rn(a.w, v.w));
    }
    y[i] = v;
}

// ---- PP_OP_WINDOW_ATTN -------------------------------------------------------------------------------------------------------
// One wave per (window, head).  The map is zero-padded to multiples of 7 (pad / 2 in front, the rest behind) BEFORE the qkv Linear
// in mmpose, so a padded token has q = k = v = the Linear's bias: it takes part as a key with k = b_k, v = b_v (read from the blob)
// and its own output row is cropped away.  q, k, v of the window's 49 tokens sit in LDS with the head dim zero-padded to HDP (a
// multiple of 4: float4 broadcast reads of k and v); lane i < 49 owns query i: 49 scores in registers, softmax, p @ v.
constexpr int WA_WS = 7, WA_T = WA_WS * WA_WS, WA_NB = (2 * WA_WS - 1) * (2 * WA_WS - 1);
template <int HDP>
__global__ __launch_bounds__(64) void window_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                         const float* __restrict__ table, const float* __restrict__ bias, int H, int W,
                                                         int cbuf, int creal, int heads, int hd, int nwx, int nwy, int pad_top,
                                                         int pad_left, float scale) {
    constexpr int V = HDP / 4;
    __shared__ float4 qs4[WA_T * V], ks4[WA_T * V], vs4[WA_T * V];
    __shared__ float tb[WA_NB];
    float* qs = reinterpret_cast<float*>(qs4);
    float* ks = reinterpret_cast<float*>(ks4);
    float* vs = reinterpret_cast<float*>(vs4);
    const int tid = threadIdx.x, head = blockIdx.y;
    int wid = blockIdx.x;
    const int wx = wid % nwx;
    wid /= nwx;
    const int wy = wid % nwy;
    const size_t n = wid / nwy;
    const int y0 = wy * WA_WS - pad_top, x0 = wx * WA_WS - pad_left;      // map coordinates of the window's first token
    for (int idx = tid; idx < WA_T * HDP; idx += 64) {
        const int t = idx / HDP, d = idx - t * HDP;
        const int y = y0 + t / WA_WS, x = x0 + t % WA_WS;
        float q = 0.f, k = 0.f, v = 0.f;
        if (d < hd) {
            const int c = head * hd + d;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const float* px = qkv + ((n * H + y) * W + x) * (size_t)(3 * cbuf);
                q = px[c];
                k = px[cbuf + c];
                v = px[2 * cbuf + c];
            } else {                     // a padded token: 0 . W + b = b exactly
                k = bias[cbuf + c];
                v = bias[2 * cbuf + c];
            }
        }
        qs[idx] = q;
        ks[idx] = k;
        vs[idx] = v;
    }
    for (int idx = tid; idx < WA_NB; idx += 64) tb[idx] = table[idx * heads + head];
    __syncthreads();
    if (tid < WA_T) {
        const int yi = tid / WA_WS, xi = tid % WA_WS;
        float4 q[V];
#pragma unroll
        for (int d = 0; d < V; ++d) {
            const float4 a = qs4[tid * V + d];
            q[d] = make_float4(__fmul_rn(a.x, scale), __fmul_rn(a.y, scale), __fmul_rn(a.z, scale), __fmul_rn(a.w, scale));
        }
        // B[i][j] = table[(yi - yj + 6) * 13 + (xi - xj + 6)]
        const int bi = (yi + WA_WS - 1) * (2 * WA_WS - 1) + xi + WA_WS - 1;
        float s[WA_T];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < WA_T; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < V; ++d) {
                const float4 k = ks4[j * V + d];
                acc = fmaf(q[d].x, k.x, acc);
                acc = fmaf(q[d].y, k.y, acc);
                acc = fmaf(q[d].z, k.z, acc);
                acc = fmaf(q[d].w, k.w, acc);
            }
            s[j] = acc + tb[bi - ((j / WA_WS) * (2 * WA_WS - 1) + j % WA_WS)];
            m = fmaxf(m, s[j]);
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < WA_T; ++j) {
            s[j] = (float)exp((double)(s[j] - m));
            sum += s[j];
        }
        float4 o[V];
#pragma unroll
        for (int d = 0; d < V; ++d) o[d] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < WA_T; ++j) {
            const float p = s[j] / sum;
#pragma unroll
            for (int d = 0; d < V; ++d) {
                const float4 v = vs4[j * V + d];
                o[d].x = fmaf(p, v.x, o[d].x);
                o[d].y = fmaf(p, v.y, o[d].y);
                o[d].z = fmaf(p, v.z, o[d].z);
                o[d].w = fmaf(p, v.w, o[d].w);
            }
        }
        // row `tid` of qs was read by this lane alone: reuse it to hand the result to the coalesced store below
#pragma unroll
        for (int d = 0; d < V; ++d) qs4[tid * V + d] = o[d];
    }
    __syncthreads();
    for (int idx = tid; idx < WA_T * HDP; idx += 64) {
        const int t = idx / HDP, d = idx - t * HDP;
        const int y = y0 + t / WA_WS, x = x0 + t % WA_WS;
        if (d < hd && y >= 0 && y < H && x >= 0 && x < W) out[((n * H + y) * W + x) * (size_t)cbuf + head * hd + d] = qs[idx];
    }
    if (head == heads - 1 && creal < cbuf && tid < WA_T) {      // the buffer's padding channels: exact zeros
        const int y = y0 + tid / WA_WS, x = x0 + tid % WA_WS;
        if (y >= 0 && y < H && x >= 0 && x < W)
            for (int c = creal; c < cbuf; ++c) out[((n * H + y) * W + x) * (size_t)cbuf + c] = 0.f;
    }
}

}  // namespace

int pp_launch_dwconv3x3(const float* x, const float* w, const float* bias, float* y, int n, int hin, int win, int c, int stride,
                        int act, int gelu_in, hipStream_t stream) {
    PP_REQUIRE(n > 0 && hin > 0 && win > 0 && c > 0 && (c & 3) == 0, "dwconv3x3: c = %d must be a positive multiple of 4", c);
    PP_REQUIRE(stride == 1 || stride == 2, "dwconv3x3: stride %d (1 or 2)", stride);
    PP_REQUIRE(act == PP_RELU_NONE || act == PP_RELU_LAST || act == PP_ACT_GELU, "dwconv3x3: activation %d (PP_RELU_NONE, PP_RELU_LAST, PP_ACT_GELU)", act);
    PP_REQUIRE(!gelu_in || stride == 1, "dwconv3x3: GELU on the input needs stride 1");
    const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;
    const float4 *x4 = reinterpret_cast<const float4*>(x), *w4 = reinterpret_cast<const float4*>(w), *b4 = reinterpret_cast<const float4*>(bias);
    if (gelu_in) {
        const int tx = (win + DW_T - 1) / DW_T, ty = (hin + DW_T - 1) / DW_T;
        PP_REQUIRE((size_t)n * tx * ty < ((size_t)1 << 31), "dwconv3x3: too many tiles");
        hipLaunchKernelGGL(dwconv3x3_gelu_in_kernel, dim3((unsigned)(n * tx * ty), (unsigned)((c / 4 + DW_C - 1) / DW_C)), dim3(256), 0, stream,
                           x4, w4, b4, reinterpret_cast<float4*>(y), hin, win, c / 4, tx, ty, act);
    } else {
        const size_t total = (size_t)n * ho * wo * (c / 4);
        PP_REQUIRE((total + 255) / 256 < ((size_t)1 << 31), "dwconv3x3: too many outputs");
        hipLaunchKernelGGL(dwconv3x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x4, w4, b4,
                           reinterpret_cast<float4*>(y), total, hin, win, ho, wo, c / 4, stride, act);
    }
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_launch_layernorm_nhwc(const float* x, const float* gamma, const float* beta_eps, float* y, size_t rows, int c_real,
                             int c_buf, hipStream_t stream) {
    PP_REQUIRE(rows > 0 && c_real > 0 && c_real <= c_buf && (c_buf & 3) == 0 && c_buf <= 256 * LN_V,
               "layernorm: %d real channels of %d (a multiple of 4, at most %d)", c_real, c_buf, 256 * LN_V);
    PP_REQUIRE((rows + 3) / 4 < ((size_t)1 << 31), "layernorm: too many rows");
    hipLaunchKernelGGL(layernorm_nhwc_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<const float4*>(gamma), reinterpret_cast<const float4*>(beta_eps), reinterpret_cast<float4*>(y),
                       rows, c_real, c_buf / 4);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_launch_gelu_add(const float* x, const float* res, float* y, size_t elems, hipStream_t stream) {
    PP_REQUIRE(elems > 0 && (elems & 3) == 0 && (elems / 4 + 255) / 256 < ((size_t)1 << 31), "gelu_add: bad element count");
    const size_t total = elems / 4;
    hipLaunchKernelGGL(gelu_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<const float4*>(res), reinterpret_cast<float4*>(y), total);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_window_attn_max_head_dim() { return 64; }

int pp_launch_window_attn(const float* qkv, const float* table, const float* bias, float* out, int n, int h, int w, int c_real,
                          int c_buf, int heads, hipStream_t stream) {
    PP_REQUIRE(n > 0 && h > 0 && w > 0 && heads > 0 && c_real > 0 && c_real % heads == 0 && c_real <= c_buf && (c_buf & 3) == 0,
               "window_attn: %d channels of %d in %d heads", c_real, c_buf, heads);
    const int hd = c_real / heads;
    PP_REQUIRE(hd <= pp_window_attn_max_head_dim(), "window_attn: head dim %d (at most %d)", hd, pp_window_attn_max_head_dim());
    const int nwy = (h + WA_WS - 1) / WA_WS, nwx = (w + WA_WS - 1) / WA_WS;
    const int pad_top = (nwy * WA_WS - h) / 2, pad_left = (nwx * WA_WS - w) / 2;
    PP_REQUIRE((size_t)n * nwy * nwx < ((size_t)1 << 31) && heads < 65536, "window_attn: too many windows");
    const float scale = (float)(1.0 / sqrt((double)hd));
    const dim3 grid((unsigned)(n * nwy * nwx), (unsigned)heads);
#define PP_WA_LAUNCH(HDP)                                                                                                           \
    hipLaunchKernelGGL(window_attn_kernel<HDP>, grid, dim3(64), 0, stream, qkv, out, table, bias, h, w, c_buf, c_real, heads, hd, nwx, \
                       nwy, pad_top, pad_left, scale)
    if (hd <= 8) PP_WA_LAUNCH(8);
    else if (hd <= 40) PP_WA_LAUNCH(40);
    else PP_WA_LAUNCH(64);
#undef PP_WA_LAUNCH
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
