// PoseFormer (ICCV 2021, the 81-frame model) as the 2D -> 3D lifter behind pose_pipeline/wrappers/poseformer.py (models/poseformer.py):
//   spatial_encoder_kernel   the whole spatial transformer of one frame in one launch: [n][17][2] -> [n][544]
//   PP_OP_ATTENTION          global multi-head self-attention in float32 on a qkv map, tokens <= 128, head dim <= 128
//   window_gather_kernel     win[b][f][:] = feature[i_b + f][:] + Temporal_pos_embed[f][:], the temporal program's input
//   mean_head_kernel         weighted mean over the frame axis + head LayerNorm (eps 1e-5) + Linear 544 -> 51
//   pp_poseformer_lift       spatial stage ONCE over the clip, then the windows in batches: gather -> temporal program -> mean + head
// The reference evaluates the whole network once per 81-frame window; the spatial transformer sees every frame on its own, so its
// result for a frame is the same in every window and is computed once per frame here (81x less spatial work).
// All float32 on the vector ALU; the Linear layers of the temporal stage are 1x1 PP_OP_CONV on the matrix-core kernels.  erf and
// exp are evaluated in double and rounded once (the header's convention).  No atomics: every sum has one fixed order.
#include "pp_internal.h"

#include <algorithm>
#include <climits>

namespace {

__device__ __forceinline__ float pf_gelu(float x) {
    const double d = (double)x;
    return (float)(0.5 * d * (1.0 + erf(d * 0.70710678118654752440)));
}
__device__ __forceinline__ float pf_exp(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---- spatial encoder ---------------------------------------------------------------------------------------------------------
// One wave per frame.  The frame's tokens x [17][32], the LayerNorm / attention output [17][32], qkv [17][96] and the hidden layer
// [17][64] (in qkv's place) live in LDS with row strides whose float4 count is odd (no bank conflicts between token rows).  A Linear
// layer gives every lane one output channel: its weight row sits in registers and the tokens are read as float4 broadcasts, each
// output one fmaf chain over the input channels in order starting from the bias.  What a frame's wave computes depends on the
// frame's 34 numbers and the weights only: not on n, not on the frame's position.
constexpr int SP_J = 17, SP_D = 32, SP_H = 8, SP_HD = 4, SP_HID = 64, SP_DEPTH = 4, SP_F = SP_J * SP_D;
constexpr int SP_XS = 36, SP_QS = 100, SP_HS = 68;     // row strides (floats)
constexpr int SP_EMBED = SP_D * 2 + SP_D + SP_J * SP_D;                                            // embedding w, b, pos
constexpr int SP_BLOCK = 2 * SP_D + 3 * SP_D * SP_D + 3 * SP_D + SP_D * SP_D + SP_D + 2 * SP_D + SP_HID * SP_D + SP_HID + SP_D * SP_HID + SP_D;
constexpr int SP_PARAMS = SP_EMBED + SP_DEPTH * SP_BLOCK + 2 * SP_D;

// dst[t][o] = (res ? res[t][o] : 0) + act(b[o] + sum_c src[t][c] * w[o][c]) for the tokens t = t0, t0 + tstep, ...; K % 4 == 0
template <int K, bool GELU>
__device__ __forceinline__ void sp_linear(const float* __restrict__ w, const float* __restrict__ b, int o, const float* src, int src_stride,
                                          float* dst, int dst_stride, const float* res, int t0, int tstep) {
    float4 wr[K / 4];
#pragma unroll
    for (int c = 0; c < K / 4; ++c) wr[c] = reinterpret_cast<const float4*>(w + (size_t)o * K)[c];
    const float bias = b[o];
    for (int t = t0; t < SP_J; t += tstep) {
        float acc = bias;
#pragma unroll
        for (int c = 0; c < K / 4; ++c) acc = dot4(reinterpret_cast<const float4*>(src + t * src_stride)[c], wr[c], acc);
        if (GELU) acc = pf_gelu(acc);
        if (res) acc = __fadd_rn(res[t * dst_stride + o], acc);
        dst[t * dst_stride + o] = acc;
    }
}

// lane t < 17: dst[t][:] = LayerNorm(src[t][:]) over 32 channels, biased variance, two passes in channel order
__device__ __forceinline__ void sp_layernorm(const float* src, int src_stride, const float* __restrict__ g, const float* __restrict__ b,
                                             float eps, float* dst, int dst_stride, int lane) {
    if (lane < SP_J) {
        const float* r = src + lane * src_stride;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < SP_D; ++c) s += r[c];
        const float mean = s / (float)SP_D;
        float d2 = 0.f;
#pragma unroll
        for (int c = 0; c < SP_D; ++c) {
            const float d = r[c] - mean;
            d2 = fmaf(d, d, d2);
        }
        const float rstd = 1.f / sqrtf(d2 / (float)SP_D + eps);
#pragma unroll
        for (int c = 0; c < SP_D; ++c) dst[lane * dst_stride + c] = (r[c] - mean) * rstd * g[c] + b[c];
    }
}

__global__ __launch_bounds__(64) void spatial_encoder_kernel(const float* __restrict__ kpts, const float* __restrict__ params,
                                                             float* __restrict__ feat, int n) {
    __shared__ float4 xs4[SP_J * SP_XS / 4], ls4[SP_J * SP_XS / 4], qs4[SP_J * SP_QS / 4];
    float* xs = reinterpret_cast<float*>(xs4);
    float* ls = reinterpret_cast<float*>(ls4);
    float* qs = reinterpret_cast<float*>(qs4);
    const int lane = threadIdx.x;
    const size_t frame = blockIdx.x;
    if (frame >= (size_t)n) return;                       // (the whole workgroup leaves)
    const float* in = kpts + frame * (SP_J * 2);
    const float* ew = params;
    const float* eb = params + 2 * SP_D;
    const float* pos = params + 3 * SP_D;
    // x[j][c] = (b[c] + in[j][0] * w[c][0] + in[j][1] * w[c][1]) + pos[j][c]
    for (int idx = lane; idx < SP_F; idx += 64) {
        const int j = idx / SP_D, c = idx % SP_D;
        float acc = eb[c];
        acc = fmaf(in[2 * j], ew[2 * c], acc);
        acc = fmaf(in[2 * j + 1], ew[2 * c + 1], acc);
        xs[j * SP_XS + c] = __fadd_rn(acc, pos[idx]);
    }
    __syncthreads();
    const float* p = params + SP_EMBED;
    for (int blk = 0; blk < SP_DEPTH; ++blk, p += SP_BLOCK) {
        const float* n1w = p;
        const float* n1b = n1w + SP_D;
        const float* qw = n1b + SP_D;
        const float* qb = qw + 3 * SP_D * SP_D;
        const float* pw = qb + 3 * SP_D;
        const float* pb = pw + SP_D * SP_D;
        const float* n2w = pb + SP_D;
        const float* n2b = n2w + SP_D;
        const float* f1w = n2b + SP_D;
        const float* f1b = f1w + SP_HID * SP_D;
        const float* f2w = f1b + SP_HID;
        const float* f2b = f2w + SP_D * SP_HID;
        sp_layernorm(xs, SP_XS, n1w, n1b, 1e-6f, ls, SP_XS, lane);
        __syncthreads();
        sp_linear<SP_D, false>(qw, qb, lane, ls, SP_XS, qs, SP_QS, nullptr, 0, 1);                       // channels 0 .. 63
        if (lane < 32) sp_linear<SP_D, false>(qw, qb, 64 + lane, ls, SP_XS, qs, SP_QS, nullptr, 0, 1);   // 64 .. 95
        __syncthreads();
        // attention: one (head, query) pair per lane and pass; 17 scores in registers; the result goes to ls[query][head * 4 ..]
        for (int pr = lane; pr < SP_H * SP_J; pr += 64) {
            const int h = pr / SP_J, i = pr % SP_J;
            const float4 q = *reinterpret_cast<const float4*>(qs + i * SP_QS + h * SP_HD);
            float s[SP_J];
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < SP_J; ++j) {
                s[j] = __fmul_rn(dot4(q, *reinterpret_cast<const float4*>(qs + j * SP_QS + SP_D + h * SP_HD), 0.f), 0.5f);
                m = fmaxf(m, s[j]);
            }
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < SP_J; ++j) {
                s[j] = pf_exp(s[j] - m);
                sum += s[j];
            }
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < SP_J; ++j) {
                const float pj = s[j] / sum;
                const float4 v = *reinterpret_cast<const float4*>(qs + j * SP_QS + 2 * SP_D + h * SP_HD);
                o.x = fmaf(pj, v.x, o.x);
                o.y = fmaf(pj, v.y, o.y);
                o.z = fmaf(pj, v.z, o.z);
                o.w = fmaf(pj, v.w, o.w);
            }
            *reinterpret_cast<float4*>(ls + i * SP_XS + h * SP_HD) = o;
        }
        __syncthreads();
        // x += proj(attn): lane = (token parity, channel); every (token, channel) of xs is read and written by one lane only
        sp_linear<SP_D, false>(pw, pb, lane & 31, ls, SP_XS, xs, SP_XS, xs, lane >> 5, 2);
        __syncthreads();
        sp_layernorm(xs, SP_XS, n2w, n2b, 1e-6f, ls, SP_XS, lane);
        __syncthreads();
        sp_linear<SP_D, true>(f1w, f1b, lane, ls, SP_XS, qs, SP_HS, nullptr, 0, 1);                      // hidden [17][64] in qkv's place
        __syncthreads();
        sp_linear<SP_HID, false>(f2w, f2b, lane & 31, qs, SP_HS, xs, SP_XS, xs, lane >> 5, 2);
        __syncthreads();
    }
    sp_layernorm(xs, SP_XS, p, p + SP_D, 1e-6f, ls, SP_XS, lane);
    __syncthreads();
    for (int idx = lane; idx < SP_F; idx += 64) feat[frame * SP_F + idx] = ls[(idx / SP_D) * SP_XS + idx % SP_D];
}

// ---- PP_OP_ATTENTION ---------------------------------------------------------------------------------------------------------
// One workgroup of four waves per (sample, head).  K and V of the head sit in LDS ([tokens][ks], ks = the head dim, + 4 when its
// float4 count is even: conflict-free float4 reads across rows).  A wave takes the queries w, w + 4, ...: the lanes share the keys
// (lane l: keys l and l + 64), each score one fmaf chain over the head dim, scaled afterwards; the row maximum and the sum are
// reduced across the wave in a fixed butterfly; the probabilities go through LDS and the lanes then share the head dim (lane l:
// d = l and l + 64), each output one fmaf chain over the keys in order.
constexpr int AT_MAX_T = 128, AT_MAX_HD = 128, AT_WAVES = 4;
__host__ __device__ inline int at_kstride(int hd) { return ((hd / 4) & 1) ? hd : hd + 4; }
__host__ __device__ inline size_t at_lds_floats(int tokens, int hd) {
    return (size_t)2 * tokens * at_kstride(hd) + (size_t)AT_WAVES * (AT_MAX_HD + AT_MAX_T);
}

__global__ __launch_bounds__(64 * AT_WAVES) void attention_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int tokens,
                                                                       int heads, int hd, int creal, int cbuf, float scale) {
    extern __shared__ float4 at_lds4[];
    float* lds = reinterpret_cast<float*>(at_lds4);
    const int ks = at_kstride(hd), hd4 = hd / 4;
    float* kl = lds;
    float* vl = kl + (size_t)tokens * ks;
    float* ql = vl + (size_t)tokens * ks;                 // [AT_WAVES][AT_MAX_HD]
    float* pl = ql + AT_WAVES * AT_MAX_HD;                // [AT_WAVES][AT_MAX_T]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int head = blockIdx.x % heads;
    const size_t n = blockIdx.x / heads;
    const float* base = qkv + n * tokens * (size_t)(3 * cbuf) + head * hd;
    for (int idx = tid; idx < tokens * hd4; idx += 64 * AT_WAVES) {
        const int t = idx / hd4, d = 4 * (idx - t * hd4);
        const float* px = base + (size_t)t * (3 * cbuf) + d;
        *reinterpret_cast<float4*>(kl + t * ks + d) = *reinterpret_cast<const float4*>(px + cbuf);
        *reinterpret_cast<float4*>(vl + t * ks + d) = *reinterpret_cast<const float4*>(px + 2 * cbuf);
    }
    __syncthreads();
    float* qw = ql + wave * AT_MAX_HD;
    float* pw = pl + wave * AT_MAX_T;
    const int rounds = (tokens + AT_WAVES - 1) / AT_WAVES;          // the same for every wave: the barriers below are uniform
    for (int r = 0; r < rounds; ++r) {
        const int i = r * AT_WAVES + wave;
        const bool live = i < tokens;
        if (live)
            for (int d = lane; d < hd; d += 64) qw[d] = base[(size_t)i * (3 * cbuf) + d];
        __syncthreads();
        float s0 = -INFINITY, s1 = -INFINITY;
        if (live) {
            if (lane < tokens) {
                float acc = 0.f;
                for (int d = 0; d < hd4; ++d)
                    acc = dot4(reinterpret_cast<const float4*>(qw)[d], reinterpret_cast<const float4*>(kl + lane * ks)[d], acc);
                s0 = __fmul_rn(acc, scale);
            }
            if (lane + 64 < tokens) {
                float acc = 0.f;
                for (int d = 0; d < hd4; ++d)
                    acc = dot4(reinterpret_cast<const float4*>(qw)[d], reinterpret_cast<const float4*>(kl + (lane + 64) * ks)[d], acc);
                s1 = __fmul_rn(acc, scale);
            }
        }
        const float m = wave_max_f(fmaxf(s0, s1));
        float e0 = 0.f, e1 = 0.f;
        if (live && lane < tokens) e0 = pf_exp(s0 - m);
        if (live && lane + 64 < tokens) e1 = pf_exp(s1 - m);
        const float sum = wave_sum_f(__fadd_rn(e0, e1));
        if (live) {
            pw[lane] = e0 / sum;
            pw[lane + 64] = e1 / sum;
        }
        __syncthreads();
        if (live) {
            for (int d = lane; d < hd; d += 64) {
                float acc = 0.f;
                for (int j = 0; j < tokens; ++j) acc = fmaf(pw[j], vl[j * ks + d], acc);
                out[(n * tokens + i) * (size_t)cbuf + head * hd + d] = acc;
            }
        }
    }
    if (head == heads - 1 && creal < cbuf) {               // the buffer's padding channels: exact zeros
        const int np = cbuf - creal;
        for (int idx = tid; idx < tokens * np; idx += 64 * AT_WAVES)
            out[(n * tokens + idx / np) * (size_t)cbuf + creal + idx % np] = 0.f;
    }
}

// ---- window gather -----------------------------------------------------------------------------------------------------------
// win[b][f][c] = c < 544 ? feat[i0 + b + f][c] + pos[f][c] : 0, one float4 of channels per thread (c4 = channels / 4 of the program's input)
__global__ __launch_bounds__(256) void window_gather_kernel(const float4* __restrict__ feat, const float4* __restrict__ pos,
                                                            float4* __restrict__ win, size_t total, int frames, int f4, int c4, int i0) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % c4);
    const size_t row = idx / c4;
    const int f = (int)(row % frames);
    const size_t b = row / frames;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < f4) {
        const float4 a = feat[((size_t)i0 + b + f) * f4 + c], p = pos[(size_t)f * f4 + c];
        v = make_float4(__fadd_rn(a.x, p.x), __fadd_rn(a.y, p.y), __fadd_rn(a.z, p.z), __fadd_rn(a.w, p.w));
    }
    win[idx] = v;
}

// ---- weighted mean + head ----------------------------------------------------------------------------------------------------
// One workgroup per window: y[c] = (sum_f w[f] * x[f][c], in frame order) + b; LayerNorm(y) with eps 1e-5; out[o] = hb[o] + hw[o] . ln.
// params: w[84] (81 used), b[4] (1 used), gamma[544], beta[544], hw[51][544], hb[52] (51 used)
constexpr int MH_F = 81, MH_C = SP_F, MH_O = 51;
constexpr int MH_PARAMS = 84 + 4 + 2 * MH_C + MH_O * MH_C + 52;
__device__ __forceinline__ float block_sum_256(float v, float* red) {      // fixed order: butterfly per wave, then the four waves in order
    v = wave_sum_f(v);
    __syncthreads();                                                        // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ __launch_bounds__(256) void mean_head_kernel(const float* __restrict__ x, const float* __restrict__ params, float* __restrict__ out,
                                                        int cbuf) {
    __shared__ float ys[MH_C + 32];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xb = x + (size_t)blockIdx.x * MH_F * cbuf;
    const float* w = params;
    const float wb = params[84];
    const float* g = params + 88;
    const float* beta = g + MH_C;
    const float* hw = beta + MH_C;
    const float* hb = hw + MH_O * MH_C;
    float part = 0.f;
    for (int c = tid; c < MH_C; c += 256) {
        float acc = 0.f;
        for (int f = 0; f < MH_F; ++f) acc = fmaf(w[f], xb[(size_t)f * cbuf + c], acc);
        acc = __fadd_rn(acc, wb);
        ys[c] = acc;
        part += acc;
    }
    const float mean = block_sum_256(part, red) / (float)MH_C;
    float d2 = 0.f;
    for (int c = tid; c < MH_C; c += 256) {
        const float d = ys[c] - mean;
        d2 = fmaf(d, d, d2);
    }
    const float rstd = 1.f / sqrtf(block_sum_256(d2, red) / (float)MH_C + 1e-5f);
    for (int c = tid; c < MH_C; c += 256) ys[c] = (ys[c] - mean) * rstd * g[c] + beta[c];
    __syncthreads();
    for (int o = wave; o < MH_O; o += 4) {
        float acc = 0.f;
        for (int c = lane; c < MH_C; c += 64) acc = fmaf(ys[c], hw[(size_t)o * MH_C + c], acc);
        acc = wave_sum_f(acc);
        if (lane == 0) out[(size_t)blockIdx.x * MH_O + o] = __fadd_rn(acc, hb[o]);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_spatial(const float* kpts_dev, const float* params_dev, float* feat_dev, int n, hipStream_t s) {
    hipLaunchKernelGGL(spatial_encoder_kernel, dim3((unsigned)n), dim3(64), 0, s, kpts_dev, params_dev, feat_dev, n);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

struct StageTimer {          // HIP events around the stages of one call; read after the call's synchronisation
    bool on;
    std::vector<hipEvent_t> ev;
    std::vector<int> stage;  // ev[2k], ev[2k + 1] enclose one piece of stage[k]
    explicit StageTimer(bool enable) : on(enable) {}
    ~StageTimer() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
    int mark(hipStream_t s) {
        hipEvent_t e;
        PP_HIP_CHECK(hipEventCreate(&e));
        ev.push_back(e);
        PP_HIP_CHECK(hipEventRecord(e, s));
        return PP_OK;
    }
    int begin(int st, hipStream_t s) {
        if (!on) return PP_OK;
        stage.push_back(st);
        return mark(s);
    }
    int end(hipStream_t s) { return on ? mark(s) : PP_OK; }
    void collect(float* ms) {
        for (size_t k = 0; k < stage.size() && 2 * k + 1 < ev.size(); ++k) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, ev[2 * k], ev[2 * k + 1]) == hipSuccess) ms[stage[k]] += t;
        }
    }
};

}  // namespace

int pp_attention_f32_max_tokens() { return AT_MAX_T; }
int pp_attention_f32_max_head_dim() { return AT_MAX_HD; }

int pp_launch_attention_f32(const float* qkv, float* out, int batch, int tokens, int heads, int c_real, int c_buf, hipStream_t stream) {
    PP_REQUIRE(batch > 0 && tokens > 0 && tokens <= AT_MAX_T, "attention: %d tokens (1 .. %d)", tokens, AT_MAX_T);
    PP_REQUIRE(heads > 0 && c_real > 0 && c_real % heads == 0 && c_real <= c_buf && (c_buf & 3) == 0,
               "attention: %d channels of %d in %d heads", c_real, c_buf, heads);
    const int hd = c_real / heads;
    PP_REQUIRE(hd <= AT_MAX_HD && (hd & 3) == 0, "attention: head dim %d (a multiple of 4, at most %d)", hd, AT_MAX_HD);
    PP_REQUIRE((size_t)batch * heads < ((size_t)1 << 31), "attention: too many (sample, head) pairs");
    PP_REQUIRE(aligned16(qkv) && aligned16(out), "attention: buffers must be 16-byte aligned");
    const size_t lds = at_lds_floats(tokens, hd) * sizeof(float);     // at most 2 * 128 * 132 * 4 + 4 KiB = 136 KiB of the CU's 160
    static PpPerDeviceOnce configured;
    configured.run([&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(at_lds_floats(AT_MAX_T, AT_MAX_HD) * sizeof(float)));
    });
    const float scale = (float)(1.0 / sqrt((double)hd));
    hipLaunchKernelGGL(attention_f32_kernel, dim3((unsigned)(batch * heads)), dim3(64 * AT_WAVES), lds, stream, qkv, out, tokens, heads, hd,
                       c_real, c_buf, scale);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

extern "C" int pp_attention_f32(pp_ctx* ctx, const float* qkv, int batch, int tokens, int heads, int c_real, int c_buf, float* out) {
    PP_REQUIRE(ctx && qkv && out, "pp_attention_f32: NULL argument");
    return pp_launch_attention_f32(qkv, out, batch, tokens, heads, c_real, c_buf, ctx->stream);
}

extern "C" int pp_poseformer_spatial_param_floats() { return SP_PARAMS; }
extern "C" int pp_poseformer_head_param_floats() { return MH_PARAMS; }

extern "C" int pp_poseformer_spatial(pp_ctx* ctx, const float* params, const float* kpts2d_norm, int n_frames, int kpts_mem, float* features) {
    PP_REQUIRE(ctx && params && kpts2d_norm && features, "pp_poseformer_spatial: NULL argument");
    PP_REQUIRE(n_frames >= 0, "pp_poseformer_spatial: %d frames", n_frames);
    PP_REQUIRE((size_t)n_frames * SP_F <= (size_t)INT_MAX, "pp_poseformer_spatial: %d frames in one call", n_frames);
    PP_REQUIRE(kpts_mem == PP_MEM_HOST || kpts_mem == PP_MEM_DEVICE, "pp_poseformer_spatial: mem %d is neither PP_MEM_HOST nor PP_MEM_DEVICE", kpts_mem);
    PP_REQUIRE(aligned16(params), "pp_poseformer_spatial: the parameter block must be 16-byte aligned");
    if (n_frames == 0) return PP_OK;
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    const float* d_k = kpts2d_norm;
    if (kpts_mem == PP_MEM_HOST) {
        const size_t bytes = (size_t)n_frames * SP_J * 2 * sizeof(float);
        int rc = ctx->ensure_scratch(bytes);
        if (rc != PP_OK) return rc;
        PP_HIP_CHECK(hipMemcpyAsync(ctx->scratch, kpts2d_norm, bytes, hipMemcpyHostToDevice, ctx->stream));
        d_k = static_cast<const float*>(ctx->scratch);
    }
    int rc = launch_spatial(d_k, params, features, n_frames, ctx->stream);
    // the staged copy reads the caller's host array: complete on return
    return kpts_mem == PP_MEM_HOST ? pp_sync_after(ctx->stream, rc) : rc;
}

namespace {
int poseformer_enqueue(pp_net* net, pp_ctx* ctx, int in_buf, int out_buf, const float* w, long long spatial_off, long long pos_off,
                       long long head_off, const float* kpts, int n_frames, int cbuf, float* out, int mem, StageTimer& tm) {
    hipStream_t s = ctx->stream;
    const int max_b = pp_net_max_batch(net), n_win = n_frames - (MH_F - 1);
    const bool host = mem == PP_MEM_HOST;
    const size_t k_e = (size_t)n_frames * SP_J * 2, f_e = (size_t)n_frames * SP_F, o_e = (size_t)n_win * MH_O;
    int rc = ctx->ensure_scratch(ScratchCursor::align(f_e * sizeof(float)) +
                                 (host ? ScratchCursor::align(k_e * sizeof(float)) + ScratchCursor::align(o_e * sizeof(float)) : 0));
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    float* d_feat = cur.take<float>(f_e);
    const float* d_k = kpts;
    float* d_out = out;
    if (host) {
        float* staged = cur.take<float>(k_e);
        d_out = cur.take<float>(o_e);
        PP_HIP_CHECK(hipMemcpyAsync(staged, kpts, k_e * sizeof(float), hipMemcpyHostToDevice, s));
        d_k = staged;
    }
    void *in_ptr = nullptr, *out_ptr = nullptr;
    rc = pp_net_buffer(net, in_buf, &in_ptr, nullptr);
    if (rc == PP_OK) rc = pp_net_buffer(net, out_buf, &out_ptr, nullptr);
    if (rc != PP_OK) return rc;
    if ((rc = tm.begin(0, s)) != PP_OK) return rc;
    if ((rc = launch_spatial(d_k, w + spatial_off, d_feat, n_frames, s)) != PP_OK) return rc;
    if ((rc = tm.end(s)) != PP_OK) return rc;
    for (int i0 = 0; i0 < n_win; i0 += max_b) {
        const int b = std::min(max_b, n_win - i0);
        const size_t total = (size_t)b * MH_F * (cbuf / 4);
        if ((rc = tm.begin(1, s)) != PP_OK) return rc;
        hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(d_feat),
                           reinterpret_cast<const float4*>(w + pos_off), static_cast<float4*>(in_ptr), total, MH_F, SP_F / 4, cbuf / 4, i0);
        PP_HIP_CHECK(hipGetLastError());
        if ((rc = tm.end(s)) != PP_OK) return rc;
        pp_net_void_input_amax(net, in_buf);      // the input was just overwritten here, not by pp_net_forward
        if ((rc = tm.begin(2, s)) != PP_OK) return rc;
        if ((rc = pp_net_run(net, b, 0, -1)) != PP_OK) return rc;
        if ((rc = tm.end(s)) != PP_OK) return rc;
        if ((rc = tm.begin(3, s)) != PP_OK) return rc;
        hipLaunchKernelGGL(mean_head_kernel, dim3((unsigned)b), dim3(256), 0, s, static_cast<const float*>(out_ptr), w + head_off,
                           d_out + (size_t)i0 * MH_O, cbuf);
        PP_HIP_CHECK(hipGetLastError());
        if ((rc = tm.end(s)) != PP_OK) return rc;
    }
    if (host) PP_HIP_CHECK(hipMemcpyAsync(out, d_out, o_e * sizeof(float), hipMemcpyDeviceToHost, s));
    return PP_OK;
}
}  // namespace

extern "C" int pp_poseformer_lift(pp_net* net, int in_buf, int out_buf, long long spatial_off, long long pos_off, long long head_off,
                                  const float* kpts2d_norm, int n_frames, float* out, int mem, float* stage_ms) {
    PP_REQUIRE(net && kpts2d_norm && out, "pp_poseformer_lift: NULL argument");
    PP_REQUIRE(mem == PP_MEM_HOST || mem == PP_MEM_DEVICE, "pp_poseformer_lift: mem %d is neither PP_MEM_HOST nor PP_MEM_DEVICE", mem);
    PP_REQUIRE(n_frames >= MH_F, "pp_poseformer_lift: %d frames, the receptive field is %d", n_frames, MH_F);
    PP_REQUIRE((size_t)n_frames * SP_F <= (size_t)INT_MAX, "pp_poseformer_lift: %d frames in one call", n_frames);
    int ih, iw, ic, oh, ow, oc;
    PP_REQUIRE(pp_net_dims(net, in_buf, &ih, &iw, &ic) == PP_OK && pp_net_dims(net, out_buf, &oh, &ow, &oc) == PP_OK,
               "pp_poseformer_lift: bad buffer id");
    PP_REQUIRE(ih == 1 && oh == 1 && iw == MH_F && ow == MH_F && ic == oc && ic >= SP_F && (ic & 3) == 0,
               "pp_poseformer_lift: program shape (in %dx%dx%d, out %dx%dx%d) is not [1][%d][c >= %d]", ih, iw, ic, oh, ow, oc, MH_F, SP_F);
    size_t n_w = 0;
    const float* w = pp_net_weights(net, &n_w);
    PP_REQUIRE(w != nullptr, "pp_poseformer_lift: the net has no weights");
    PP_REQUIRE(spatial_off >= 0 && (spatial_off & 3) == 0 && (size_t)spatial_off + SP_PARAMS <= n_w && pos_off >= 0 && (pos_off & 3) == 0 &&
                   (size_t)pos_off + (size_t)MH_F * SP_F <= n_w && head_off >= 0 && (head_off & 3) == 0 && (size_t)head_off + MH_PARAMS <= n_w,
               "pp_poseformer_lift: parameter blocks out of blob (offsets must be multiples of 4)");
    pp_ctx* ctx = pp_net_ctx(net);
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    PpRange range("pp_poseformer_lift");
    StageTimer tm(stage_ms != nullptr);
    int rc = poseformer_enqueue(net, ctx, in_buf, out_buf, w, spatial_off, pos_off, head_off, kpts2d_norm, n_frames, ic, out, mem, tm);
    // one synchronisation per call, also after an error: the caller's host arrays are read by queued copies
    rc = pp_sync_after(ctx->stream, rc);
    if (rc != PP_OK) return rc;
    if (stage_ms) {
        for (int k = 0; k < 4; ++k) stage_ms[k] = 0.f;
        tm.collect(stage_ms);
    }
    return PP_OK;
}
