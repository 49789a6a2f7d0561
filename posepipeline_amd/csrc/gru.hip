// nn.GRU forward (unidirectional, zero initial state, gate order r, z, n): the temporal encoder of VIBE (2 layers, 2048 -> 1024).
//
// Per layer: the input projection gi = W_ih x + b_ih of all B * T rows is one matrix product (gru_inproj_kernel), then the recurrence
// runs as ONE LAUNCH PER TIME STEP (gru_step_kernel): stream order is the only synchronisation between steps -- no cooperative
// launch, no grid-wide barrier, no workgroup ever waits on memory another workgroup writes.
//
// Both kernels give one wave one output unit.  A dot product is: every lane adds its own terms in ascending k as one fmaf chain,
// then the 64 lane sums are added by the xor butterfly (offsets 32, 16, ... 1; a + b is commutative, so every lane ends with the
// same bits).  The order depends on nothing but the vector length: results are bit-identical from run to run and a sequence's
// result does not depend on the batch it rides in.  The sigmoid and tanh are evaluated in double and rounded once (the PP_ACT_*
// convention); the products and sums around them are float32, in the order of the formulas in posepipe_hip.h.
//
// Memory-bound by design: a step reads W_hh (3 H x H floats, 12.6 MB at H = 1024; it stays in the 256 MB last-level cache between
// steps) once per 4 sequences; the W registers of a wave are reused for up to GRU_BT sequences.
#include <cmath>

#include "pp_internal.h"

namespace {

constexpr int GRU_WAVES = 4;   // waves (output units) per workgroup
constexpr int GRU_BT = 4;      // sequences (step kernel) / rows (input projection) sharing one pass over a weight row
constexpr int GRU_RT = 8;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out[m][j] = bias[j] + sum_k W[j][k] x[m][k];  x [M][K], W [N][K], out [M][N].  grid (ceil(N / GRU_WAVES), ceil(M / GRU_RT))
__global__ __launch_bounds__(64 * GRU_WAVES) void gru_inproj_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                     const float* __restrict__ bias, float* __restrict__ out, int M,
                                                                     int K, int N) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * GRU_WAVES + (threadIdx.x >> 6);
    if (j >= N) return;                                   // wave-uniform
    const int m0 = blockIdx.y * GRU_RT;
    const float* wr = W + (size_t)j * K;
    float acc[GRU_RT];
#pragma unroll
    for (int r = 0; r < GRU_RT; ++r) acc[r] = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float w = wr[k];
#pragma unroll
        for (int r = 0; r < GRU_RT; ++r)
            if (m0 + r < M) acc[r] = fmaf(w, x[(size_t)(m0 + r) * K + k], acc[r]);
    }
    const float b = bias[j];
#pragma unroll
    for (int r = 0; r < GRU_RT; ++r) {
        const float s = wave_sum(acc[r]);
        if (lane == 0 && m0 + r < M) out[(size_t)(m0 + r) * N + j] = s + b;
    }
}

// one time step of one layer for all B sequences.  gi [B][T][3 H] (the input projection), y [B][T][H]: row t - 1 is the previous
// state (t == 0: zeros, the products are skipped: 0 + b_hh = b_hh exactly), row t is written.  grid ceil(H / GRU_WAVES)
__global__ __launch_bounds__(64 * GRU_WAVES) void gru_step_kernel(const float* __restrict__ gi, const float* __restrict__ Whh,
                                                                   const float* __restrict__ bhh, float* __restrict__ y, int B, int T,
                                                                   int H, int t) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * GRU_WAVES + (threadIdx.x >> 6);
    if (j >= H) return;                                   // wave-uniform
    const float* wr = Whh + (size_t)j * H;
    const float* wz = Whh + (size_t)(H + j) * H;
    const float* wn = Whh + (size_t)(2 * H + j) * H;
    const float br = bhh[j], bz = bhh[H + j], bn = bhh[2 * H + j];
    for (int b0 = 0; b0 < B; b0 += GRU_BT) {
        float ar[GRU_BT], az[GRU_BT], an[GRU_BT];
#pragma unroll
        for (int q = 0; q < GRU_BT; ++q) ar[q] = az[q] = an[q] = 0.f;
        if (t > 0) {
            for (int k = lane * 4; k < H; k += 256) {
                const float4 r4 = *reinterpret_cast<const float4*>(wr + k);
                const float4 z4 = *reinterpret_cast<const float4*>(wz + k);
                const float4 n4 = *reinterpret_cast<const float4*>(wn + k);
#pragma unroll
                for (int q = 0; q < GRU_BT; ++q) {
                    if (b0 + q < B) {
                        const float4 h4 = *reinterpret_cast<const float4*>(y + ((size_t)(b0 + q) * T + (t - 1)) * H + k);
                        ar[q] = fmaf(r4.w, h4.w, fmaf(r4.z, h4.z, fmaf(r4.y, h4.y, fmaf(r4.x, h4.x, ar[q]))));
                        az[q] = fmaf(z4.w, h4.w, fmaf(z4.z, h4.z, fmaf(z4.y, h4.y, fmaf(z4.x, h4.x, az[q]))));
                        an[q] = fmaf(n4.w, h4.w, fmaf(n4.z, h4.z, fmaf(n4.y, h4.y, fmaf(n4.x, h4.x, an[q]))));
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < GRU_BT; ++q) {
            const float sr = wave_sum(ar[q]), sz = wave_sum(az[q]), sn = wave_sum(an[q]);
            if (lane == 0 && b0 + q < B) {
                const size_t row = (size_t)(b0 + q) * T + t;
                const float* g = gi + row * 3 * H;
                const float hp = t > 0 ? y[(row - 1) * H + j] : 0.f;
                const float xr = g[j] + (sr + br);
                const float xz = g[H + j] + (sz + bz);
                const float r = (float)(1.0 / (1.0 + exp(-(double)xr)));
                const float z = (float)(1.0 / (1.0 + exp(-(double)xz)));
                const float xn = g[2 * H + j] + r * (sn + bn);
                const float n = (float)tanh((double)xn);
                y[row * H + j] = (1.f - z) * n + z * hp;
            }
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

size_t layer_floats(int in_l, int H) { return (size_t)3 * H * in_l + (size_t)3 * H * H + (size_t)6 * H; }

}  // namespace

extern "C" long long pp_gru_param_floats(int in, int hidden, int layers) {
    if (in < 1 || hidden < 1 || layers < 1) return 0;
    return (long long)(layer_floats(in, hidden) + (size_t)(layers - 1) * layer_floats(hidden, hidden));
}

extern "C" int pp_gru_forward(pp_ctx* ctx, const float* x, int B, int T, int in, int hidden, int layers, const float* params, float* y,
                              int mem) {
    PP_REQUIRE(ctx && x && params && y, "pp_gru_forward: NULL argument");
    PP_REQUIRE(mem == PP_MEM_HOST || mem == PP_MEM_DEVICE, "pp_gru_forward: mem %d is neither PP_MEM_HOST nor PP_MEM_DEVICE", mem);
    PP_REQUIRE(B >= 1 && T >= 1 && in >= 1, "pp_gru_forward: B = %d, T = %d, in = %d (each at least 1)", B, T, in);
    PP_REQUIRE(layers >= 1, "pp_gru_forward: %d layers", layers);
    PP_REQUIRE(hidden >= 4 && (hidden & 3) == 0, "pp_gru_forward: hidden size %d is not a positive multiple of 4", hidden);
    PP_REQUIRE(aligned16(params), "pp_gru_forward: the parameter blob must be 16-byte aligned");
    const size_t H = (size_t)hidden, rows = (size_t)B * T;
    PP_REQUIRE(rows * 3 * H < ((size_t)1 << 31) && rows * in < ((size_t)1 << 31), "pp_gru_forward: %d x %d rows in one call", B, T);
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    const bool host = mem == PP_MEM_HOST;
    const size_t x_e = rows * in, y_e = rows * H, gi_e = rows * 3 * H;
    // gi, the layers' outputs ping-pong (the last layer writes y itself), and the staged x / y of a host call
    size_t need = ScratchCursor::align(gi_e * 4) + 2 * ScratchCursor::align(y_e * 4);
    if (host) need += ScratchCursor::align(x_e * 4) + ScratchCursor::align(y_e * 4);
    int rc = ctx->ensure_scratch(need);
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    hipStream_t s = ctx->stream;
    float* gi = cur.take<float>(gi_e);
    float* mid[2] = {cur.take<float>(y_e), cur.take<float>(y_e)};
    const float* d_x = x;
    float* d_y = y;
    if (host) {
        float* sx = cur.take<float>(x_e);
        d_y = cur.take<float>(y_e);
        PP_HIP_CHECK(hipMemcpyAsync(sx, x, x_e * 4, hipMemcpyHostToDevice, s));
        d_x = sx;
    }
    PP_REQUIRE(aligned16(d_y), "pp_gru_forward: y must be 16-byte aligned");
    const float* p = params;
    const float* lin = d_x;
    int in_l = in;
    rc = PP_OK;
    for (int l = 0; l < layers && rc == PP_OK; ++l) {
        const float* Wih = p;
        const float* Whh = Wih + (size_t)3 * H * in_l;
        const float* bih = Whh + (size_t)3 * H * H;
        const float* bhh = bih + 3 * H;
        float* lout = l == layers - 1 ? d_y : mid[l & 1];
        dim3 g1((unsigned)((3 * H + GRU_WAVES - 1) / GRU_WAVES), (unsigned)((rows + GRU_RT - 1) / GRU_RT));
        hipLaunchKernelGGL(gru_inproj_kernel, g1, dim3(64 * GRU_WAVES), 0, s, lin, Wih, bih, gi, (int)rows, in_l, (int)(3 * H));
        for (int t = 0; t < T; ++t)
            hipLaunchKernelGGL(gru_step_kernel, dim3((unsigned)((H + GRU_WAVES - 1) / GRU_WAVES)), dim3(64 * GRU_WAVES), 0, s, gi, Whh, bhh,
                               lout, B, T, hidden, t);
        if (hipGetLastError() != hipSuccess) {
            pp_set_error("pp_gru_forward: kernel launch failed (layer %d)", l);
            rc = PP_ERR_HIP;
        }
        p = bhh + 3 * H;
        lin = lout;
        in_l = hidden;
    }
    if (host) {
        // the staged copies read / write the caller's arrays: complete on return, also after an error
        hipError_t e = rc == PP_OK ? hipMemcpyAsync(y, d_y, y_e * 4, hipMemcpyDeviceToHost, s) : hipSuccess;
        hipError_t e2 = hipStreamSynchronize(s);
        if (rc != PP_OK) return rc;
        PP_HIP_CHECK(e);
        PP_HIP_CHECK(e2);
    }
    return rc;
}
