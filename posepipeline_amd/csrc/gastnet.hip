// GAST-Net (Liu et al., "A Graph Attention Spatio-temporal Convolutional Network for 3D Human Pose Estimation in Video") as the lifter
// behind pose_pipeline/wrappers/gastnet_lifting.py (models/gastnet.py): the two ops of its graph-attention blocks that the library
// lacked.  Activations are [n][17 joints][w time steps][channels]; both ops mix over the 17-long joint axis of one time step.
//   PP_OP_GRAPH_MIX    channel-wise graph convolution (SemCHGraphConv with the softmaxed adjacency, and the BatchNorm behind it, folded
//                      into a per-channel 17 x 17 matrix on the host), g graphs in one pass
//   PP_OP_JOINT_ATTN   per time step and head, softmax(q k^T) v over the 17 joints (MultiGlobalGraph), no scale
// Both are float32 on the vector ALU and memory bound: every input element is read from global memory once, every output written
// once.  exp is evaluated in double and rounded once (the header's convention).  No atomics: every sum has one fixed order.
#include "pp_internal.h"

namespace {

constexpr int GJ = 17;                  // joints of the H36M skeleton: the H axis of every buffer

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 acc) {
    acc.x = fmaf(a.x, b.x, acc.x);
    acc.y = fmaf(a.y, b.y, acc.y);
    acc.z = fmaf(a.z, b.z, acc.z);
    acc.w = fmaf(a.w, b.w, acc.w);
    return acc;
}

// ---- PP_OP_GRAPH_MIX ---------------------------------------------------------------------------------------------------------------
// One thread per (graph, time step, float4 of channels); a workgroup of 256 threads is a tile of 256 / (c / 4) time steps of one graph
// for all 17 joints.  The thread first reads its 34 input float4 (h0 and h1 of every joint: the only global reads of the activations,
// all in flight together, coalesced over the channels), then walks the 17 output joints: per joint one fmaf chain over the source
// joints of the neighbour mask in ascending order (h0 on the diagonal, h1 off it), the matrix entries read as float4 over the channels
// (1156 c floats per graph: they stay in L2 and are shared by every time step).  The mask of (graph, joint) is the same for all lanes
// of a wave whenever a wave does not straddle two graphs, so the skipped terms cost a scalar branch.  Nothing is staged in LDS: a
// time step's 17 x 2 g c inputs are 139 KiB at c = 512, and no element is needed by a second thread.
__global__ __launch_bounds__(256) void graph_mix_kernel(const float* __restrict__ x, const float* __restrict__ amat,
                                                         const float* __restrict__ bias_nb, float* __restrict__ y, int w, int g, int c,
                                                         int y_stride, int y_coff, int relu) {
    const int c4 = c >> 2;
    const size_t per_sample = (size_t)g * w * c4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= per_sample) return;
    const int ch = 4 * (int)(idx % c4);
    const int t = (int)((idx / c4) % w);
    const int gr = (int)(idx / ((size_t)c4 * w));
    const size_t n = blockIdx.y;
    const int cin = 2 * g * c;
    const float* xb = x + ((n * GJ) * w + t) * (size_t)cin + (size_t)gr * 2 * c + ch;
    const size_t xj = (size_t)w * cin;                                   // one joint further
    float4 h0[GJ], h1[GJ];
#pragma unroll
    for (int j = 0; j < GJ; ++j) {
        h0[j] = *reinterpret_cast<const float4*>(xb + j * xj);
        h1[j] = *reinterpret_cast<const float4*>(xb + j * xj + c);
    }
    const float* ag = amat + (size_t)gr * GJ * GJ * c + ch;              // A[j][i][c]
    const float4 b = *reinterpret_cast<const float4*>(bias_nb + (size_t)gr * c + ch);
    const float* nb = bias_nb + (size_t)g * c + gr * GJ;                 // per (graph, joint): the 17 mask bits as an exact float
    float* yb = y + ((n * GJ) * w + t) * (size_t)y_stride + y_coff + (size_t)gr * c + ch;
    const size_t yj = (size_t)w * y_stride;
#pragma unroll
    for (int j = 0; j < GJ; ++j) {
        const unsigned mask = (unsigned)nb[j];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < GJ; ++i)
            if ((mask >> i) & 1u)
                acc = fma4(*reinterpret_cast<const float4*>(ag + (size_t)(j * GJ + i) * c), i == j ? h0[i] : h1[i], acc);
        acc = make_float4(__fadd_rn(acc.x, b.x), __fadd_rn(acc.y, b.y), __fadd_rn(acc.z, b.z), __fadd_rn(acc.w, b.w));
        if (relu) acc = make_float4(fmaxf(acc.x, 0.f), fmaxf(acc.y, 0.f), fmaxf(acc.z, 0.f), fmaxf(acc.w, 0.f));
        *reinterpret_cast<float4*>(yb + j * yj) = acc;
    }
}

// ---- PP_OP_JOINT_ATTN --------------------------------------------------------------------------------------------------------------
// One wave per (sample, time step, head); a workgroup is a tile of `waves` consecutive time steps of one head.  The wave stages the q,
// k and v rows of its 17 joints in its own part of LDS ([17][ks] each, ks = the head dim, + 4 when its float4 count is even: float4
// reads of consecutive rows hit distinct banks), once.  Then, with barriers between the phases (every wave of the workgroup takes
// every barrier; a wave beyond the last time step only skips the work):
//   scores   lane p, p + 64, ... : pair (i, j) = (p / 17, p % 17), s[i][j] = q_i . k_j, one fmaf chain over d from 0
//   softmax  lane i < 17: m = max_j s[i][j]; e_j = exp(s[i][j] - m) (the difference rounded to float32, exp in double, rounded once);
//            sum = ((e_0 + e_1) + ...) in joint order; p[i][j] = e_j / sum
//   output   lane over (i, float4 of d): out_i = one fmaf chain over j = 0 .. 16 of p[i][j] * v_j from 0, stored as float4
constexpr int JA_MAX_HD = 128, JA_SS = 20;            // score rows of 20 floats
__host__ __device__ inline int ja_kstride(int hd) { return ((hd / 4) & 1) ? hd : hd + 4; }
__host__ __device__ inline int ja_wave_floats(int hd) { return 3 * GJ * ja_kstride(hd) + GJ * JA_SS; }
inline int ja_waves(int hd) { return hd > 64 ? 2 : 4; }     // 2 x 27.6 KiB at hd = 128, 4 x 15.2 KiB at hd = 64: under 64 KiB

__global__ __launch_bounds__(256) void joint_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int w, int heads, int hd,
                                                          int creal, int cbuf, int y_stride, int y_coff) {
    extern __shared__ float4 ja_lds4[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int ks = ja_kstride(hd), hd4 = hd >> 2;
    float* ql = reinterpret_cast<float*>(ja_lds4) + (size_t)wave * ja_wave_floats(hd);
    float* kl = ql + GJ * ks;
    float* vl = kl + GJ * ks;
    float* sl = vl + GJ * ks;
    const int head = blockIdx.x % heads;
    const int t = (blockIdx.x / heads) * waves + wave;
    const size_t n = blockIdx.y;
    const bool live = t < w;
    const size_t jstride = (size_t)w * (3 * cbuf);
    const float* base = qkv + ((n * GJ) * w + (live ? t : 0)) * (size_t)(3 * cbuf) + head * hd;
    if (live)
        for (int idx = lane; idx < GJ * hd4; idx += 64) {
            const int j = idx / hd4, d = 4 * (idx - j * hd4);
            const float* px = base + j * jstride + d;
            *reinterpret_cast<float4*>(ql + j * ks + d) = *reinterpret_cast<const float4*>(px);
            *reinterpret_cast<float4*>(kl + j * ks + d) = *reinterpret_cast<const float4*>(px + cbuf);
            *reinterpret_cast<float4*>(vl + j * ks + d) = *reinterpret_cast<const float4*>(px + 2 * cbuf);
        }
    __syncthreads();
    if (live)
        for (int p = lane; p < GJ * GJ; p += 64) {
            const int i = p / GJ, j = p - i * GJ;
            const float4* q4 = reinterpret_cast<const float4*>(ql + i * ks);
            const float4* k4 = reinterpret_cast<const float4*>(kl + j * ks);
            float acc = 0.f;
            for (int d = 0; d < hd4; ++d) {
                const float4 a = q4[d], b = k4[d];
                acc = fmaf(a.x, b.x, acc);
                acc = fmaf(a.y, b.y, acc);
                acc = fmaf(a.z, b.z, acc);
                acc = fmaf(a.w, b.w, acc);
            }
            sl[i * JA_SS + j] = acc;
        }
    __syncthreads();
    if (live && lane < GJ) {
        float* s = sl + lane * JA_SS;
        float m = s[0];
#pragma unroll
        for (int j = 1; j < GJ; ++j) m = fmaxf(m, s[j]);
        float e[GJ];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < GJ; ++j) {
            e[j] = (float)exp((double)__fsub_rn(s[j], m));
            sum = __fadd_rn(sum, e[j]);
        }
#pragma unroll
        for (int j = 0; j < GJ; ++j) s[j] = __fdiv_rn(e[j], sum);
    }
    __syncthreads();
    if (live) {
        float* ob = out + ((n * GJ) * w + t) * (size_t)y_stride + y_coff + head * hd;
        const size_t oj = (size_t)w * y_stride;
        for (int idx = lane; idx < GJ * hd4; idx += 64) {
            const int i = idx / hd4, d = 4 * (idx - i * hd4);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < GJ; ++j) {
                const float pj = sl[i * JA_SS + j];
                acc = fma4(make_float4(pj, pj, pj, pj), *reinterpret_cast<const float4*>(vl + j * ks + d), acc);
            }
            *reinterpret_cast<float4*>(ob + i * oj + d) = acc;
        }
        if (head == heads - 1 && creal < cbuf) {          // the padding channels [cin, cout): exact zeros
            const int np4 = (cbuf - creal) >> 2;
            float* zb = out + ((n * GJ) * w + t) * (size_t)y_stride + y_coff + creal;
            for (int idx = lane; idx < GJ * np4; idx += 64)
                *reinterpret_cast<float4*>(zb + (idx / np4) * oj + 4 * (idx % np4)) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

}  // namespace

int pp_launch_graph_mix(const float* x, const float* amat, const float* bias_nb, float* y, int n, int h, int w, int g, int c,
                        int y_stride, int y_coff, int relu, hipStream_t stream) {
    PP_REQUIRE(n > 0 && h == GJ && w > 0, "graph_mix: maps of %d joints (expected %d), %d time steps", h, GJ, w);
    PP_REQUIRE(g > 0 && g <= 4 && c > 0 && (c & 3) == 0, "graph_mix: %d graphs (1 .. 4) of %d channels (a multiple of 4)", g, c);
    PP_REQUIRE(y_coff >= 0 && (y_coff & 3) == 0 && (y_stride & 3) == 0 && y_coff + g * c <= y_stride,
               "graph_mix: channels [%d, %d) do not fit the out buffer (%d channels)", y_coff, y_coff + g * c, y_stride);
    PP_REQUIRE(n <= 65535, "graph_mix: %d samples in one launch (at most 65535)", n);
    PP_REQUIRE(aligned16(x) && aligned16(amat) && aligned16(bias_nb) && aligned16(y), "graph_mix: buffers must be 16-byte aligned");
    const size_t per_sample = (size_t)g * w * (c >> 2);
    PP_REQUIRE((per_sample + 255) / 256 < ((size_t)1 << 31), "graph_mix: map too large");
    hipLaunchKernelGGL(graph_mix_kernel, dim3((unsigned)((per_sample + 255) / 256), (unsigned)n), dim3(256), 0, stream, x, amat, bias_nb, y,
                       w, g, c, y_stride, y_coff, relu);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_joint_attn_max_head_dim() { return JA_MAX_HD; }

int pp_launch_joint_attn(const float* qkv, float* out, int n, int h, int w, int heads, int c_real, int c_buf, int y_stride, int y_coff,
                         hipStream_t stream) {
    PP_REQUIRE(n > 0 && h == GJ && w > 0, "joint_attn: maps of %d joints (expected %d), %d time steps", h, GJ, w);
    PP_REQUIRE(heads > 0 && c_real > 0 && c_real % heads == 0 && c_real <= c_buf && (c_buf & 3) == 0,
               "joint_attn: %d channels of %d in %d heads", c_real, c_buf, heads);
    const int hd = c_real / heads;
    PP_REQUIRE(hd <= JA_MAX_HD && (hd & 3) == 0, "joint_attn: head dim %d (a multiple of 4, at most %d)", hd, JA_MAX_HD);
    PP_REQUIRE(y_coff >= 0 && (y_coff & 3) == 0 && (y_stride & 3) == 0 && y_coff + c_buf <= y_stride,
               "joint_attn: channels [%d, %d) do not fit the out buffer (%d channels)", y_coff, y_coff + c_buf, y_stride);
    PP_REQUIRE(n <= 65535, "joint_attn: %d samples in one launch (at most 65535)", n);
    PP_REQUIRE(aligned16(qkv) && aligned16(out), "joint_attn: buffers must be 16-byte aligned");
    const int waves = ja_waves(hd);
    const size_t blocks = (size_t)((w + waves - 1) / waves) * heads;
    PP_REQUIRE(blocks < ((size_t)1 << 31), "joint_attn: map too large");
    const size_t lds = (size_t)waves * ja_wave_floats(hd) * sizeof(float);            // at most 56.6 KiB (hd = 128, two waves)
    hipLaunchKernelGGL(joint_attn_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(64 * waves), lds, stream, qkv, out, w, heads, hd,
                       c_real, c_buf, y_stride, y_coff);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
