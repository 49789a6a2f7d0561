// GAST-Net (Liu et al., "A Graph Attention Spatio-temporal Convolutional Network for 3D Human Pose Estimation in Video") as the lifter
// behind pose_pipeline/wrappers/gastnet_lifting.py (models/gastnet.py): the two ops of its graph-attention blocks that the library
// lacked.  Activations are [n][17 joints][w time steps][channels]; both ops mix over the 17-long joint axis of one time step.
//   PP_OP_GRAPH_MIX    channel-wise graph convolution (SemCHGraphConv with the softmaxed adjacency, and the BatchNorm behind it, folded
//                      into a per-channel 17 x 17 matrix on the host), g graphs in one pass
//   PP_OP_JOINT_ATTN   per time step and head, softmax(q k^T) v over the 17 joints (MultiGlobalGraph), no scale
// and pp_gastnet_lift_many (at the end of the file): the lifter's chunk loop for every track of a call, windows, mirror images, flip
// merge and camera rotation as two kernels around the program.
// Both ops are float32 on the vector ALU and memory bound: every input element is read from global memory once, every output written
// once.  exp is evaluated in double and rounded once (the header's convention).  No atomics: every sum has one fixed order.
#include "chunked_lift.h"

#include <algorithm>
#include <climits>
#include <vector>

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

// ---- pp_gastnet_lift_many ----------------------------------------------------------------------------------------------------------
// The chunk loop of wrappers/gastnet.lift_chunks for every track of a call, on the device, through the driver VideoPose3D uses
// (chunked_lift.h: work table, staging, the loop over the batch groups, download, one synchronisation per call): a work item is one
// (segment, chunk of T output frames) pair; with flip it takes two batch samples, the window and its mirror image, next to each
// other.  Here are the two kernels around the program and the entry's argument checks: gast_pack_kernel writes the samples of one
// batch group from the packed tracks, gast_merge_kernel averages each pair, rotates into world space and scatters the item's frames
// into the packed result.  Every float32 operation of the merge is one rounded product, sum or difference in the order of the host
// formula (wrappers/gastnet.lift_chunks, camera_to_world): the result is the host's, bit for bit.
namespace {

struct GastQuat {
    float w, x, y, z;
};

// wrappers/gastnet._MIRROR: the left and right joints of the H36M skeleton swapped (its own inverse)
__device__ __forceinline__ int gast_mirror(int j) {
    constexpr int m[GJ] = {0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13};
    return m[j];
}

// in[item * S + s][j][w][0 .. 3] = (x, y, 0, 0) of frame clamp(t0 - pad + w, 0, len - 1) of the item's segment (np.pad 'edge', and the
// last chunk filled up with its last frame); sample s = 1: joint mirror(j) with x negated.  One thread per float4.
__global__ __launch_bounds__(256) void gast_pack_kernel(const float2* __restrict__ src, const LiftItem* __restrict__ items, int total,
                                                         int iw, int pad, int S, float4* __restrict__ in) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int w = idx % iw;
    const int j = (idx / iw) % GJ;
    const int smp = idx / (iw * GJ);
    const LiftItem it = items[smp / S];
    const bool mir = (smp % S) != 0;
    int row = it.t0 - pad + w;
    row = row < 0 ? 0 : (row >= it.len ? it.len - 1 : row);
    const float2 v = src[((size_t)it.base + row) * GJ + (mir ? gast_mirror(j) : j)];
    in[idx] = make_float4(mir ? -v.x : v.x, v.y, 0.f, 0.f);
}

// np.cross(q, v) in float32: per component two rounded products and one rounded difference
__device__ __forceinline__ void gast_cross(float qx, float qy, float qz, const float* v, float* c) {
    c[0] = __fsub_rn(__fmul_rn(qy, v[2]), __fmul_rn(qz, v[1]));
    c[1] = __fsub_rn(__fmul_rn(qz, v[0]), __fmul_rn(qx, v[2]));
    c[2] = __fsub_rn(__fmul_rn(qx, v[1]), __fmul_rn(qy, v[0]));
}

// dst[base + t0 + r][j] = rotate((y0[j][r] + mirror(y1)[j][r]) / 2) for r < min(T, len - t0).  One thread per (item, joint, frame).
__global__ __launch_bounds__(256) void gast_merge_kernel(const float* __restrict__ out, const LiftItem* __restrict__ items, int total,
                                                          int T, int S, int rotate, GastQuat q, float* __restrict__ dst) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int r = idx % T;
    const int j = (idx / T) % GJ;
    const int ci = idx / (T * GJ);
    const LiftItem it = items[ci];
    if (r >= it.len - it.t0) return;
    const float* y0 = out + (((size_t)ci * S * GJ + j) * T + r) * 3;
    float v[3] = {y0[0], y0[1], y0[2]};
    if (S == 2) {
        const float* y1 = out + ((((size_t)ci * S + 1) * GJ + gast_mirror(j)) * T + r) * 3;
        v[0] = __fmul_rn(__fadd_rn(v[0], -y1[0]), 0.5f);
        v[1] = __fmul_rn(__fadd_rn(v[1], y1[1]), 0.5f);
        v[2] = __fmul_rn(__fadd_rn(v[2], y1[2]), 0.5f);
    }
    if (rotate) {
        float uv[3], uuv[3];
        gast_cross(q.x, q.y, q.z, v, uv);
        gast_cross(q.x, q.y, q.z, uv, uuv);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = __fadd_rn(v[k], __fmul_rn(2.f, __fadd_rn(__fmul_rn(q.w, uv[k]), uuv[k])));
    }
    float* d = dst + (((size_t)it.base + it.t0 + r) * GJ + j) * 3;
    d[0] = v[0];
    d[1] = v[1];
    d[2] = v[2];
}

}  // namespace

extern "C" int pp_gastnet_lift_many(pp_net* net, int in_buf, int out_buf, const float* kpts_norm, const int32_t* seg_len, int n_seg,
                                    int pad, int flip, const float* cam_quat, float* out, int mem) {
    PP_REQUIRE(net, "pp_gastnet_lift_many: NULL net");
    PP_REQUIRE(n_seg >= 0 && pad >= 0, "pp_gastnet_lift_many: bad dims (n_seg %d, pad %d)", n_seg, pad);
    PP_REQUIRE(mem == PP_MEM_HOST || mem == PP_MEM_DEVICE, "pp_gastnet_lift_many: mem %d is neither PP_MEM_HOST nor PP_MEM_DEVICE", mem);
    if (n_seg == 0) return PP_OK;
    PP_REQUIRE(kpts_norm && seg_len && out, "pp_gastnet_lift_many: NULL argument");
    size_t rows = 0;
    for (int i = 0; i < n_seg; ++i) {
        PP_REQUIRE(seg_len[i] > 0, "pp_gastnet_lift_many: segment %d has %d frames (every segment needs at least one)", i, seg_len[i]);
        rows += (size_t)seg_len[i];
    }
    PP_REQUIRE(rows <= (size_t)INT_MAX / (GJ * 3), "pp_gastnet_lift_many: %zu frames in one call (the work table holds int32 rows)", rows);
    const int S = flip ? 2 : 1, max_b = pp_net_max_batch(net);
    PP_REQUIRE(max_b >= S, "pp_gastnet_lift_many: flip needs two samples per work item, the net has max_batch %d", max_b);
    int ih, iw, ic, oh, ow, oc;
    PP_REQUIRE(pp_net_dims(net, in_buf, &ih, &iw, &ic) == PP_OK && pp_net_dims(net, out_buf, &oh, &ow, &oc) == PP_OK,
               "pp_gastnet_lift_many: bad buffer id");
    PP_REQUIRE(ih == GJ && ic == 4 && oh == GJ && oc == 3 && ow > 0 && iw == ow + 2 * pad,
               "pp_gastnet_lift_many: program shape (in %dx%dx%d, out %dx%dx%d) is not [17][T + 2 pad][4] -> [17][T][3] at pad=%d",
               ih, iw, ic, oh, ow, oc, pad);
    const int T = ow;
    PP_REQUIRE((size_t)max_b * GJ * iw <= (size_t)INT_MAX, "pp_gastnet_lift_many: batch of %d samples of %d time steps is too large", max_b, iw);
    GastQuat q{1.f, 0.f, 0.f, 0.f};
    if (cam_quat) q = GastQuat{cam_quat[0], cam_quat[1], cam_quat[2], cam_quat[3]};
    const int rotate = cam_quat ? 1 : 0;
    // src: the packed tracks where the kernel reads them (a host array's staged copy).  Both refusals are the same for every group of
    // a call, so a refused call has launched nothing.
    auto pack = [=](hipStream_t s, const float* src, const LiftItem* items, int b, void* in) -> int {
        PP_REQUIRE((reinterpret_cast<uintptr_t>(src) & 7) == 0, "pp_gastnet_lift_many: kpts_norm must be 8-byte aligned");
        PP_REQUIRE(aligned16(in), "pp_gastnet_lift_many: the program's input buffer must be 16-byte aligned");
        const int total = b * S * GJ * iw;
        hipLaunchKernelGGL(gast_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float2*>(src), items, total,
                           iw, pad, S, static_cast<float4*>(in));
        return PP_OK;
    };
    auto merge = [=](hipStream_t s, const float* net_out, const LiftItem* items, int b, float* dst) -> int {
        const int total = b * GJ * T;
        hipLaunchKernelGGL(gast_merge_kernel, dim3((total + 255) / 256), dim3(256), 0, s, net_out, items, total, T, S, rotate, q, dst);
        return PP_OK;
    };
    PpRange range("pp_gastnet_lift_many");
    return chunked_lift(net, in_buf, out_buf, kpts_norm, seg_len, n_seg, rows, T, S, GJ * 2, GJ * 3, out, mem, pack, merge);
}
