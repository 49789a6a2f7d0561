// TraDeS (DLA-34 + cost volume association, TrackingBboxMethodLookup row 4) on the device: what the method needs besides the layers
// of models/dla.py.
//
//   pp_trades_cva            cost-volume association of two embedding maps, ONE fused kernel: the P x P volume c[q][i][j] =
//                            <cur[q], prev[i][j]> is formed on the matrix cores (v_mfma_f32_32x32x2_f32, exact float32) tile by tile
//                            and reduced at once to its row maxima ch[q][i] and column maxima cw[q][j], which live in LDS; then the
//                            two softmaxes and the two expected offsets.  Upstream materialises the volume (168 MB at 60 x 108).
//   pp_trades_render_prehm   the tracker's boxes rendered as Gaussians (draw_umich_gaussian, elementwise max), written after
//                            AvgPool2d(4, 4): the input-resolution map is never stored
//   PP_OP_SUB_CAT / PP_OP_BCAST_MUL / PP_OP_BLEND2   the elementwise steps of program B (difference + concatenation, the pre_hm gate,
//                            the two-way attention blend)
// (pp_trades_decode lives next to pp_fairmot_decode in fairmot.hip and shares its peak and key kernels.)
// TraDeS and CenterTrack are not vendored: UNPINNED restatements, rules in include/posepipe_hip.h, numpy twins in tests/trades_ref.py.
#include "pp_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- pp_trades_cva ---------------------------------------------------------------------------------------------------------------
// A workgroup (4 waves) owns CVA_TQ = 32 queries of one frame pair and walks the previous frame's P keys in tiles of 4 x 32: wave v
// stages keys [tile + 32 v, + 32) x 128 channels in its own LDS rows and multiplies them with the 32 queries, whose 128 channels stay
// in registers for the whole kernel (the B operand: lane = query, 64 registers).  A tile is staged in two halves of 64 channels, so
// that the keys take 34 KB of LDS and two workgroups fit a CU; an LDS row holds the half's even channels, then its odd channels (row
// stride 68 floats): MFMA step t takes channel 2 t + (lane >> 5), so a lane's A operands of four steps are ONE 16-byte LDS read, and a
// staged float4 of four channels is two 8-byte stores.  The MFMA leaves lane (query = lane & 31) with 16 keys
// (rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), ascending: the lane folds runs of keys of one map row into one value and commits it
// to ch[query][i]; every value goes to cw[query][j].  Both by an LDS integer atomic max on an order-preserving image of the float
// (exact: a maximum is a selection), so that waves and half waves need no ordering: the workgroup meets at two barriers only, after
// the maxima are initialised and before the finish.  Keys >= P are skipped, queries >= P not stored.
constexpr int CVA_TQ = 32;
constexpr int CVA_TK = 128;        // keys per tile: 32 per wave
constexpr int CVA_DIM = 128;
constexpr int CVA_KH = CVA_DIM / 2;        // channels per staging phase: a tile is staged in two halves, which halves the LDS
constexpr int CVA_KS = CVA_KH + 4;
constexpr int CVA_THREADS = 256;

__device__ __forceinline__ int f2ord(float f) {
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float ord2f(int o) { return __int_as_float(o >= 0 ? o : o ^ 0x7fffffff); }

__device__ __forceinline__ float wave_max(float v) {
    for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int s = 32; s > 0; s >>= 1) v = v + __shfl_xor(v, s, 64);
    return v;
}

// orders this wave's LDS accesses across its lanes (a wave's LDS instructions are executed in order; the fences keep the compiler
// from moving them)
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct CvaArgs {
    const float* cur;    // [n][P][128]
    const float* prev;   // [n][P][128]
    float* offset;       // [n][2 hc][2 wc][2]
    float* soft_h;       // [n][P][hc] or null
    float* soft_w;       // [n][P][wc] or null
    int hc, wc, P, sh, sw;   // sh, sw: LDS row strides of ch / cw (odd)
};

// softmax over `len` maxima of one query (one wave), temperature 5, max-subtracted; returns sum_k p_k 2 (k - k_q)
__device__ __forceinline__ float cva_expect(const int* row, int len, int kq, float* soft, int lane) {
    float m = -INFINITY;
    for (int k = lane; k < len; k += 64) m = fmaxf(m, 5.f * ord2f(row[k]));
    m = wave_max(m);
    float s = 0.f;
    for (int k = lane; k < len; k += 64) s = s + (float)exp((double)(5.f * ord2f(row[k]) - m));
    s = wave_sum(s);
    float e = 0.f;
    for (int k = lane; k < len; k += 64) {
        const float p = (float)exp((double)(5.f * ord2f(row[k]) - m)) / s;
        if (soft) soft[k] = p;
        e = e + p * (float)(2 * (k - kq));
    }
    return wave_sum(e);
}

__global__ __launch_bounds__(CVA_THREADS) void cva_kernel(CvaArgs a) {
    __shared__ __attribute__((aligned(16))) float keys[4][32][CVA_KS];
    extern __shared__ int maxima[];                  // ch [32][sh], then cw [32][sw]
    int* ch = maxima;
    int* cw = maxima + CVA_TQ * a.sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const size_t pair = blockIdx.y;
    const float* cur = a.cur + pair * (size_t)a.P * CVA_DIM;
    const float* prev = a.prev + pair * (size_t)a.P * CVA_DIM;
    const int q0 = blockIdx.x * CVA_TQ;

    for (int e = tid; e < CVA_TQ * (a.sh + a.sw); e += CVA_THREADS) maxima[e] = INT_MIN;

    // B operand: query l31, channels 2 t + half
    float qv[CVA_DIM / 2];
    {
        const int q = q0 + l31;
        const float* qp = cur + (size_t)(q < a.P ? q : 0) * CVA_DIM + half;
#pragma unroll
        for (int t = 0; t < CVA_DIM / 2; ++t) qv[t] = q < a.P ? qp[2 * t] : 0.f;
    }

    // staging items of this lane: key (lane >> 5) + 2 u, channels 4 l31 .. + 3, u = 0 .. 15
    float4 pre[16];
    auto prefetch = [&](int tile) {
        const int kbase = tile * CVA_TK + wave * 32;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int key = kbase + half + 2 * u;
            pre[u] = key < a.P ? *reinterpret_cast<const float4*>(prev + (size_t)key * CVA_DIM + 4 * l31) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // phase p stages channels [64 p, 64 p + 64) of the wave's 32 keys: the lanes whose float4 lies in that half store it
    auto deposit = [&](int p) {
        if ((l31 >> 4) == p) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                float* d = &keys[wave][half + 2 * u][2 * (l31 & 15)];      // channels 4 l31 .. + 3: evens to [2 (l31 & 15), + 2), odds to 32 + the same
                *reinterpret_cast<float2*>(d) = make_float2(pre[u].x, pre[u].z);
                *reinterpret_cast<float2*>(d + CVA_KH / 2) = make_float2(pre[u].y, pre[u].w);
            }
        }
    };

    const int ntiles = (a.P + CVA_TK - 1) / CVA_TK;
    prefetch(0);
    __syncthreads();                                  // the maxima are initialised
    for (int tile = 0; tile < ntiles; ++tile) {
        // keys[wave] is this wave's own: its LDS instructions execute in program order, so ordering within the wave suffices (the
        // stores of this tile after the reads of the last one, the reads of this tile after its stores); no workgroup barrier per tile
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float4* arow = reinterpret_cast<const float4*>(&keys[wave][l31][half * (CVA_KH / 2)]);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            wave_lds_order();
            deposit(p);
            wave_lds_order();
            if (p == 1 && tile + 1 < ntiles) prefetch(tile + 1);      // the staged registers are free once both halves are stored
#pragma unroll
            for (int g = 0; g < CVA_KH / 8; ++g) {
                const float4 a4 = arow[g];
                const int t = 32 * p + 4 * g;                          // MFMA step: channel 2 t + half
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, qv[t], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, qv[t + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, qv[t + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, qv[t + 3], acc, 0, 0, 0);
            }
        }

        // this lane: query l31, keys kfirst + (r & 3) + 8 (r >> 2), ascending in r
        const int kfirst = tile * CVA_TK + wave * 32 + 4 * half;
        if (kfirst < a.P) {
            int i = kfirst / a.wc, j = kfirst - i * a.wc;
            int run_i = i;
            float run = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (r > 0) {
                    j += (r & 3) ? 1 : 5;
                    while (j >= a.wc) { j -= a.wc; ++i; }
                }
                const int key = kfirst + (r & 3) + 8 * (r >> 2);
                if (key < a.P) {
                    const float v = acc[r];
                    atomicMax(&cw[l31 * a.sw + j], f2ord(v));
                    if (i != run_i) {
                        atomicMax(&ch[l31 * a.sh + run_i], f2ord(run));
                        run_i = i;
                        run = v;
                    } else {
                        run = fmaxf(run, v);
                    }
                }
            }
            atomicMax(&ch[l31 * a.sh + run_i], f2ord(run));
        }
    }
    __syncthreads();

    // wave v finishes queries 8 v .. 8 v + 7
    for (int u = 0; u < 8; ++u) {
        const int ql = wave * 8 + u, q = q0 + ql;
        if (q >= a.P) break;
        const int iq = q / a.wc, jq = q - iq * a.wc;
        const size_t row = pair * (size_t)a.P + q;
        const float oh = cva_expect(ch + ql * a.sh, a.hc, iq, a.soft_h ? a.soft_h + row * a.hc : nullptr, lane);
        const float ow = cva_expect(cw + ql * a.sw, a.wc, jq, a.soft_w ? a.soft_w + row * a.wc : nullptr, lane);
        if (lane < 4) {                                // nearest x2: the 2 x 2 block of cell (iq, jq)
            const int y = 2 * iq + (lane >> 1), x = 2 * jq + (lane & 1);
            float* o = a.offset + ((pair * (size_t)(2 * a.hc) + y) * (size_t)(2 * a.wc) + x) * 2;
            o[0] = ow;
            o[1] = oh;
        }
    }
}

// ---- pp_trades_render_prehm ------------------------------------------------------------------------------------------------------
// One thread per cell of the pooled map: the 4 x 4 input pixels are rendered in registers (per pixel the maximum over the boxes of the
// Gaussian, evaluated in double and rounded once to float32, as numpy's float64 gaussian2D stored into the float32 map), then summed
// in (ky, kx) order in float32 and divided by 16 (PP_OP_AVGPOOL's rule).
__global__ __launch_bounds__(256) void render_prehm_kernel(const int* __restrict__ boxes, int nb, int hp, int wp, float* __restrict__ out) {
    const int ho = hp >> 2, wo = wp >> 2;
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= ho * wo) return;
    const int oy = cell / wo, ox = cell - oy * wo;
    float px[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) px[k] = 0.f;
    for (int b = 0; b < nb; ++b) {
        const int cx = boxes[3 * b], cy = boxes[3 * b + 1], r = boxes[3 * b + 2];
        if (cx + r < 4 * ox || cx - r > 4 * ox + 3 || cy + r < 4 * oy || cy - r > 4 * oy + 3) continue;
        const double sigma = (double)(2 * r + 1) / 6.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int dy = 4 * oy + (k >> 2) - cy, dx = 4 * ox + (k & 3) - cx;
            if (dx < -r || dx > r || dy < -r || dy > r) continue;
            double g = exp(-(double)(dx * dx + dy * dy) / (2.0 * sigma * sigma));
            if (g < 2.220446049250313e-16) g = 0.0;          // h[h < eps * h.max()] = 0; the maximum (the centre) is 1
            px[k] = fmaxf(px[k], (float)g);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s = s + px[k];
    out[cell] = s / 16.f;
}

// ---- PP_OP_SUB_CAT / PP_OP_BCAST_MUL / PP_OP_BLEND2: the small ops of program B, one thread per (pixel, 4 channels) ----------------
__global__ __launch_bounds__(256) void sub_cat_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ lead,
                                                      float* __restrict__ y, size_t pixels, int c, int c2) {
    const int q4 = (c >> 2) + 1;                       // quad 0: the leading channels
    const size_t total = pixels * q4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / q4;
        const int q = (int)(i - p * q4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q == 0) {
            const float* l = lead + p * c2;
            v.x = l[0];
            if (c2 > 1) v.y = l[1];
            if (c2 > 2) v.z = l[2];
            if (c2 > 3) v.w = l[3];
        } else {
            const float4 x = *reinterpret_cast<const float4*>(a + p * c + 4 * (q - 1));
            const float4 z = *reinterpret_cast<const float4*>(b + p * c + 4 * (q - 1));
            v = make_float4(x.x - z.x, x.y - z.y, x.z - z.z, x.w - z.w);
        }
        *reinterpret_cast<float4*>(y + p * (size_t)(c + 4) + 4 * q) = v;
    }
}

__global__ __launch_bounds__(256) void bcast_mul_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ y,
                                                        size_t pixels, int c) {
    const int q4 = c >> 2;
    const size_t total = pixels * q4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float s = g[i / q4];
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<float4*>(y)[i] = make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
    }
}

__global__ __launch_bounds__(256) void blend2_kernel(const float* __restrict__ x0, const float* __restrict__ x1, const float* __restrict__ l0,
                                                     const float* __restrict__ l1, float* __restrict__ y, size_t pixels, int c) {
    const int q4 = c >> 2;
    const size_t total = pixels * q4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / q4;
        const float a = l0[p], b = l1[p];
        const float m = fmaxf(a, b);
        const float e0 = (float)exp((double)(a - m)), e1 = (float)exp((double)(b - m));
        const float s = e0 + e1;
        const float w0 = e0 / s, w1 = e1 / s;
        const float4 u = reinterpret_cast<const float4*>(x0)[i];
        const float4 v = reinterpret_cast<const float4*>(x1)[i];
        reinterpret_cast<float4*>(y)[i] = make_float4(__fadd_rn(__fmul_rn(w0, u.x), __fmul_rn(w1, v.x)), __fadd_rn(__fmul_rn(w0, u.y), __fmul_rn(w1, v.y)),
                                                      __fadd_rn(__fmul_rn(w0, u.z), __fmul_rn(w1, v.z)), __fadd_rn(__fmul_rn(w0, u.w), __fmul_rn(w1, v.w)));
    }
}

inline int ew_grid(size_t total) { return (int)std::min<size_t>(std::max<size_t>((total + 255) / 256, 1), 65536); }

}  // namespace

int pp_launch_sub_cat(const float* a, const float* b, const float* lead, float* y, size_t pixels, int c, int c2, hipStream_t stream) {
    PP_REQUIRE(a && b && lead && y && pixels > 0 && c > 0 && (c & 3) == 0 && c2 > 0 && c2 <= 4, "sub_cat needs c %% 4 == 0 and 1 .. 4 leading channels");
    hipLaunchKernelGGL(sub_cat_kernel, dim3(ew_grid(pixels * ((c >> 2) + 1))), dim3(256), 0, stream, a, b, lead, y, pixels, c, c2);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_launch_bcast_mul(const float* x, const float* g, float* y, size_t pixels, int c, hipStream_t stream) {
    PP_REQUIRE(x && g && y && pixels > 0 && c > 0 && (c & 3) == 0, "bcast_mul needs c %% 4 == 0");
    hipLaunchKernelGGL(bcast_mul_kernel, dim3(ew_grid(pixels * (c >> 2))), dim3(256), 0, stream, x, g, y, pixels, c);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_launch_blend2(const float* x0, const float* x1, const float* l0, const float* l1, float* y, size_t pixels, int c, hipStream_t stream) {
    PP_REQUIRE(x0 && x1 && l0 && l1 && y && pixels > 0 && c > 0 && (c & 3) == 0, "blend2 needs c %% 4 == 0");
    hipLaunchKernelGGL(blend2_kernel, dim3(ew_grid(pixels * (c >> 2))), dim3(256), 0, stream, x0, x1, l0, l1, y, pixels, c);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

extern "C" {

int pp_trades_cva(pp_ctx* ctx, const float* emb_cur, const float* emb_prev, int n, int hc, int wc, int dim, float* offset,
                  float* soft_h, float* soft_w, int mem) {
    PP_REQUIRE(ctx && emb_cur && emb_prev && offset, "pp_trades_cva: NULL argument");
    PP_REQUIRE(n > 0 && hc > 0 && wc > 0 && dim == CVA_DIM && (long long)hc * wc * CVA_DIM < (1ll << 31) && n <= 65535,
               "pp_trades_cva needs %d-channel embeddings and 0 < n <= 65535", CVA_DIM);
    PP_REQUIRE((soft_h == nullptr) == (soft_w == nullptr), "pp_trades_cva: soft_h and soft_w go together");
    const int P = hc * wc;
    CvaArgs a{};
    a.hc = hc; a.wc = wc; a.P = P; a.sh = hc | 1; a.sw = wc | 1;
    const size_t dyn = (size_t)CVA_TQ * (a.sh + a.sw) * sizeof(int);
    PP_REQUIRE(dyn <= 64 * 1024, "pp_trades_cva: hc + wc = %d exceeds the LDS rows of the maxima (at most 510)", hc + wc);
    const bool host = mem == PP_MEM_HOST;
    const size_t e_bytes = (size_t)n * P * CVA_DIM * 4, o_bytes = (size_t)n * 4 * P * 2 * 4;
    const size_t sh_bytes = (size_t)n * P * hc * 4, sw_bytes = (size_t)n * P * wc * 4;
    hipStream_t s = ctx->stream;
    if (host) {
        size_t need = 2 * ScratchCursor::align(e_bytes) + ScratchCursor::align(o_bytes);
        if (soft_h) need += ScratchCursor::align(sh_bytes) + ScratchCursor::align(sw_bytes);
        int rc = ctx->ensure_scratch(need);
        if (rc != PP_OK) return rc;
        ScratchCursor cur(ctx);
        float* d_cur = cur.take<float>(e_bytes / 4);
        float* d_prev = cur.take<float>(e_bytes / 4);
        a.offset = cur.take<float>(o_bytes / 4);
        if (soft_h) {
            a.soft_h = cur.take<float>(sh_bytes / 4);
            a.soft_w = cur.take<float>(sw_bytes / 4);
        }
        PP_HIP_CHECK(hipMemcpyAsync(d_cur, emb_cur, e_bytes, hipMemcpyHostToDevice, s));
        PP_HIP_CHECK(hipMemcpyAsync(d_prev, emb_prev, e_bytes, hipMemcpyHostToDevice, s));
        a.cur = d_cur; a.prev = d_prev;
    } else {
        a.cur = emb_cur; a.prev = emb_prev; a.offset = offset; a.soft_h = soft_h; a.soft_w = soft_w;
    }
    static PpPerDeviceOnce once;
    once.run([] { (void)hipFuncSetAttribute((const void*)cva_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024); });
    const dim3 grid((P + CVA_TQ - 1) / CVA_TQ, n);
    hipLaunchKernelGGL(cva_kernel, grid, dim3(CVA_THREADS), dyn, s, a);
    PP_HIP_CHECK(hipGetLastError());
    if (host) {
        PP_HIP_CHECK(hipMemcpyAsync(offset, a.offset, o_bytes, hipMemcpyDeviceToHost, s));
        if (soft_h) {
            PP_HIP_CHECK(hipMemcpyAsync(soft_h, a.soft_h, sh_bytes, hipMemcpyDeviceToHost, s));
            PP_HIP_CHECK(hipMemcpyAsync(soft_w, a.soft_w, sw_bytes, hipMemcpyDeviceToHost, s));
        }
        PP_HIP_CHECK(hipStreamSynchronize(s));
    }
    return PP_OK;
}

int pp_trades_render_prehm(pp_ctx* ctx, const int32_t* boxes, int n_boxes, int hp, int wp, float* out, int mem) {
    PP_REQUIRE(ctx && out && (boxes || n_boxes == 0), "pp_trades_render_prehm: NULL argument");
    PP_REQUIRE(n_boxes >= 0 && n_boxes <= 4096 && hp > 0 && wp > 0 && (hp & 3) == 0 && (wp & 3) == 0 && (long long)hp * wp < (1ll << 31),
               "pp_trades_render_prehm needs hp, wp multiples of 4 and at most 4096 boxes");
    for (int b = 0; b < n_boxes; ++b)
        PP_REQUIRE(boxes[3 * b + 2] >= 0 && boxes[3 * b + 2] < (1 << 14) && std::abs(boxes[3 * b]) < (1 << 20) && std::abs(boxes[3 * b + 1]) < (1 << 20),
                   "pp_trades_render_prehm: box %d has a negative or oversized radius or centre", b);
    const bool host = mem == PP_MEM_HOST;
    const size_t cells = (size_t)(hp >> 2) * (wp >> 2);
    size_t need = ScratchCursor::align((size_t)std::max(n_boxes, 1) * 12);
    if (host) need += ScratchCursor::align(cells * 4);
    int rc = ctx->ensure_scratch(need);
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    int* d_boxes = cur.take<int>((size_t)std::max(n_boxes, 1) * 3);
    float* d_out = host ? cur.take<float>(cells) : out;
    hipStream_t s = ctx->stream;
    if (n_boxes) PP_HIP_CHECK(hipMemcpyAsync(d_boxes, boxes, (size_t)n_boxes * 12, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(render_prehm_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_boxes, n_boxes, hp, wp, d_out);
    PP_HIP_CHECK(hipGetLastError());
    if (host) PP_HIP_CHECK(hipMemcpyAsync(out, d_out, cells * 4, hipMemcpyDeviceToHost, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));      // the host boxes must outlive the copy
    return PP_OK;
}

}  // extern "C"
