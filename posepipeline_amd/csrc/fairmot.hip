// FairMOT (DLA-34 + DCNv2 heads, one-shot detection + identity embedding) on the device: what `fairmot_bounding_boxes`
// (pose_pipeline/wrappers/fairmot.py:64-141) needs besides plain convolutions.
//
//   PP_OP_DCN3X3            modulated deformable 3x3 convolution (DCNv2), ONE fused kernel: the sampled columns of a tile of 64
//                           output pixels live in LDS only and are multiplied on the matrix cores (v_mfma_f32_32x32x2_f32).  The
//                           upstream extension writes the 9 * cin * h * w column tensor to global memory; here it never leaves the CU.
//   PP_OP_DWDECONV          depthwise ConvTranspose2d(2f, stride f, padding f / 2): at most 2 x 2 input pixels per output pixel
//   pp_fairmot_preprocess   cv2.resize(1920 x 1080) -> letterbox (INTER_AREA + constant border) -> RGB / 255, one pass per frame
//   pp_fairmot_decode       sigmoid, 3x3 peak test, top K, boxes and normalised embeddings of the K peaks
// DCNv2, FairMOT and OpenCV are not vendored: UNPINNED restatements, rules in include/posepipe_hip.h, numpy twins in
// tests/fairmot_ref.py.
#include "pp_internal.h"

#include <algorithm>
#include <cmath>

namespace {

// ---- PP_OP_DCN3X3 --------------------------------------------------------------------------------------------------------------
// Tile: 64 output pixels (flat over h * w of one sample) x all output channels; K = (tap, channel) walked in steps of one tap x 32
// channels.  Per step the 256 threads sample 64 x 32 column values into LDS (transposed, [channel][pixel], row stride 65 floats: the
// MFMA's A operand -- 32 consecutive pixels of one channel per half wave -- reads conflict-free, the 4-byte stores of a float4's
// components are two-way at most), double buffered: the global loads of step s + 1 are issued before the MFMAs of step s and
// their bilinear blend is written after them, so one barrier per step suffices.  The B operand (weights [tap][cin][cout], 32
// consecutive output channels per half wave) is read from global memory: 128-byte rows that stay in L2.
// A wave owns up to four 32 x 32 output blocks: (pixel block = wave & 1) x (channel blocks (wave >> 1) + 2 u).
// Bilinear weights, validity and the sigmoid of the 9 x 64 (tap, pixel) pairs are computed once per tile into LDS.
constexpr int DCN_TP = 64;
constexpr int DCN_CK = 32;
constexpr int DCN_PS = DCN_TP + 1;
constexpr int DCN_THREADS = 256;
constexpr int DCN_MAX_COUT = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct DcnTap {
    float w00, w01, w10, w11, mask;
    int base;        // (y0 * w + x0): the low corner, may be negative (row / column -1)
    int flags;       // bit 0..3: neighbour (0,0), (0,1), (1,0), (1,1) lies inside the map
    int pad_;
};

struct DcnArgs {
    const float* x;      // [n][h][w][cin]
    const float* om;     // [n][h][w][om_c]: 2k = dy, 2k + 1 = dx, 18 + k = mask logit of tap k
    const float* wgt;    // [9][cin_p][cout_p]
    const float* bias;   // [cout_p]
    float* y;            // [n][h][w][cout]
    int h, w, cin, cin_p, cout, cout_p, om_c, relu;
};

__device__ __forceinline__ float sigmoid_d(float v) {
    // evaluated in double, rounded once (the header's convention for transcendentals)
    return (float)(1.0 / (1.0 + exp(-(double)v)));
}

__device__ __forceinline__ float4 dcn_blend(const DcnTap& t, float4 v1, float4 v2, float4 v3, float4 v4) {
    float4 r;
    r.x = (((t.w00 * v1.x + t.w01 * v2.x) + t.w10 * v3.x) + t.w11 * v4.x) * t.mask;
    r.y = (((t.w00 * v1.y + t.w01 * v2.y) + t.w10 * v3.y) + t.w11 * v4.y) * t.mask;
    r.z = (((t.w00 * v1.z + t.w01 * v2.z) + t.w10 * v3.z) + t.w11 * v4.z) * t.mask;
    r.w = (((t.w00 * v1.w + t.w01 * v2.w) + t.w10 * v3.w) + t.w11 * v4.w) * t.mask;
    return r;
}

__global__ __launch_bounds__(DCN_THREADS) void dcn3x3_kernel(DcnArgs a) {
    __shared__ DcnTap taps[9][DCN_TP];
    __shared__ float col[2][DCN_CK][DCN_PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = a.h * a.w;
    const int pix0 = blockIdx.x * DCN_TP;
    const size_t n = blockIdx.y;
    const float* xs = a.x + n * (size_t)hw * a.cin;
    const float* oms = a.om + n * (size_t)hw * a.om_c;

    for (int e = tid; e < 9 * DCN_TP; e += DCN_THREADS) {
        const int tap = e / DCN_TP, p = e - tap * DCN_TP;
        const int pix = pix0 + p;
        DcnTap t;
        t.w00 = t.w01 = t.w10 = t.w11 = 0.f;
        t.mask = 0.f;
        t.base = 0;
        t.flags = 0;
        t.pad_ = 0;
        if (pix < hw) {
            const int yy = pix / a.w, xx = pix - yy * a.w;
            const float* o = oms + (size_t)pix * a.om_c;
            const float py = (float)(yy - 1 + tap / 3) + o[2 * tap];
            const float px = (float)(xx - 1 + tap % 3) + o[2 * tap + 1];
            if (py > -1.f && py < (float)a.h && px > -1.f && px < (float)a.w) {      // NaN offsets fail every comparison: sample 0
                const float fy = floorf(py), fx = floorf(px);
                const int y0 = (int)fy, x0 = (int)fx;
                const float lh = py - fy, lw = px - fx;
                const float hh = 1.f - lh, hw_ = 1.f - lw;
                t.w00 = hh * hw_;
                t.w01 = hh * lw;
                t.w10 = lh * hw_;
                t.w11 = lh * lw;
                t.mask = sigmoid_d(o[18 + tap]);
                t.base = y0 * a.w + x0;
                const int ylo = y0 >= 0, yhi = y0 + 1 <= a.h - 1, xlo = x0 >= 0, xhi = x0 + 1 <= a.w - 1;
                t.flags = (ylo & xlo) | ((ylo & xhi) << 1) | ((yhi & xlo) << 2) | ((yhi & xhi) << 3);
            }
        }
        taps[tap][p] = t;
    }
    __syncthreads();

    const int cchunks = (a.cin + DCN_CK - 1) / DCN_CK;
    const int nsteps = 9 * cchunks;
    const int nb = a.cout_p / 32;
    const int n_units = 2 * nb;
    // sampling items of this thread: pixel sp (+ 32), channel quad sc
    const int sc = tid & 7, sp = tid >> 3;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pre[2][4];

    auto prefetch = [&](int step) {
        const int tap = step / cchunks, c = (step - tap * cchunks) * DCN_CK + 4 * sc;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const DcnTap& t = taps[tap][sp + 32 * i];
            const int fl = c < a.cin ? t.flags : 0;
            const float* p = xs + ((long long)t.base * a.cin + c);
            pre[i][0] = (fl & 1) ? *reinterpret_cast<const float4*>(p) : zero4;
            pre[i][1] = (fl & 2) ? *reinterpret_cast<const float4*>(p + a.cin) : zero4;
            pre[i][2] = (fl & 4) ? *reinterpret_cast<const float4*>(p + (size_t)a.w * a.cin) : zero4;
            pre[i][3] = (fl & 8) ? *reinterpret_cast<const float4*>(p + (size_t)(a.w + 1) * a.cin) : zero4;
        }
    };
    auto deposit = [&](int step) {
        const int tap = step / cchunks, b = step & 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = sp + 32 * i;
            const float4 v = dcn_blend(taps[tap][p], pre[i][0], pre[i][1], pre[i][2], pre[i][3]);
            col[b][4 * sc + 0][p] = v.x;
            col[b][4 * sc + 1][p] = v.y;
            col[b][4 * sc + 2][p] = v.z;
            col[b][4 * sc + 3][p] = v.w;
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
    const int pb = wave & 1, cb0 = wave >> 1;
    const int half = lane >> 5, l31 = lane & 31;

    prefetch(0);
    for (int step = 0; step < nsteps; ++step) {
        deposit(step);
        __syncthreads();
        if (step + 1 < nsteps) prefetch(step + 1);
        const int tap = step / cchunks, ci0 = (step - tap * cchunks) * DCN_CK;
        const float* wrow = a.wgt + ((size_t)tap * a.cin_p + ci0 + half) * a.cout_p + l31;
        const float* arow = &col[step & 1][half][pb * 32 + l31];
        if (wave < n_units) {
#pragma unroll 4
            for (int kk = 0; kk < DCN_CK; kk += 2) {
                const float av = arow[kk * DCN_PS];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int cb = cb0 + 2 * u;
                    if (cb < nb) {
                        const float bv = wrow[(size_t)kk * a.cout_p + cb * 32];
                        acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[u], 0, 0, 0);
                    }
                }
            }
        }
    }

    float* ys = a.y + n * (size_t)hw * a.cout;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int cb = cb0 + 2 * u;
        if (wave >= n_units || cb >= nb) continue;
        const int co = cb * 32 + l31;
        if (co >= a.cout) continue;
        const float bs = a.bias[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int pix = pix0 + pb * 32 + row;
            if (pix < hw) {
                float v = acc[u][r] + bs;
                if (a.relu) v = v > 0.f ? v : 0.f;
                ys[(size_t)pix * a.cout + co] = v;
            }
        }
    }
}

// ---- PP_OP_DWDECONV ------------------------------------------------------------------------------------------------------------
// out[oy][ox][c] = sum over (ky, kx) ascending of x[iy][ix][c] * w[ky][kx][c], iy = (oy + pad - ky) / s where that divides and lies
// in the map; kernel 2 s, padding s / 2: at most two ky and two kx per output pixel.  acc = 0, acc = acc + x * w, no FMA;
// then (+ res).  One thread per (pixel, 4 channels): coalesced over channels.
__global__ __launch_bounds__(256) void dwdeconv_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                       const float* __restrict__ res, float* __restrict__ y, int n, int h, int w,
                                                       int c, int s) {
    const int c4n = c >> 2, ho = h * s, wo = w * s, pad = s >> 1, k = 2 * s;
    const size_t total = (size_t)n * ho * wo * c4n;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        size_t r = i / c4n;
        const int ox = (int)(r % wo);
        r /= wo;
        const int oy = (int)(r % ho);
        const int b = (int)(r / ho);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ky = (oy + pad) % s; ky < k; ky += s) {
            const int iy = (oy + pad - ky) / s;
            if (oy + pad - ky < 0 || iy >= h) continue;
            for (int kx = (ox + pad) % s; kx < k; kx += s) {
                const int ix = (ox + pad - kx) / s;
                if (ox + pad - kx < 0 || ix >= w) continue;
                const float4 xv = *reinterpret_cast<const float4*>(x + (((size_t)b * h + iy) * w + ix) * c + 4 * c4);
                const float4 wv = *reinterpret_cast<const float4*>(wgt + ((size_t)ky * k + kx) * c + 4 * c4);
                acc.x = acc.x + xv.x * wv.x;
                acc.y = acc.y + xv.y * wv.y;
                acc.z = acc.z + xv.z * wv.z;
                acc.w = acc.w + xv.w * wv.w;
            }
        }
        const size_t o = (((size_t)b * ho + oy) * wo + ox) * c + 4 * c4;
        if (res) {
            const float4 rv = *reinterpret_cast<const float4*>(res + o);
            acc.x = acc.x + rv.x;
            acc.y = acc.y + rv.y;
            acc.z = acc.z + rv.z;
            acc.w = acc.w + rv.w;
        }
        *reinterpret_cast<float4*>(y + o) = acc;
    }
}

// ---- pre-processing -------------------------------------------------------------------------------------------------------------
constexpr int FM_W = 1920, FM_H = 1080;   // upstream LoadVideo squeezes every frame to this size first
constexpr int FM_AT = 8;                  // most source cells of one INTER_AREA output cell (scale < 7)

// cv::resize(INTER_LINEAR) 8-bit coefficient table of one axis: (source index, w0, w1), weights * 2048 (as detector.hip)
void linear_table(int src, int dst, std::vector<int32_t>& tab) {
    tab.resize((size_t)dst * 3);
    const double scale = 1.0 / ((double)dst / src);
    for (int d = 0; d < dst; ++d) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(fx);
        fx -= (float)s;
        if (s < 0) { fx = 0.f; s = 0; }
        if (s >= src - 1) { fx = 0.f; s = src - 1; }
        tab[3 * d] = s;
        tab[3 * d + 1] = (int32_t)std::lrintf((1.f - fx) * 2048.f);
        tab[3 * d + 2] = (int32_t)std::lrintf(fx * 2048.f);
    }
}

// cv::resize(INTER_AREA), computeResizeAreaTab: per output cell the first source cell, the count, and float32 weights
bool area_table(int ssize, int dsize, std::vector<int32_t>& ti, std::vector<float>& tf) {
    ti.assign((size_t)dsize * 2, 0);
    tf.assign((size_t)dsize * FM_AT, 0.f);
    const double scale = (double)ssize / dsize;
    for (int dx = 0; dx < dsize; ++dx) {
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        int first = sx1, cnt = 0;
        float* f = &tf[(size_t)dx * FM_AT];
        if (sx1 - fsx1 > 1e-3) {
            first = sx1 - 1;
            f[cnt++] = (float)((sx1 - fsx1) / cell);
        }
        for (int sx = sx1; sx < sx2; ++sx) {
            if (cnt >= FM_AT) return false;
            f[cnt++] = (float)(1.0 / cell);
        }
        if (fsx2 - sx2 > 1e-3) {
            if (cnt >= FM_AT) return false;
            f[cnt++] = (float)(std::min(std::min(fsx2 - sx2, 1.0), cell) / cell);
        }
        ti[2 * dx] = first;
        ti[2 * dx + 1] = cnt;
    }
    return true;
}

struct FmPreArgs {
    const uint8_t* frames;
    float* out;
    int n, src_h, src_w, hp, wp, nh, nw, top, left, identity;
    const int32_t *lx, *ly;        // linear tables src -> 1920 x 1080
    const int32_t *axi, *ayi;      // area tables 1920 x 1080 -> nw x nh
    const float *axf, *ayf;
};

// one pixel of the 1920 x 1080 image: the source pixel, or cv::resize's fixed-point bilinear
__device__ __forceinline__ void fm_stage1(const FmPreArgs& a, const uint8_t* f, int sy, int sx, float v[3]) {
    if (a.identity) {
        const uint8_t* p = f + ((size_t)sy * a.src_w + sx) * 3;
        v[0] = (float)p[0]; v[1] = (float)p[1]; v[2] = (float)p[2];
        return;
    }
    const int x0 = a.lx[3 * sx], ax0 = a.lx[3 * sx + 1], ax1 = a.lx[3 * sx + 2];
    const int y0 = a.ly[3 * sy], b0 = a.ly[3 * sy + 1], b1 = a.ly[3 * sy + 2];
    const int x1 = x0 + 1 < a.src_w ? x0 + 1 : a.src_w - 1, y1 = y0 + 1 < a.src_h ? y0 + 1 : a.src_h - 1;
    const uint8_t* r0 = f + (size_t)y0 * a.src_w * 3;
    const uint8_t* r1 = f + (size_t)y1 * a.src_w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int s0 = r0[3 * x0 + c] * ax0 + r0[3 * x1 + c] * ax1;
        const int s1 = r1[3 * x0 + c] * ax0 + r1[3 * x1 + c] * ax1;
        v[c] = (float)((((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2);
    }
}

__global__ __launch_bounds__(256) void fm_preprocess_kernel(FmPreArgs a) {
    const size_t total = (size_t)a.n * a.hp * a.wp;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % a.wp);
        const size_t r = i / a.wp;
        const int y = (int)(r % a.hp), b = (int)(r / a.hp);
        const int dx = x - a.left, dy = y - a.top;
        float bgr[3] = {128.f, 128.f, 128.f};      // the border: 127.5 stored to u8
        if (dx >= 0 && dx < a.nw && dy >= 0 && dy < a.nh) {
            const uint8_t* f = a.frames + (size_t)b * a.src_h * a.src_w * 3;
            const int sx0 = a.axi[2 * dx], nx = a.axi[2 * dx + 1], sy0 = a.ayi[2 * dy], ny = a.ayi[2 * dy + 1];
            float sum[3] = {0.f, 0.f, 0.f};
            for (int j = 0; j < ny; ++j) {
                float buf[3] = {0.f, 0.f, 0.f};
                for (int k = 0; k < nx; ++k) {
                    float v[3];
                    fm_stage1(a, f, sy0 + j, sx0 + k, v);
                    const float al = a.axf[dx * FM_AT + k];
                    buf[0] = buf[0] + v[0] * al;
                    buf[1] = buf[1] + v[1] * al;
                    buf[2] = buf[2] + v[2] * al;
                }
                const float be = a.ayf[dy * FM_AT + j];
                if (j == 0) {
                    sum[0] = be * buf[0]; sum[1] = be * buf[1]; sum[2] = be * buf[2];
                } else {
                    sum[0] = sum[0] + be * buf[0]; sum[1] = sum[1] + be * buf[1]; sum[2] = sum[2] + be * buf[2];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int q = __float2int_rn(sum[c]);      // saturate_cast<uchar>: round half to even, clamp
                q = q < 0 ? 0 : q > 255 ? 255 : q;
                bgr[c] = (float)q;
            }
        }
        *reinterpret_cast<float4*>(a.out + i * 4) = make_float4(bgr[2] / 255.f, bgr[1] / 255.f, bgr[0] / 255.f, 0.f);
    }
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------
// key = sigmoid bits << 32 | ~flat index: positive floats order like their bit patterns, so descending keys are descending values
// with equal values ranked by the LOWER flat index; keys are unique, a peak's output slot is the number of larger keys -- no result
// depends on the order in which the peaks were appended.
__global__ __launch_bounds__(256) void fm_sigmoid_kernel(const float* __restrict__ hm, float* __restrict__ sig, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) sig[i] = sigmoid_d(hm[i]);
}

__global__ __launch_bounds__(256) void fm_peaks_kernel(const float* __restrict__ sig, int h, int w, unsigned long long* __restrict__ keys,
                                                       int* __restrict__ cnt) {
    const int hw = h * w, f = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hw) return;
    const float* m = sig + (size_t)f * hw;
    const int y = p / w, x = p - y * w;
    const float v = m[p];
    bool keep = true;
    for (int yy = y - 1; yy <= y + 1; ++yy)
        for (int xx = x - 1; xx <= x + 1; ++xx)
            if (yy >= 0 && yy < h && xx >= 0 && xx < w && m[yy * w + xx] > v) keep = false;
    if (keep) {
        const int slot = atomicAdd(&cnt[f], 1);
        keys[(size_t)f * hw + slot] = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xffffffffu - (unsigned)p);
    }
}

// rank of `key` among the np keys of a frame = the number of larger keys (the equal-score rule lives in the key); sh: 256 LDS slots;
// called by every thread of a 256-thread workgroup
__device__ __forceinline__ int fm_rank_of(const unsigned long long* __restrict__ kf, int np, unsigned long long key, unsigned long long* sh) {
    int rank = 0;
    for (int base = 0; base < np; base += 256) {
        sh[threadIdx.x] = base + (int)threadIdx.x < np ? kf[base + threadIdx.x] : 0ull;
        __syncthreads();
        const int lim = np - base < 256 ? np - base : 256;
        for (int j = 0; j < lim; ++j) rank += sh[j] > key;
        __syncthreads();
    }
    return rank;
}

__global__ __launch_bounds__(256) void fm_rank_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ cnt, int h, int w,
                                                      int K, const float* __restrict__ wh, const float* __restrict__ reg,
                                                      float* __restrict__ dets, int* __restrict__ inds) {
    __shared__ unsigned long long sh[256];
    const int hw = h * w, f = blockIdx.y, np = cnt[f];
    if ((int)(blockIdx.x * blockDim.x) >= np) return;            // uniform per workgroup
    const unsigned long long* kf = keys + (size_t)f * hw;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long key = i < np ? kf[i] : ~0ull;
    const int rank = fm_rank_of(kf, np, key, sh);
    if (i < np && rank < K) {
        const int p = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
        const int y = p / w, x = p - y * w;
        const float* r = reg + ((size_t)f * hw + p) * 2;
        const float* q = wh + ((size_t)f * hw + p) * 4;
        const float xs = (float)x + r[0], ys = (float)y + r[1];
        float* d = dets + ((size_t)f * K + rank) * 5;
        d[0] = xs - q[0];
        d[1] = ys - q[1];
        d[2] = xs + q[2];
        d[3] = ys + q[3];
        d[4] = __uint_as_float((unsigned)(key >> 32));
        inds[(size_t)f * K + rank] = p;
    }
}

// F.normalize of the gathered embedding: x / max(||x||_2, 1e-12); one wave per slot, the squares summed lane-wise in channel
// order (c = lane, lane + 64, ...) and then by a butterfly
__global__ __launch_bounds__(64) void fm_feats_kernel(const float* __restrict__ id, const int* __restrict__ inds, int hw, int K, int dim,
                                                      float* __restrict__ feats) {
    const int slot = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    const int p = inds[(size_t)f * K + slot];
    float* o = feats + ((size_t)f * K + slot) * dim;
    if (p < 0) {
        for (int c = lane; c < dim; c += 64) o[c] = 0.f;
        return;
    }
    const float* v = id + ((size_t)f * hw + p) * dim;
    float ss = 0.f;
    for (int c = lane; c < dim; c += 64) ss = ss + v[c] * v[c];
    for (int s = 32; s > 0; s >>= 1) ss = ss + __shfl_xor(ss, s, 64);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    for (int c = lane; c < dim; c += 64) o[c] = v[c] / nrm;
}

__global__ __launch_bounds__(256) void fm_fill_kernel(float* __restrict__ dets, int* __restrict__ inds, size_t slots, int width) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < slots; i += (size_t)gridDim.x * blockDim.x) {
        inds[i] = -1;
        for (int k = 0; k < width; ++k) dets[i * width + k] = 0.f;
    }
}

inline int grid_for(size_t total, int threads, int cap = 65536) {
    const size_t g = (total + threads - 1) / threads;
    return (int)std::min<size_t>(std::max<size_t>(g, 1), (size_t)cap);
}

}  // namespace

int pp_dcn3x3_max_cout() { return DCN_MAX_COUT; }

int pp_launch_dcn3x3(const float* x, const float* om, const float* wgt, const float* bias, float* y, int n, int h, int w, int cin,
                     int cout, int om_c, int relu, hipStream_t stream) {
    PP_REQUIRE(x && om && wgt && bias && y && n > 0 && h > 0 && w > 0, "dcn3x3: bad argument");
    PP_REQUIRE(cin > 0 && (cin & 3) == 0 && cout > 0 && cout <= DCN_MAX_COUT && om_c >= 27,
               "dcn3x3 needs cin %% 4 == 0, 0 < cout <= %d and an offset / mask tensor of at least 27 channels", DCN_MAX_COUT);
    PP_REQUIRE((long long)h * w * std::max(cin, om_c) < (1ll << 31), "dcn3x3: a sample's map exceeds 2^31 elements");
    DcnArgs a{};
    a.x = x; a.om = om; a.wgt = wgt; a.bias = bias; a.y = y;
    a.h = h; a.w = w; a.cin = cin; a.cin_p = (cin + 31) / 32 * 32; a.cout = cout; a.cout_p = (cout + 31) / 32 * 32;
    a.om_c = om_c; a.relu = relu;
    const dim3 grid((h * w + DCN_TP - 1) / DCN_TP, n);
    hipLaunchKernelGGL(dcn3x3_kernel, grid, dim3(DCN_THREADS), 0, stream, a);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_launch_dwdeconv(const float* x, const float* wgt, const float* res, float* y, int n, int h, int w, int c, int stride,
                       hipStream_t stream) {
    PP_REQUIRE(x && wgt && y && n > 0 && h > 0 && w > 0 && c > 0 && (c & 3) == 0 && stride >= 2 && (stride & 1) == 0,
               "dwdeconv needs c %% 4 == 0 and an even stride >= 2");
    const size_t total = (size_t)n * h * stride * w * stride * (c >> 2);
    hipLaunchKernelGGL(dwdeconv_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, x, wgt, res, y, n, h, w, c, stride);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

extern "C" {

int pp_fairmot_input_size(int src_h, int src_w, int32_t* hp, int32_t* wp, int32_t* nh, int32_t* nw, int32_t* top, int32_t* left) {
    PP_REQUIRE(src_h > 0 && src_w > 0 && hp && wp && nh && nw && top && left, "pp_fairmot_input_size: bad argument");
    const int H = src_h > src_w ? 1088 : 608, W = src_h > src_w ? 608 : 1088;
    const double ratio = std::min((double)H / FM_H, (double)W / FM_W);
    const int a = (int)std::nearbyint(FM_W * ratio), b = (int)std::nearbyint(FM_H * ratio);      // Python's round: half to even
    const double dw = (W - a) / 2.0, dh = (H - b) / 2.0;
    *hp = H; *wp = W; *nw = a; *nh = b;
    *top = (int)std::nearbyint(dh - 0.1);
    *left = (int)std::nearbyint(dw - 0.1);
    return PP_OK;
}

int pp_fairmot_preprocess(pp_ctx* ctx, const uint8_t* frames, int n, int src_h, int src_w, int frames_mem, int hp, int wp, int nh,
                          int nw, int top, int left, float* out_device) {
    PP_REQUIRE(ctx && frames && out_device, "pp_fairmot_preprocess: NULL argument");
    PP_REQUIRE(n > 0 && src_h > 0 && src_w > 0 && nh > 0 && nw > 0 && top >= 0 && left >= 0 && top + nh <= hp && left + nw <= wp &&
                   nh <= FM_H && nw <= FM_W, "pp_fairmot_preprocess: the letterbox does not fit the network input");
    std::vector<int32_t> lx, ly, axi, ayi;
    std::vector<float> axf, ayf;
    linear_table(src_w, FM_W, lx);
    linear_table(src_h, FM_H, ly);
    PP_REQUIRE(area_table(FM_W, nw, axi, axf) && area_table(FM_H, nh, ayi, ayf), "pp_fairmot_preprocess: INTER_AREA scale above %d", FM_AT - 1);
    const size_t frame_bytes = (size_t)n * src_h * src_w * 3;
    size_t need = ScratchCursor::align(lx.size() * 4) + ScratchCursor::align(ly.size() * 4) + ScratchCursor::align(axi.size() * 4) +
                  ScratchCursor::align(ayi.size() * 4) + ScratchCursor::align(axf.size() * 4) + ScratchCursor::align(ayf.size() * 4);
    if (frames_mem == PP_MEM_HOST) need += ScratchCursor::align(frame_bytes);
    int rc = ctx->ensure_scratch(need);
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    hipStream_t s = ctx->stream;
    auto up = [&](const void* src, size_t bytes, void* dst) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); };
    int32_t* d_lx = cur.take<int32_t>(lx.size());
    int32_t* d_ly = cur.take<int32_t>(ly.size());
    int32_t* d_axi = cur.take<int32_t>(axi.size());
    int32_t* d_ayi = cur.take<int32_t>(ayi.size());
    float* d_axf = cur.take<float>(axf.size());
    float* d_ayf = cur.take<float>(ayf.size());
    PP_HIP_CHECK(up(lx.data(), lx.size() * 4, d_lx));
    PP_HIP_CHECK(up(ly.data(), ly.size() * 4, d_ly));
    PP_HIP_CHECK(up(axi.data(), axi.size() * 4, d_axi));
    PP_HIP_CHECK(up(ayi.data(), ayi.size() * 4, d_ayi));
    PP_HIP_CHECK(up(axf.data(), axf.size() * 4, d_axf));
    PP_HIP_CHECK(up(ayf.data(), ayf.size() * 4, d_ayf));
    const uint8_t* df = frames;
    if (frames_mem == PP_MEM_HOST) {
        uint8_t* st = cur.take<uint8_t>(frame_bytes);
        PP_HIP_CHECK(up(frames, frame_bytes, st));
        df = st;
    }
    FmPreArgs a{};
    a.frames = df; a.out = out_device; a.n = n; a.src_h = src_h; a.src_w = src_w; a.hp = hp; a.wp = wp; a.nh = nh; a.nw = nw;
    a.top = top; a.left = left; a.identity = src_h == FM_H && src_w == FM_W;
    a.lx = d_lx; a.ly = d_ly; a.axi = d_axi; a.ayi = d_ayi; a.axf = d_axf; a.ayf = d_ayf;
    hipLaunchKernelGGL(fm_preprocess_kernel, dim3(grid_for((size_t)n * hp * wp, 256)), dim3(256), 0, s, a);
    PP_HIP_CHECK(hipGetLastError());
    PP_HIP_CHECK(hipStreamSynchronize(s));      // the host tables must outlive the copies
    return PP_OK;
}

int pp_fairmot_decode(pp_ctx* ctx, const float* hm, const float* wh, const float* reg, const float* id, int n, int h, int w, int K,
                      int id_dim, float* dets, float* feats, int32_t* inds, int mem) {
    PP_REQUIRE(ctx && hm && wh && reg && id && dets && feats && inds, "pp_fairmot_decode: NULL argument");
    PP_REQUIRE(n > 0 && h > 0 && w > 0 && K > 0 && (long long)K <= (long long)h * w && id_dim > 0 && (long long)n * h * w < (1ll << 31),
               "pp_fairmot_decode needs 0 < K <= h * w");
    const size_t hw = (size_t)h * w, slots = (size_t)n * K;
    const bool host = mem == PP_MEM_HOST;
    size_t need = ScratchCursor::align(n * hw * 4) + ScratchCursor::align(n * hw * 8) + ScratchCursor::align((size_t)n * 4);
    if (host) need += ScratchCursor::align(slots * 5 * 4) + ScratchCursor::align(slots * id_dim * 4) + ScratchCursor::align(slots * 4);
    int rc = ctx->ensure_scratch(need);
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    float* sig = cur.take<float>(n * hw);
    unsigned long long* keys = cur.take<unsigned long long>(n * hw);
    int* cnt = cur.take<int>(n);
    float* d_dets = host ? cur.take<float>(slots * 5) : dets;
    float* d_feats = host ? cur.take<float>(slots * id_dim) : feats;
    int* d_inds = host ? cur.take<int>(slots) : inds;
    hipStream_t s = ctx->stream;
    PP_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)n * 4, s));
    // slots beyond the number of peaks: index -1, zeros (torch.topk fills them with zero-valued non-peaks in an unspecified
    // order; their score 0 is below every confidence threshold)
    hipLaunchKernelGGL(fm_fill_kernel, dim3(grid_for(slots, 256)), dim3(256), 0, s, d_dets, d_inds, slots, 5);
    hipLaunchKernelGGL(fm_sigmoid_kernel, dim3(grid_for(n * hw, 256)), dim3(256), 0, s, hm, sig, n * hw);
    const dim3 grid((unsigned)((hw + 255) / 256), n);
    hipLaunchKernelGGL(fm_peaks_kernel, grid, dim3(256), 0, s, sig, h, w, keys, cnt);
    hipLaunchKernelGGL(fm_rank_kernel, grid, dim3(256), 0, s, keys, cnt, h, w, K, wh, reg, d_dets, d_inds);
    hipLaunchKernelGGL(fm_feats_kernel, dim3(K, n), dim3(64), 0, s, id, d_inds, (int)hw, K, id_dim, d_feats);
    PP_HIP_CHECK(hipGetLastError());
    if (host) {
        PP_HIP_CHECK(hipMemcpyAsync(dets, d_dets, slots * 5 * 4, hipMemcpyDeviceToHost, s));
        PP_HIP_CHECK(hipMemcpyAsync(feats, d_feats, slots * id_dim * 4, hipMemcpyDeviceToHost, s));
        PP_HIP_CHECK(hipMemcpyAsync(inds, d_inds, slots * 4, hipMemcpyDeviceToHost, s));
        PP_HIP_CHECK(hipStreamSynchronize(s));
    }
    return PP_OK;
}

}  // extern "C"

// ---- pp_trades_decode (TraDeS, wrappers/trades.py): the peak, key and rank scheme above with CenterTrack's outputs ---------------
namespace {

__global__ __launch_bounds__(256) void trades_rank_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ cnt, int h, int w,
                                                         int K, const float* __restrict__ reg, const float* __restrict__ ltrb,
                                                         const float* __restrict__ trk, float* __restrict__ dets, int* __restrict__ inds) {
    __shared__ unsigned long long sh[256];
    const int hw = h * w, f = blockIdx.y, np = cnt[f];
    if ((int)(blockIdx.x * blockDim.x) >= np) return;            // uniform per workgroup
    const unsigned long long* kf = keys + (size_t)f * hw;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long key = i < np ? kf[i] : ~0ull;
    const int rank = fm_rank_of(kf, np, key, sh);
    if (i < np && rank < K) {
        const int p = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
        const int y = p / w, x = p - y * w;
        const float* r = reg + ((size_t)f * hw + p) * 2;
        const float* q = ltrb + ((size_t)f * hw + p) * 4;
        const float* t = trk + ((size_t)f * hw + p) * 2;
        float* d = dets + ((size_t)f * K + rank) * 9;
        d[0] = (float)x + r[0];
        d[1] = (float)y + r[1];
        d[2] = (float)x + q[0];
        d[3] = (float)y + q[1];
        d[4] = (float)x + q[2];
        d[5] = (float)y + q[3];
        d[6] = t[0];
        d[7] = t[1];
        d[8] = __uint_as_float((unsigned)(key >> 32));
        inds[(size_t)f * K + rank] = p;
    }
}

}  // namespace

extern "C" int pp_trades_decode(pp_ctx* ctx, const float* hm, const float* reg, const float* ltrb, const float* tracking, int n, int h, int w,
                                int K, float* dets, int32_t* inds, int mem) {
    PP_REQUIRE(ctx && hm && reg && ltrb && tracking && dets && inds, "pp_trades_decode: NULL argument");
    PP_REQUIRE(n > 0 && h > 0 && w > 0 && K > 0 && (long long)K <= (long long)h * w && (long long)n * h * w < (1ll << 31),
               "pp_trades_decode needs 0 < K <= h * w");
    const size_t hw = (size_t)h * w, slots = (size_t)n * K;
    const bool host = mem == PP_MEM_HOST;
    size_t need = ScratchCursor::align(n * hw * 4) + ScratchCursor::align(n * hw * 8) + ScratchCursor::align((size_t)n * 4);
    if (host) need += ScratchCursor::align(slots * 9 * 4) + ScratchCursor::align(slots * 4);
    int rc = ctx->ensure_scratch(need);
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    float* sig = cur.take<float>(n * hw);
    unsigned long long* keys = cur.take<unsigned long long>(n * hw);
    int* cnt = cur.take<int>(n);
    float* d_dets = host ? cur.take<float>(slots * 9) : dets;
    int* d_inds = host ? cur.take<int>(slots) : inds;
    hipStream_t s = ctx->stream;
    PP_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(fm_fill_kernel, dim3(grid_for(slots, 256)), dim3(256), 0, s, d_dets, d_inds, slots, 9);
    hipLaunchKernelGGL(fm_sigmoid_kernel, dim3(grid_for(n * hw, 256)), dim3(256), 0, s, hm, sig, n * hw);
    const dim3 grid((unsigned)((hw + 255) / 256), n);
    hipLaunchKernelGGL(fm_peaks_kernel, grid, dim3(256), 0, s, sig, h, w, keys, cnt);
    hipLaunchKernelGGL(trades_rank_kernel, grid, dim3(256), 0, s, keys, cnt, h, w, K, reg, ltrb, tracking, d_dets, d_inds);
    PP_HIP_CHECK(hipGetLastError());
    if (host) {
        PP_HIP_CHECK(hipMemcpyAsync(dets, d_dets, slots * 9 * 4, hipMemcpyDeviceToHost, s));
        PP_HIP_CHECK(hipMemcpyAsync(inds, d_inds, slots * 4, hipMemcpyDeviceToHost, s));
        PP_HIP_CHECK(hipStreamSynchronize(s));
    }
    return PP_OK;
}
