// PoseC3D (the SkeletonAction stage, pose_pipeline/wrappers/mmaction.py) on the device: what the stage needs besides the layers of
// models/posec3d.py.
//
//   pp_pose_target      mmaction's GeneratePoseTarget(with_kp, use_score, double) for ONE person: per frame and joint one Gaussian
//                       patch, written NHWC with zero pad channels, the mirrored copies (Flip of the key points: x -> w - x for non-zero x,
//                       left / right joints swapped, rendered again) behind the plain ones.  With one person every
//                       channel of a frame holds exactly ONE patch, so the reference's np.maximum(heatmap, patch) over the persons is
//                       a plain store: an output element is a function of its own (frame, joint) key point alone.  That is what makes
//                       the kernel gather-free: no memset + scatter, one thread computes four channels of one pixel and EVERY element
//                       of the output is written exactly once.
//   pp_gather_samples   dst[i] = src[idx[i]] for whole samples, float4 copies: expands the distinct frame maps of a window (or the
//                       front stage's results on them) to clip order.
// mmaction2 is not vendored: UNPINNED restatements, rules in include/posepipe_hip.h, numpy twins in tests/posec3d_ref.py.
#include "pp_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

// The reference's int(): truncation toward zero.  The argument is clamped first so that the conversion is defined for any key point;
// +-2^30 is far outside every map, so the clamp changes no patch.
__device__ __forceinline__ long long trunc_ll(double v) {
    v = v < -1073741824.0 ? -1073741824.0 : (v > 1073741824.0 ? 1073741824.0 : v);
    return (long long)v;
}

// One thread = the four channels [4 q, 4 q + 4) of one pixel of one output sample.
__global__ __launch_bounds__(256) void pose_target_kernel(const double* __restrict__ kps, const int* __restrict__ perm, int n, int K, int h,
                                                          int w, double sigma, int c_pad, float* __restrict__ out) {
    const int cq = c_pad >> 2;
    const long long total = 2ll * n * h * w * cq;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % cq);
    long long r = t / cq;
    const int x = (int)(r % w);
    r /= w;
    const int y = (int)(r % h);
    const int s = (int)(r / h);
    const bool mirrored = s >= n;
    const int f = mirrored ? s - n : s;
    const double r3 = 3.0 * sigma, s2 = sigma * sigma;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * q + j;
        v[j] = 0.f;
        if (c >= K) continue;
        const int k = mirrored ? perm[c] : c;
        if (k < 0 || k >= K) continue;                 // a permutation entry outside [0, K): reads nothing, the channel is zeros
        const double* p = kps + ((size_t)f * K + k) * 3;
        // the mirrored copy: Flip's kp_x[kp_x != 0] = img_width - kp_x, in the key points' own float64
        const double mu_x = mirrored && p[0] != 0.0 ? (double)w - p[0] : p[0], mu_y = p[1], score = p[2];
        if (score < 1e-4) continue;
        const long long st_x = max(trunc_ll(mu_x - r3), 0ll), ed_x = min(trunc_ll(mu_x + r3) + 1, (long long)w);
        const long long st_y = max(trunc_ll(mu_y - r3), 0ll), ed_y = min(trunc_ll(mu_y + r3) + 1, (long long)h);
        if (x < st_x || x >= ed_x || y < st_y || y >= ed_y) continue;
        const double dx = (double)x - mu_x, dy = (double)y - mu_y;
        v[j] = (float)(exp(-(dx * dx + dy * dy) / 2.0 / s2) * score);
    }
    reinterpret_cast<float4*>(out)[t] = make_float4(v[0], v[1], v[2], v[3]);
}

// blockIdx.y = destination sample; the block's threads sweep the sample's float4s.
__global__ __launch_bounds__(256) void gather_samples_kernel(const float4* __restrict__ src, const int* __restrict__ idx, int n_src,
                                                             long long sample_f4, float4* __restrict__ dst) {
    const int i = blockIdx.y;
    const int j = idx[i];
    const bool ok = j >= 0 && j < n_src;
    const float4* s = src + (size_t)(ok ? j : 0) * sample_f4;
    float4* d = dst + (size_t)i * sample_f4;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < sample_f4; e += (long long)gridDim.x * blockDim.x)
        d[e] = ok ? s[e] : make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace

extern "C" {

int pp_pose_target(pp_ctx* ctx, const double* kps, int n, int K, int h, int w, double sigma, const int32_t* perm, int c_pad, float* out) {
    PP_REQUIRE(ctx && kps && perm && out, "pp_pose_target: NULL argument");
    PP_REQUIRE(n > 0 && K > 0 && h > 0 && w > 0 && c_pad >= K && (c_pad & 3) == 0 && sigma > 0.0 && std::isfinite(sigma),
               "pp_pose_target: n %d, K %d, map %d x %d, c_pad %d (a multiple of 4, >= K), sigma %g", n, K, h, w, c_pad, sigma);
    const long long total = 2ll * n * h * w * (c_pad >> 2);
    PP_REQUIRE(total < (1ll << 31) * 256, "pp_pose_target: output too large");
    hipLaunchKernelGGL(pose_target_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, kps, perm, n, K, h, w, sigma,
                       c_pad, out);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_gather_samples(pp_ctx* ctx, const float* src, int n_src, const int32_t* idx, int n, long long sample_floats, float* dst) {
    PP_REQUIRE(ctx && src && idx && dst, "pp_gather_samples: NULL argument");
    PP_REQUIRE(n > 0 && n <= 65535 && n_src > 0 && sample_floats > 0 && (sample_floats & 3) == 0,
               "pp_gather_samples: n %d (1 .. 65535), n_src %d, sample_floats %lld (a positive multiple of 4)", n, n_src, sample_floats);
    PP_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "pp_gather_samples: src and dst must be 16-byte aligned");
    const long long f4 = sample_floats >> 2;
    const unsigned gx = (unsigned)std::min<long long>((f4 + 255) / 256, 64);
    hipLaunchKernelGGL(gather_samples_kernel, dim3(gx, (unsigned)n), dim3(256), 0, ctx->stream, reinterpret_cast<const float4*>(src), idx,
                       n_src, f4, reinterpret_cast<float4*>(dst));
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

}  // extern "C"
