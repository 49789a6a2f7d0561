// pp_ecc_euclidean: ECC image alignment (Evangelidis & Psarakis 2008) of many image pairs at once -- the camera-motion compensation
// of mmtrack's Tracktor configuration (3rdparty/mmtracking/mot/tracktor/tracktor_faster-rcnn_r50_fpn_4e_mot17-private-half.py:
// motion = CameraMotionCompensation(warp_mode MOTION_EUCLIDEAN, num_iters 100, stop_eps 1e-5)), which the reference runs frame after
// frame on the CPU with cv2.findTransformECC.  The pairs of a chunk are independent of one another: all of them advance in the same
// launches.
//
// The algorithm is OpenCV's findTransformECC(template, input, identity, MOTION_EUCLIDEAN, (COUNT + EPS, num_iters, stop_eps),
// inputMask = None, gaussFiltSize = 1), restated here; OpenCV is neither vendored nor pinned, so this text is the definition
// (PARITY UNPINNED; the float64 statement the tests compare with is tests/tracktor_ref.py, written from the same text).
//
//   before the loop   gx, gy = the INPUT image filtered with [-0.5, 0, 0.5] along x / along y, border REFLECT_101
//                     (pixel -1 is pixel 1, pixel w is pixel w - 2); float32.
//   M = identity (2 x 3), rho = -1, last_rho = -stop_eps
//   for (i = 1; i <= num_iters && |rho - last_rho| >= stop_eps; ++i):
//     warp the input image, gx and gy with M: dst(x, y) = src(M (x, y, 1)), bilinear, constant border 0 (every tap outside the
//       image reads 0), with warpAffine's coordinate arithmetic (WARP_INVERSE_MAP, so M itself is used):
//         X = (rint((M01 y + M02) 1024) + 16 + rint(M00 x 1024)) >> 5     Y = (rint((M11 y + M12) 1024) + 16 + rint(M10 x 1024)) >> 5
//         column X >> 5 + (X & 31) / 32, row Y >> 5 + (Y & 31) / 32        (rint: to nearest, ties to even; 1/32 px steps)
//     mask = the all-ones image warped with nearest neighbour: column (rint((M01 y + M02) 1024) + 512 + rint(M00 x 1024)) >> 10
//       (row alike) lies inside the image
//     n = pixels of the mask; mI, mT = mean of the warped image / of the template over the mask
//     Izm = warped image - mI inside the mask (its raw value outside), Tzm = template - mT inside the mask, 0 outside
//     imgNorm = sqrt(sum over the mask of Izm^2), tmpNorm = sqrt(sum of Tzm^2)               (= sqrt(n var))
//     J0 = gx (-X s - Y c) + gy (X c - Y s), J1 = gx, J2 = gy      (c = M00, s = M10, X / Y the pixel's column / row, gx / gy WARPED)
//     H = J^T J, corr = <Tzm, Izm>, ip = J^T Izm, tp = J^T Tzm     (all pixels)
//     last_rho = rho; rho = corr / (imgNorm tmpNorm)               NaN: status PP_ECC_NAN (OpenCV raises)
//     lambda = (imgNorm^2 - ip . H^-1 ip) / (corr - tp . H^-1 ip)  denominator <= 0: status PP_ECC_DIVERGED (OpenCV raises)
//     dp = H^-1 (lambda tp - ip)
//     theta = asin(M10) + dp0; M02 += dp1; M12 += dp2; M00 = M11 = cos theta, M10 = -M01 = sin theta
//   `iters` = loop bodies executed; a pair that ends with a status other than PP_ECC_OK keeps the M it entered that iteration with.
//
// Arithmetic: images, gradients and the template are float32; the interpolation, the Jacobian, every sum, the 3 x 3 solve and M are
// float64 (OpenCV: float32 images and M, float64 dot products).  The sums over the mask are taken of (value - the image's pixel
// (0, 0)), which changes no term of the text above and keeps the variance of a constant image exactly 0.
//
// Shape: one interleaved float4 {I, gx, gy, 0} plane per image, so that one bilinear fetch (four 16-byte taps) serves the three warps.
// An iteration is two launches: ecc_accum_kernel (grid: blocks x pairs) leaves per-workgroup partial sums of the 21 quantities --
// per thread in float64 over a fixed pixel set, then per wave by shuffles, then per workgroup through LDS, no atomics -- and
// ecc_update_kernel (one workgroup per pair) adds the partials in block order, solves and updates on one thread.  num_iters such
// pairs of launches are queued back to back; a per-pair `done` word on the device makes the workgroups of a finished pair return at
// once, so there is no host round trip, no persistent kernel and no grid-wide wait.  Two calls on the same inputs give the same bits.
//
// Traffic: an iteration must read 16 B (plane) + 4 B (template) per pixel and pair; the four taps of neighbouring pixels overlap, so
// the rest is cache hits.  At 608 x 1088 that is 13.2 MB per pair and iteration.
#include <cmath>

#include "pp_internal.h"

namespace {

constexpr int ECC_THREADS = 256;     // 4 waves
constexpr int ECC_NSUM = 21;
constexpr int ECC_MAX_BLOCKS = 128;  // workgroups per pair
constexpr int ECC_PIX_PER_BLOCK = 1024;

struct EccState {
    double m[6];
    double rho, last_rho;
    int32_t iters, status, done, pad;
};

__global__ __launch_bounds__(256) void gray_from_nhwc4_kernel(const float4* __restrict__ x, size_t n_px, int r, int g, int b,
                                                             float* __restrict__ gray) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = x[i];
        auto ch = [&](int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; };
        gray[i] = (0.299f * ch(r) + 0.587f * ch(g)) + 0.114f * ch(b);
    }
}

// {I, gx, gy, 0} of every image; REFLECT_101 at the border (a 1-pixel-wide image has gradient 0)
__global__ __launch_bounds__(256) void ecc_plane_kernel(const float* __restrict__ gray, int n_images, int h, int w,
                                                       float4* __restrict__ plane) {
    const size_t n_px = (size_t)n_images * h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % w), y = (int)((i / w) % h);
        const float* row = gray + (i - x);
        const int xl = x > 0 ? x - 1 : (w > 1 ? 1 : 0), xr = x < w - 1 ? x + 1 : (w > 1 ? w - 2 : 0);
        const int yu = y > 0 ? y - 1 : (h > 1 ? 1 : 0), yd = y < h - 1 ? y + 1 : (h > 1 ? h - 2 : 0);
        const float gx = 0.5f * row[xr] - 0.5f * row[xl];
        const float gy = 0.5f * row[(ptrdiff_t)(yd - y) * w + x] - 0.5f * row[(ptrdiff_t)(yu - y) * w + x];
        plane[i] = make_float4(row[x], gx, gy, 0.f);
    }
}

__global__ void ecc_init_kernel(EccState* __restrict__ st, int n_pairs, int num_iters, double eps) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    EccState s;
    s.m[0] = 1.0; s.m[1] = 0.0; s.m[2] = 0.0; s.m[3] = 0.0; s.m[4] = 1.0; s.m[5] = 0.0;
    s.rho = -1.0; s.last_rho = -eps;
    s.iters = 0; s.status = PP_ECC_OK; s.pad = 0;
    s.done = !(1 <= num_iters && fabs(s.rho - s.last_rho) >= eps);
    st[p] = s;
}

// rint of a coordinate scaled by 1024, as a 64-bit integer; a non-finite or absurd M cannot overflow the conversion (every tap is
// bounds-checked afterwards)
__device__ __forceinline__ long long fix1024(double v) {
    return (long long)rint(fmin(fmax(v, -1e15), 1e15));
}

// one tap of the bilinear fetch: {I, gx, gy, 0} of the pixel, zeros outside the image (constant border)
__device__ __forceinline__ float4 ecc_tap(const float4* __restrict__ P, bool inside, long long idx) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) v = P[idx];
    return v;
}

__global__ __launch_bounds__(ECC_THREADS) void ecc_accum_kernel(const float* __restrict__ gray, const float4* __restrict__ plane,
                                                               const int32_t* __restrict__ pairs, const EccState* __restrict__ st,
                                                               int h, int w, int nblk, double* __restrict__ partial) {
    const int p = blockIdx.y;
    if (st[p].done) return;
    __shared__ double s_red[ECC_THREADS / 64][ECC_NSUM];
    const size_t img_px = (size_t)h * w;
    const float* T = gray + (size_t)pairs[2 * p] * img_px;
    const float4* P = plane + (size_t)pairs[2 * p + 1] * img_px;
    const double m00 = st[p].m[0], m01 = st[p].m[1], m02 = st[p].m[2], m10 = st[p].m[3], m11 = st[p].m[4], m12 = st[p].m[5];
    const double I0 = (double)P[0].x, T0 = (double)T[0];
    double acc[ECC_NSUM];
#pragma unroll
    for (int k = 0; k < ECC_NSUM; ++k) acc[k] = 0.0;
    const int npix = h * w;
    for (int i = blockIdx.x * ECC_THREADS + threadIdx.x; i < npix; i += nblk * ECC_THREADS) {
        const int y = i / w, x = i - y * w;
        const long long ax = fix1024(m00 * (double)x * 1024.0), bx = fix1024(m10 * (double)x * 1024.0);
        const long long x0 = fix1024((m01 * (double)y + m02) * 1024.0), y0 = fix1024((m11 * (double)y + m12) * 1024.0);
        const long long X = (x0 + 16 + ax) >> 5, Y = (y0 + 16 + bx) >> 5;
        const long long sx = X >> 5, sy = Y >> 5;
        const double a = (double)(X & 31) / 32.0, b = (double)(Y & 31) / 32.0;
        const long long nx = (x0 + 512 + ax) >> 10, ny = (y0 + 512 + bx) >> 10;
        const bool in = nx >= 0 && nx < w && ny >= 0 && ny < h;
        const bool cx0 = sx >= 0 && sx < w, cx1 = sx + 1 >= 0 && sx + 1 < w, cy0 = sy >= 0 && sy < h, cy1 = sy + 1 >= 0 && sy + 1 < h;
        const float4 p00 = ecc_tap(P, cy0 && cx0, sy * w + sx), p01 = ecc_tap(P, cy0 && cx1, sy * w + sx + 1);
        const float4 p10 = ecc_tap(P, cy1 && cx0, (sy + 1) * w + sx), p11 = ecc_tap(P, cy1 && cx1, (sy + 1) * w + sx + 1);
        const double w00 = (1.0 - a) * (1.0 - b), w01 = a * (1.0 - b), w10 = (1.0 - a) * b, w11 = a * b;
        const double Iw = w00 * p00.x + w01 * p01.x + w10 * p10.x + w11 * p11.x;
        const double gx = w00 * p00.y + w01 * p01.y + w10 * p10.y + w11 * p11.y;
        const double gy = w00 * p00.z + w01 * p01.z + w10 * p10.z + w11 * p11.z;
        const double Xd = (double)x, Yd = (double)y;
        const double J0 = gx * (-Xd * m10 - Yd * m00) + gy * (Xd * m00 - Yd * m10);
        const double Iz = in ? Iw - I0 : Iw;
        if (in) {
            const double Tz = (double)T[i] - T0;
            acc[0] += 1.0;
            acc[1] += Iz; acc[2] += Tz; acc[3] += Iz * Iz; acc[4] += Tz * Tz; acc[5] += Iz * Tz;
            acc[6] += J0; acc[7] += gx; acc[8] += gy;
            acc[12] += J0 * Tz; acc[13] += gx * Tz; acc[14] += gy * Tz;
        }
        acc[9] += J0 * Iz; acc[10] += gx * Iz; acc[11] += gy * Iz;
        acc[15] += J0 * J0; acc[16] += J0 * gx; acc[17] += J0 * gy;
        acc[18] += gx * gx; acc[19] += gx * gy; acc[20] += gy * gy;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < ECC_NSUM; ++k) {
        double v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_red[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < ECC_NSUM) {
        double v = s_red[0][threadIdx.x];
        for (int k = 1; k < ECC_THREADS / 64; ++k) v += s_red[k][threadIdx.x];
        partial[((size_t)p * nblk + blockIdx.x) * ECC_NSUM + threadIdx.x] = v;
    }
}

// second stage of the sums (block order, float64), then the solve and the update on thread 0
__global__ __launch_bounds__(64) void ecc_update_kernel(const double* __restrict__ partial, int nblk, EccState* __restrict__ st,
                                                        int num_iters, double eps) {
    const int p = blockIdx.x;
    if (st[p].done) return;
    __shared__ double S[ECC_NSUM];
    if (threadIdx.x < ECC_NSUM) {
        const double* q = partial + (size_t)p * nblk * ECC_NSUM + threadIdx.x;
        double v = 0.0;
        for (int k = 0; k < nblk; ++k) v += q[(size_t)k * ECC_NSUM];
        S[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    EccState s = st[p];
    const double n = S[0], mI = S[1] / n, mT = S[2] / n;
    const double img2 = S[3] - n * mI * mI, tmp2 = S[4] - n * mT * mT, corr = S[5] - n * mI * mT;
    const double imgNorm = sqrt(img2), tmpNorm = sqrt(tmp2);
    const double ip[3] = {S[9] - mI * S[6], S[10] - mI * S[7], S[11] - mI * S[8]};
    const double tp[3] = {S[12] - mT * S[6], S[13] - mT * S[7], S[14] - mT * S[8]};
    s.last_rho = s.rho;
    s.rho = corr / (imgNorm * tmpNorm);
    s.iters += 1;
    if (isnan(s.rho)) {
        s.status = PP_ECC_NAN; s.done = 1;
        st[p] = s;
        return;
    }
    // inverse of the symmetric 3 x 3 H by cofactors
    const double h00 = S[15], h01 = S[16], h02 = S[17], h11 = S[18], h12 = S[19], h22 = S[20];
    const double c00 = h11 * h22 - h12 * h12, c01 = h02 * h12 - h01 * h22, c02 = h01 * h12 - h02 * h11;
    const double c11 = h00 * h22 - h02 * h02, c12 = h01 * h02 - h00 * h12, c22 = h00 * h11 - h01 * h01;
    const double det = h00 * c00 + h01 * c01 + h02 * c02;
    const double inv[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
    double a[3];
    for (int r = 0; r < 3; ++r) a[r] = inv[r][0] * ip[0] + inv[r][1] * ip[1] + inv[r][2] * ip[2];
    const double lambda_n = img2 - (ip[0] * a[0] + ip[1] * a[1] + ip[2] * a[2]);
    const double lambda_d = corr - (tp[0] * a[0] + tp[1] * a[1] + tp[2] * a[2]);
    if (!(lambda_d > 0.0)) {
        s.status = PP_ECC_DIVERGED; s.done = 1;
        st[p] = s;
        return;
    }
    const double lambda = lambda_n / lambda_d;
    const double e[3] = {lambda * tp[0] - ip[0], lambda * tp[1] - ip[1], lambda * tp[2] - ip[2]};
    double dp[3];
    for (int r = 0; r < 3; ++r) dp[r] = inv[r][0] * e[0] + inv[r][1] * e[1] + inv[r][2] * e[2];
    const double theta = asin(s.m[3]) + dp[0];
    s.m[2] += dp[1];
    s.m[5] += dp[2];
    s.m[0] = cos(theta); s.m[4] = s.m[0];
    s.m[3] = sin(theta); s.m[1] = -s.m[3];
    s.done = !(s.iters + 1 <= num_iters && fabs(s.rho - s.last_rho) >= eps);
    st[p] = s;
}

}  // namespace

extern "C" {

int pp_gray_from_nhwc4(pp_ctx* ctx, const float* x_nhwc4, int n, int h, int w, int r, int g, int b, float* gray) {
    PP_REQUIRE(ctx && x_nhwc4 && gray, "pp_gray_from_nhwc4: NULL argument");
    PP_REQUIRE(n > 0 && h > 0 && w > 0, "pp_gray_from_nhwc4: bad dims %d x %d x %d", n, h, w);
    PP_REQUIRE(r >= 0 && r < 4 && g >= 0 && g < 4 && b >= 0 && b < 4, "pp_gray_from_nhwc4: channel indices must be in [0, 4)");
    const size_t n_px = (size_t)n * h * w;
    const unsigned grid = (unsigned)std::min<size_t>((n_px + 255) / 256, 2048);
    hipLaunchKernelGGL(gray_from_nhwc4_kernel, dim3(grid), dim3(256), 0, ctx->stream, reinterpret_cast<const float4*>(x_nhwc4), n_px, r, g,
                       b, gray);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

int pp_ecc_euclidean(pp_ctx* ctx, const float* gray, int n_images, int h, int w, const int32_t* pairs, int n_pairs, int num_iters,
                     double stop_eps, double* warp, double* rho, int32_t* iters, int32_t* status) {
    PP_REQUIRE(ctx && gray && pairs && warp && rho && iters && status, "pp_ecc_euclidean: NULL argument");
    PP_REQUIRE(n_images > 0 && h > 0 && w > 0 && (size_t)h * w < (size_t)1 << 30, "pp_ecc_euclidean: bad dims %d x %d x %d", n_images, h, w);
    PP_REQUIRE(n_pairs > 0 && n_pairs <= 65535 && num_iters >= 0, "pp_ecc_euclidean: %d pairs, %d iterations", n_pairs, num_iters);
    for (int i = 0; i < 2 * n_pairs; ++i)
        PP_REQUIRE(pairs[i] >= 0 && pairs[i] < n_images, "pp_ecc_euclidean: pair %d names image %d of %d", i / 2, pairs[i], n_images);
    const size_t img_px = (size_t)h * w, n_px = img_px * n_images;
    const int nblk = (int)std::min<size_t>((img_px + ECC_PIX_PER_BLOCK - 1) / ECC_PIX_PER_BLOCK, ECC_MAX_BLOCKS);
    const size_t need = ScratchCursor::align(n_px * sizeof(float4)) + ScratchCursor::align((size_t)n_pairs * 2 * sizeof(int32_t)) +
                        ScratchCursor::align((size_t)n_pairs * sizeof(EccState)) +
                        ScratchCursor::align((size_t)n_pairs * nblk * ECC_NSUM * sizeof(double));
    int rc = ctx->ensure_scratch(need);
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    float4* plane = cur.take<float4>(n_px);
    int32_t* d_pairs = cur.take<int32_t>((size_t)n_pairs * 2);
    EccState* st = cur.take<EccState>(n_pairs);
    double* partial = cur.take<double>((size_t)n_pairs * nblk * ECC_NSUM);
    hipStream_t s = ctx->stream;
    PpRange range("ecc");
    PP_HIP_CHECK(hipMemcpyAsync(d_pairs, pairs, (size_t)n_pairs * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ecc_plane_kernel, dim3((unsigned)std::min<size_t>((n_px + 255) / 256, 2048)), dim3(256), 0, s, gray, n_images, h, w, plane);
    hipLaunchKernelGGL(ecc_init_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, s, st, n_pairs, num_iters, stop_eps);
    for (int it = 0; it < num_iters; ++it) {
        hipLaunchKernelGGL(ecc_accum_kernel, dim3(nblk, n_pairs), dim3(ECC_THREADS), 0, s, gray, plane, d_pairs, st, h, w, nblk, partial);
        hipLaunchKernelGGL(ecc_update_kernel, dim3(n_pairs), dim3(64), 0, s, partial, nblk, st, num_iters, stop_eps);
    }
    PP_HIP_CHECK(hipGetLastError());
    std::vector<EccState> hs(n_pairs);
    PP_HIP_CHECK(hipMemcpyAsync(hs.data(), st, (size_t)n_pairs * sizeof(EccState), hipMemcpyDeviceToHost, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));
    for (int p = 0; p < n_pairs; ++p) {
        for (int k = 0; k < 6; ++k) warp[6 * p + k] = hs[p].m[k];
        rho[p] = hs[p].rho;
        iters[p] = hs[p].iters;
        status[p] = hs[p].status;
    }
    return PP_OK;
}

}  // extern "C"
