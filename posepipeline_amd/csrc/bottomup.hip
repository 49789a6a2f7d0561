// Associative-embedding post-processing of the bottom-up stage (HigherHRNet), on the device.
//
// Replaces, for `mmpose_bottom_up` (pose_pipeline/wrappers/mmpose.py:84-121), what mmpose 0.x runs on the host after the
// network (test_cfg of 3rdparty/mmpose/config/bottom_up/higherhrnet/coco/higher_hrnet48_coco_512x512.py:109-125):
//   flip_feature_maps + aggregate_stage_flip   (mirror, channel permutation, bilinear projection to the input size, average)
//   HeatmapParser.nms + top_k                  (5x5 local maxima, the max_num_people largest per joint)
//   HeatmapParser.refine                       (argmax of hm - round(|tag - mean tag|) per person and missing joint)
// mmpose is not vendored: an UNPINNED restatement, rules in include/posepipe_hip.h.  At 1080p these work on 17 x 512 x 960 maps per
// frame; the host gets 30 candidates per joint and one position per refined joint and never touches a map.
//
// What is stored: the aggregated heat-maps (the 5x5 test reads every pixel 25 times and needs four bilinear samples per read
// otherwise).  The tags are NOT stored: they are needed at <= 30 pixels per joint and in the refine scan only, and their source
// (one low-resolution plane per tag) stays in cache; `tag_at` is the one place that evaluates them, so the candidate pass and the
// refine pass see the same bits.
//
// Selection is by a 64-bit key (value bits << 32 | ~flat index): positive floats order like their bit patterns, so the maximum
// key is the largest value at the lowest index, keys are unique, and "the next one" is the largest key below the previous one --
// no list is modified, no atomics, the result does not depend on the launch shape.
#include "pp_internal.h"

namespace {

constexpr int BU_THREADS = 256;
constexpr int BU_PER_THREAD = 16;
constexpr int BU_TILE = BU_THREADS * BU_PER_THREAD;   // pixels of one plane per workgroup of the candidate pass
constexpr int BU_MAX_PEOPLE = 64;
constexpr int BU_REFINE_SPAN = 8192;                  // pixels per workgroup of the refine scan (at least)
constexpr int BU_REFINE_MAX_SPLIT = 64;

struct BuArgs {
    const float* s0;
    int n_frames, k, h0, w0, hr, wr, align;
    float sy0, sx0;       // source step per output pixel of the s0 maps
};

__host__ __device__ inline float bu_scale(int in, int out, int align) {
    // torch area_pixel_compute_scale<float>
    if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    return (float)in / (float)out;
}

__device__ __forceinline__ float bu_src(float scale, int dst, int align) {
    if (align) return scale * (float)dst;
    const float s = scale * ((float)dst + 0.5f) - 0.5f;
    return s < 0.f ? 0.f : s;
}

// F.interpolate(mode='bilinear') of one [h][w] plane at output pixel (y, x), float32; flip: the plane is mirrored in x first
__device__ __forceinline__ float bu_bilinear(const float* __restrict__ p, int h, int w, float sy, float sx, int y, int x,
                                             int align, int flip) {
    const float fy = bu_src(sy, y, align), fx = bu_src(sx, x, align);
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 > h - 1 ? h - 1 : y0;
    x0 = x0 > w - 1 ? w - 1 : x0;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const int c0 = flip ? w - 1 - x0 : x0, c1 = flip ? w - 1 - x1 : x1;
    const float a00 = p[(size_t)y0 * w + c0], a01 = p[(size_t)y0 * w + c1];
    const float a10 = p[(size_t)y1 * w + c0], a11 = p[(size_t)y1 * w + c1];
    return ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11);
}

// the two tag dimensions of joint c of frame f at pixel (y, x): the plain map and the mirrored one (channel perm[c])
__device__ __forceinline__ void tag_at(const BuArgs& a, const int32_t* __restrict__ perm, int f, int c, int y, int x, float& t0,
                                       float& t1) {
    const size_t plane = (size_t)a.h0 * a.w0;
    const float* p0 = a.s0 + ((size_t)f * 2 * a.k + a.k + c) * plane;
    const float* p1 = a.s0 + ((size_t)(a.n_frames + f) * 2 * a.k + a.k + perm[c]) * plane;
    t0 = bu_bilinear(p0, a.h0, a.w0, a.sy0, a.sx0, y, x, a.align, 0);
    t1 = bu_bilinear(p1, a.h0, a.w0, a.sy0, a.sx0, y, x, a.align, 1);
}

__global__ __launch_bounds__(BU_THREADS) void bu_aggregate_kernel(BuArgs a, const float* __restrict__ s1, int h1, int w1, float sy1,
                                                                  float sx1, const int32_t* __restrict__ perm,
                                                                  float* __restrict__ hm) {
    const size_t npix = (size_t)a.hr * a.wr;
    const size_t total = (size_t)a.n_frames * a.k * npix;
    const size_t pl0 = (size_t)a.h0 * a.w0, pl1 = (size_t)h1 * w1;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t fc = i / npix;
        const int p = (int)(i - fc * npix);
        const int f = (int)(fc / a.k), c = (int)(fc - (size_t)f * a.k);
        const int y = p / a.wr, x = p - y * a.wr;
        const int cf = perm[c];
        float v = 0.f;
        v = v + bu_bilinear(a.s0 + ((size_t)f * 2 * a.k + c) * pl0, a.h0, a.w0, a.sy0, a.sx0, y, x, a.align, 0);
        v = v + bu_bilinear(s1 + ((size_t)f * a.k + c) * pl1, h1, w1, sy1, sx1, y, x, a.align, 0);
        v = v + bu_bilinear(a.s0 + ((size_t)(a.n_frames + f) * 2 * a.k + cf) * pl0, a.h0, a.w0, a.sy0, a.sx0, y, x, a.align, 1);
        v = v + bu_bilinear(s1 + ((size_t)(a.n_frames + f) * a.k + cf) * pl1, h1, w1, sy1, sx1, y, x, a.align, 1);
        hm[i] = v / 4.f;
    }
}

__device__ __forceinline__ unsigned long long bu_block_max(unsigned long long v, unsigned long long* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = BU_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            const unsigned long long o = sh[t + s];
            if (o > sh[t]) sh[t] = o;
        }
        __syncthreads();
    }
    const unsigned long long r = sh[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ unsigned long long bu_key(unsigned value_bits, int p) {
    return ((unsigned long long)value_bits << 32) | (unsigned long long)(0xffffffffu - (unsigned)p);
}

// pass 1: the max_people best survivors (value > 0) of one tile of one plane -> part[plane][tile][max_people], 0 = none
__global__ __launch_bounds__(BU_THREADS) void bu_candidates_tile_kernel(const float* __restrict__ hm, int hr, int wr, int max_people,
                                                                        unsigned long long* __restrict__ part) {
    __shared__ unsigned long long sh[BU_THREADS];
    const int npix = hr * wr;
    const float* m = hm + (size_t)blockIdx.y * npix;
    unsigned long long keys[BU_PER_THREAD];
#pragma unroll
    for (int i = 0; i < BU_PER_THREAD; ++i) {
        const int p = blockIdx.x * BU_TILE + i * BU_THREADS + threadIdx.x;
        unsigned long long key = 0;
        if (p < npix) {
            const float v = m[p];
            if (v > 0.f) {
                const int y = p / wr, x = p - y * wr;
                const int ya = y - 2 < 0 ? 0 : y - 2, yb = y + 2 > hr - 1 ? hr - 1 : y + 2;
                const int xa = x - 2 < 0 ? 0 : x - 2, xb = x + 2 > wr - 1 ? wr - 1 : x + 2;
                bool keep = true;
                for (int yy = ya; yy <= yb && keep; ++yy)
                    for (int xx = xa; xx <= xb; ++xx)
                        if (m[(size_t)yy * wr + xx] > v) { keep = false; break; }
                if (keep) key = bu_key(__float_as_uint(v), p);
            }
        }
        keys[i] = key;
    }
    unsigned long long* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * max_people;
    unsigned long long prev = ~0ull;
    int r = 0;
    for (; r < max_people; ++r) {
        unsigned long long local = 0;
#pragma unroll
        for (int i = 0; i < BU_PER_THREAD; ++i)
            if (keys[i] < prev && keys[i] > local) local = keys[i];
        const unsigned long long best = bu_block_max(local, sh);     // the same value in every thread
        if (best == 0) break;
        if (threadIdx.x == 0) out[r] = best;
        prev = best;
    }
    for (int j = r + threadIdx.x; j < max_people; j += BU_THREADS) out[j] = 0;
}

// pass 2: merge the tiles of one plane, then one thread per candidate writes its record
__global__ __launch_bounds__(BU_THREADS) void bu_candidates_merge_kernel(BuArgs a, const float* __restrict__ hm,
                                                                         const int32_t* __restrict__ perm,
                                                                         const unsigned long long* __restrict__ part, int n_tiles,
                                                                         int max_people, float* __restrict__ cand) {
    __shared__ unsigned long long sh[BU_THREADS];
    __shared__ unsigned long long sel[BU_MAX_PEOPLE];
    const int plane = blockIdx.x;
    const int n_keys = n_tiles * max_people;
    const unsigned long long* keys = part + (size_t)plane * n_keys;
    for (int j = threadIdx.x; j < max_people; j += BU_THREADS) sel[j] = 0;
    __syncthreads();
    unsigned long long prev = ~0ull;
    for (int r = 0; r < max_people; ++r) {
        unsigned long long local = 0;
        for (int j = threadIdx.x; j < n_keys; j += BU_THREADS) {
            const unsigned long long key = keys[j];
            if (key < prev && key > local) local = key;
        }
        const unsigned long long best = bu_block_max(local, sh);
        if (best == 0) break;
        if (threadIdx.x == 0) sel[r] = best;
        prev = best;
    }
    __syncthreads();
    if ((int)threadIdx.x < max_people) {
        const unsigned long long key = sel[threadIdx.x];
        float* o = cand + ((size_t)plane * max_people + threadIdx.x) * 8;
        if (key == 0) {
            o[0] = 0.f; o[1] = -1.f; o[2] = -1.f; o[3] = 0.f; o[4] = 0.f; o[5] = 0.f; o[6] = 0.f; o[7] = -1.f;
        } else {
            const int p = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
            const int y = p / a.wr, x = p - y * a.wr;
            const int f = plane / a.k, c = plane - f * a.k;
            const float* m = hm + (size_t)plane * a.hr * a.wr;
            float t0, t1;
            tag_at(a, perm, f, c, y, x, t0, t1);
            const int yu = y + 1 > a.hr - 1 ? a.hr - 1 : y + 1, yd = y - 1 < 0 ? 0 : y - 1;
            const int xu = x + 1 > a.wr - 1 ? a.wr - 1 : x + 1, xd = x - 1 < 0 ? 0 : x - 1;
            o[0] = __uint_as_float((unsigned)(key >> 32));
            o[1] = (float)x;
            o[2] = (float)y;
            o[3] = t0;
            o[4] = t1;
            o[5] = m[(size_t)yu * a.wr + x] > m[(size_t)yd * a.wr + x] ? 1.f : 0.f;
            o[6] = m[(size_t)y * a.wr + xu] > m[(size_t)y * a.wr + xd] ? 1.f : 0.f;
            o[7] = (float)p;
        }
    }
}

__device__ __forceinline__ unsigned bu_orderable(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// refine, pass 1: grid (split, joint, person); the best key of one span of the map -> part[person][joint][split]
__global__ __launch_bounds__(BU_THREADS) void bu_refine_scan_kernel(BuArgs a, const float* __restrict__ hm,
                                                                    const int32_t* __restrict__ perm,
                                                                    const int32_t* __restrict__ person_frame,
                                                                    const float* __restrict__ mean_tag,
                                                                    const int32_t* __restrict__ need,
                                                                    unsigned long long* __restrict__ part) {
    __shared__ unsigned long long sh[BU_THREADS];
    const int c = blockIdx.y, person = blockIdx.z;
    if (!need[person * a.k + c]) return;                  // uniform over the workgroup
    const int f = person_frame[person];
    const float m0 = mean_tag[2 * person], m1 = mean_tag[2 * person + 1];
    const int npix = a.hr * a.wr;
    const int span = (npix + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * span, hi = lo + span < npix ? lo + span : npix;
    const float* m = hm + ((size_t)f * a.k + c) * npix;
    unsigned long long local = 0;
    for (int p = lo + threadIdx.x; p < hi; p += BU_THREADS) {
        const int y = p / a.wr, x = p - y * a.wr;
        float t0, t1;
        tag_at(a, perm, f, c, y, x, t0, t1);
        const float d0 = t0 - m0, d1 = t1 - m1;
        const float dist = sqrtf(d0 * d0 + d1 * d1);
        const float score = (m[p] - rintf(dist)) + 0.f;       // + 0: one zero, as numpy compares them
        if (score == score) {                             // a NaN never wins
            const unsigned long long key = bu_key(bu_orderable(score), p);
            if (key > local) local = key;
        }
    }
    const unsigned long long best = bu_block_max(local, sh);
    if (threadIdx.x == 0) part[((size_t)person * a.k + c) * gridDim.x + blockIdx.x] = best;
}

// refine, pass 2: one thread per (person, joint)
__global__ __launch_bounds__(BU_THREADS) void bu_refine_merge_kernel(BuArgs a, const float* __restrict__ hm,
                                                                     const int32_t* __restrict__ person_frame,
                                                                     const int32_t* __restrict__ need,
                                                                     const unsigned long long* __restrict__ part, int n_split,
                                                                     int n_person, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_person * a.k) return;
    float* o = out + (size_t)i * 4;
    o[0] = o[1] = o[2] = o[3] = 0.f;
    if (!need[i]) return;
    unsigned long long best = 0;
    for (int s = 0; s < n_split; ++s) {
        const unsigned long long key = part[(size_t)i * n_split + s];
        if (key > best) best = key;
    }
    if (best == 0) return;
    const int person = i / a.k, c = i - person * a.k;
    const int p = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
    const int y = p / a.wr, x = p - y * a.wr;
    const float* m = hm + ((size_t)person_frame[person] * a.k + c) * a.hr * a.wr;
    const int yu = y + 1 > a.hr - 1 ? a.hr - 1 : y + 1, yd = y - 1 < 0 ? 0 : y - 1;
    const int xu = x + 1 > a.wr - 1 ? a.wr - 1 : x + 1, xd = x - 1 < 0 ? 0 : x - 1;
    const int by = m[(size_t)yu * a.wr + x] > m[(size_t)yd * a.wr + x] ? 1 : 0;
    const int bx = m[(size_t)y * a.wr + xu] > m[(size_t)y * a.wr + xd] ? 2 : 0;
    o[0] = (float)x;
    o[1] = (float)y;
    o[2] = m[p];
    o[3] = (float)(by | bx);
}

int bu_check(const char* what, pp_ctx* ctx, const void* s0, int n_frames, int k, int h0, int w0, const int32_t* flip_perm, int hr,
             int wr) {
    PP_REQUIRE(ctx && s0 && flip_perm, "%s: NULL argument", what);
    PP_REQUIRE(n_frames >= 0 && k > 0 && k <= 1024 && h0 > 0 && w0 > 0 && hr > 0 && wr > 0, "%s: empty dims", what);
    PP_REQUIRE((long long)hr * wr < (1ll << 31) && (long long)h0 * w0 < (1ll << 31), "%s: a map of 2^31 pixels or more", what);
    for (int c = 0; c < k; ++c) PP_REQUIRE(flip_perm[c] >= 0 && flip_perm[c] < k, "%s: flip_perm[%d] out of range", what, c);
    return PP_OK;
}

BuArgs bu_args(const float* s0, int n_frames, int k, int h0, int w0, int hr, int wr, int align) {
    BuArgs a;
    a.s0 = s0; a.n_frames = n_frames; a.k = k; a.h0 = h0; a.w0 = w0; a.hr = hr; a.wr = wr; a.align = align ? 1 : 0;
    a.sy0 = bu_scale(h0, hr, a.align);
    a.sx0 = bu_scale(w0, wr, a.align);
    return a;
}

}  // namespace

extern "C" int pp_bottomup_aggregate(pp_ctx* ctx, const float* s0, const float* s1, int n_frames, int k, int h0, int w0, int h1,
                                     int w1, const int32_t* flip_perm, int hr, int wr, int align_corners, float* hm) {
    int rc = bu_check("pp_bottomup_aggregate", ctx, s0, n_frames, k, h0, w0, flip_perm, hr, wr);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(s1 && hm && h1 > 0 && w1 > 0 && (long long)h1 * w1 < (1ll << 31), "pp_bottomup_aggregate: second map");
    if (n_frames == 0) return PP_OK;
    rc = ctx->ensure_scratch(ScratchCursor::align(k * sizeof(int32_t)));
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    hipStream_t s = ctx->stream;
    int32_t* dperm = cur.take<int32_t>(k);
    PP_HIP_CHECK(hipMemcpyAsync(dperm, flip_perm, k * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const BuArgs a = bu_args(s0, n_frames, k, h0, w0, hr, wr, align_corners);
    const size_t total = (size_t)n_frames * k * hr * wr;
    const unsigned blocks = (unsigned)std::min<size_t>((total + BU_THREADS - 1) / BU_THREADS, (size_t)1 << 20);
    hipLaunchKernelGGL(bu_aggregate_kernel, dim3(blocks), dim3(BU_THREADS), 0, s, a, s1, h1, w1, bu_scale(h1, hr, a.align),
                       bu_scale(w1, wr, a.align), dperm, hm);
    PP_HIP_CHECK(hipGetLastError());
    PP_HIP_CHECK(hipStreamSynchronize(s));      // the permutation lives in ctx scratch
    return PP_OK;
}

extern "C" int pp_bottomup_candidates(pp_ctx* ctx, const float* hm, const float* s0, int n_frames, int k, int h0, int w0,
                                      const int32_t* flip_perm, int hr, int wr, int align_corners, int max_people, float* cand) {
    int rc = bu_check("pp_bottomup_candidates", ctx, s0, n_frames, k, h0, w0, flip_perm, hr, wr);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(hm && cand, "pp_bottomup_candidates: NULL argument");
    PP_REQUIRE(max_people > 0 && max_people <= BU_MAX_PEOPLE, "pp_bottomup_candidates: max_people %d not in 1 .. %d", max_people,
               BU_MAX_PEOPLE);
    if (n_frames == 0) return PP_OK;
    const int npix = hr * wr;
    const int n_tiles = (npix + BU_TILE - 1) / BU_TILE;
    const size_t planes = (size_t)n_frames * k;
    PP_REQUIRE(planes <= 65535, "pp_bottomup_candidates: %zu planes in one call (at most 65535)", planes);
    const size_t n_part = planes * n_tiles * max_people, n_cand = planes * max_people * 8;
    rc = ctx->ensure_scratch(ScratchCursor::align(k * sizeof(int32_t)) + ScratchCursor::align(n_part * sizeof(unsigned long long)) +
                             ScratchCursor::align(n_cand * sizeof(float)));
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    hipStream_t s = ctx->stream;
    int32_t* dperm = cur.take<int32_t>(k);
    unsigned long long* part = cur.take<unsigned long long>(n_part);
    float* dcand = cur.take<float>(n_cand);
    PP_HIP_CHECK(hipMemcpyAsync(dperm, flip_perm, k * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const BuArgs a = bu_args(s0, n_frames, k, h0, w0, hr, wr, align_corners);
    hipLaunchKernelGGL(bu_candidates_tile_kernel, dim3(n_tiles, (unsigned)planes), dim3(BU_THREADS), 0, s, hm, hr, wr, max_people, part);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bu_candidates_merge_kernel, dim3((unsigned)planes), dim3(BU_THREADS), 0, s, a, hm, dperm, part, n_tiles,
                       max_people, dcand);
    PP_HIP_CHECK(hipGetLastError());
    PP_HIP_CHECK(hipMemcpyAsync(cand, dcand, n_cand * sizeof(float), hipMemcpyDeviceToHost, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));
    return PP_OK;
}

extern "C" int pp_bottomup_refine(pp_ctx* ctx, const float* hm, const float* s0, int n_frames, int k, int h0, int w0,
                                  const int32_t* flip_perm, int hr, int wr, int align_corners, int n_person,
                                  const int32_t* person_frame, const float* mean_tag, const int32_t* need, float* out) {
    int rc = bu_check("pp_bottomup_refine", ctx, s0, n_frames, k, h0, w0, flip_perm, hr, wr);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(n_person >= 0, "pp_bottomup_refine: n_person");
    if (n_person == 0) return PP_OK;
    PP_REQUIRE(hm && person_frame && mean_tag && need && out, "pp_bottomup_refine: NULL argument");
    PP_REQUIRE(n_person <= 65535 && k <= 65535, "pp_bottomup_refine: %d persons in one call (at most 65535)", n_person);
    for (int p = 0; p < n_person; ++p)
        PP_REQUIRE(person_frame[p] >= 0 && person_frame[p] < n_frames, "pp_bottomup_refine: person_frame[%d]=%d out of range", p,
                   person_frame[p]);
    const int npix = hr * wr;
    const int n_split = std::max(1, std::min(BU_REFINE_MAX_SPLIT, npix / BU_REFINE_SPAN));
    const size_t pk = (size_t)n_person * k;
    rc = ctx->ensure_scratch(ScratchCursor::align(k * sizeof(int32_t)) + ScratchCursor::align(n_person * sizeof(int32_t)) +
                             ScratchCursor::align(2 * n_person * sizeof(float)) + ScratchCursor::align(pk * sizeof(int32_t)) +
                             ScratchCursor::align(pk * n_split * sizeof(unsigned long long)) + ScratchCursor::align(pk * 4 * sizeof(float)));
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    hipStream_t s = ctx->stream;
    int32_t* dperm = cur.take<int32_t>(k);
    int32_t* dframe = cur.take<int32_t>(n_person);
    float* dmean = cur.take<float>(2 * (size_t)n_person);
    int32_t* dneed = cur.take<int32_t>(pk);
    unsigned long long* part = cur.take<unsigned long long>(pk * n_split);
    float* dout = cur.take<float>(pk * 4);
    PP_HIP_CHECK(hipMemcpyAsync(dperm, flip_perm, k * sizeof(int32_t), hipMemcpyHostToDevice, s));
    PP_HIP_CHECK(hipMemcpyAsync(dframe, person_frame, n_person * sizeof(int32_t), hipMemcpyHostToDevice, s));
    PP_HIP_CHECK(hipMemcpyAsync(dmean, mean_tag, 2 * (size_t)n_person * sizeof(float), hipMemcpyHostToDevice, s));
    PP_HIP_CHECK(hipMemcpyAsync(dneed, need, pk * sizeof(int32_t), hipMemcpyHostToDevice, s));
    PP_HIP_CHECK(hipMemsetAsync(part, 0, pk * n_split * sizeof(unsigned long long), s));
    const BuArgs a = bu_args(s0, n_frames, k, h0, w0, hr, wr, align_corners);
    hipLaunchKernelGGL(bu_refine_scan_kernel, dim3(n_split, k, n_person), dim3(BU_THREADS), 0, s, a, hm, dperm, dframe, dmean, dneed,
                       part);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bu_refine_merge_kernel, dim3((unsigned)((pk + BU_THREADS - 1) / BU_THREADS)), dim3(BU_THREADS), 0, s, a, hm,
                       dframe, dneed, part, n_split, n_person, dout);
    PP_HIP_CHECK(hipGetLastError());
    PP_HIP_CHECK(hipMemcpyAsync(out, dout, pk * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));
    return PP_OK;
}
