// pp_videopose3d_lift_many / pp_videopose3d_lift: 2D -> 3D temporal lifting of keypoint tracks in the whole-clip dilated form.
//
// Replaces the per-window loop of pose_pipeline/wrappers/videopose3d.py:66-85: ChunkedGenerator builds
// one edge-replicated 243-frame window per output frame and TemporalModelOptimized1f (strided convs)
// reduces each to one frame -- 10.4x redundant.  Here every track (segment) is cut into chunks of T output
// frames; each chunk reads its frames plus a `pad`-frame halo (clamped to the SEGMENT = edge replication) and
// the dilated program (posepipeline_amd/models/videopose3d.py, dilations 1,3,9,27,81) produces all T
// frames at once.  Same weights, same taps per output in the same (tap, channel) order, hence
// bit-identical to the strided form (oracle/nets.py VideoPose3DRef).
//
// A work item is one (segment, chunk) pair and occupies one batch sample; items of different segments share a
// batch.  The windows are assembled on the device: lift_gather_kernel writes the program's input buffer from the
// packed tracks, lift_scatter_kernel copies the valid rows of the output buffer into the packed result.  This file
// holds the two kernels and the entry points' argument checks; the work table, the staging, the (gather, program,
// scatter) loop over the batch groups, the download and the one synchronisation per call are chunked_lift.h's
// driver, which GAST-Net shares.  pp_videopose3d_lift is the one-segment, host-memory case of the same code.
#include "chunked_lift.h"

#include <climits>

namespace {

// in[ci][j][c] = c < in_features ? src[base + clamp(t0 - pad + j, 0, len - 1)][c] : 0, for the items of one batch group.
// V = float2 when both channel counts are even (34 -> 36 floats = 17 -> 18 float2), else float; the counts are in units of V.
template <class V>
__global__ void lift_gather_kernel(const V* __restrict__ src, const LiftItem* __restrict__ items, int total, int iw, int ic,
                                   int in_features, int pad, V* __restrict__ in) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = idx % ic;
    const int j = (idx / ic) % iw;
    const LiftItem it = items[idx / (ic * iw)];
    V v{};
    if (c < in_features) {
        int row = it.t0 - pad + j;                          // np.pad(..., 'edge') == clamp, inside the segment
        row = row < 0 ? 0 : (row >= it.len ? it.len - 1 : row);
        v = src[((size_t)it.base + row) * in_features + c];
    }
    in[idx] = v;
}

// dst[base + t0 + r][c] = out[ci][r][c] for r < min(T, len - t0): per item one contiguous run of floats
__global__ void lift_scatter_kernel(const float* __restrict__ out, const LiftItem* __restrict__ items, int total, int T, int oc,
                                    float* __restrict__ dst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int e = idx % (T * oc);
    const LiftItem it = items[idx / (T * oc)];
    const int cnt = min(T, it.len - it.t0);
    if (e < cnt * oc) dst[((size_t)it.base + it.t0) * oc + e] = out[idx];
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// `who`: the entry point the caller used, for the messages
int lift_many(const char* who, pp_net* net, int in_buf, int out_buf, const float* kpts2d_norm, const int32_t* seg_frames, int n_segs,
              int in_features, int out_features, int pad, float* out, int mem) {
    PP_REQUIRE(net && kpts2d_norm && seg_frames && out, "%s: NULL argument", who);
    PP_REQUIRE(n_segs >= 0 && in_features > 0 && out_features > 0 && pad >= 0, "%s: bad dims", who);
    PP_REQUIRE(mem == PP_MEM_HOST || mem == PP_MEM_DEVICE, "%s: mem %d is neither PP_MEM_HOST nor PP_MEM_DEVICE", who, mem);
    size_t rows = 0;
    for (int i = 0; i < n_segs; ++i) {
        PP_REQUIRE(seg_frames[i] >= 0, "%s: bad dims (segment %d has %d frames)", who, i, seg_frames[i]);
        rows += (size_t)seg_frames[i];
    }
    PP_REQUIRE(rows <= (size_t)INT_MAX, "%s: %zu frames in one call (the work table holds int32 rows)", who, rows);
    if (rows == 0) return PP_OK;
    int ih, iw, ic, oh, ow, oc;
    PP_REQUIRE(pp_net_dims(net, in_buf, &ih, &iw, &ic) == PP_OK && pp_net_dims(net, out_buf, &oh, &ow, &oc) == PP_OK,
               "%s: bad buffer id", who);
    PP_REQUIRE(ih == 1 && oh == 1 && ic >= in_features && oc == out_features && iw == ow + 2 * pad,
               "%s: program shape (in %dx%dx%d, out %dx%dx%d) does not match pad=%d / features %d->%d",
               who, ih, iw, ic, oh, ow, oc, pad, in_features, out_features);
    const int T = ow;
    auto gather = [=](hipStream_t s, const float* src, const LiftItem* items, int b, void* in) -> int {
        if (in_features % 2 == 0 && ic % 2 == 0 && aligned8(src) && aligned8(in)) {
            const int total = b * iw * (ic / 2);
            hipLaunchKernelGGL(lift_gather_kernel<float2>, dim3((total + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float2*>(src),
                               items, total, iw, ic / 2, in_features / 2, pad, static_cast<float2*>(in));
        } else {
            const int total = b * iw * ic;
            hipLaunchKernelGGL(lift_gather_kernel<float>, dim3((total + 255) / 256), dim3(256), 0, s, src, items, total, iw, ic,
                               in_features, pad, static_cast<float*>(in));
        }
        return PP_OK;
    };
    auto scatter = [=](hipStream_t s, const float* net_out, const LiftItem* items, int b, float* dst) -> int {
        const int total = b * T * oc;
        hipLaunchKernelGGL(lift_scatter_kernel, dim3((total + 255) / 256), dim3(256), 0, s, net_out, items, total, T, oc, dst);
        return PP_OK;
    };
    PpRange range("pp_videopose3d_lift_many");
    return chunked_lift(net, in_buf, out_buf, kpts2d_norm, seg_frames, n_segs, rows, T, 1, in_features, oc, out, mem, gather, scatter);
}

}  // namespace

extern "C" int pp_videopose3d_lift_many(pp_net* net, int in_buf, int out_buf, const float* kpts2d_norm, const int32_t* seg_frames,
                                        int n_segs, int in_features, int out_features, int pad, float* out, int mem) {
    return lift_many("pp_videopose3d_lift_many", net, in_buf, out_buf, kpts2d_norm, seg_frames, n_segs, in_features, out_features, pad,
                     out, mem);
}

extern "C" int pp_videopose3d_lift(pp_net* net, int in_buf, int out_buf, const float* kpts2d_norm, int n_frames,
                                   int in_features, int out_features, int pad, float* out) {
    const int32_t seg = n_frames;
    return lift_many("pp_videopose3d_lift", net, in_buf, out_buf, kpts2d_norm, &seg, 1, in_features, out_features, pad, out, PP_MEM_HOST);
}
