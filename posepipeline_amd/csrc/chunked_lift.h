// The chunked-lifting driver shared by the temporal lifters (lifting.hip: VideoPose3D, gastnet.hip: GAST-Net).
//
// Every track (segment) of a call is cut into chunks of T output frames.  A work item is one (segment, chunk) pair and occupies
// `samples` neighbouring batch samples of the lifting program; items of different segments share a batch.  A call uploads the packed
// tracks and the work table once, queues (pack kernel, program, unpack kernel) per batch group, downloads once and synchronises
// once.  What differs per lifter -- the two kernels, the samples per item, the floats per row -- comes in as arguments; the argument
// checks stay with each entry point.
#pragma once
#include "pp_internal.h"

#include <algorithm>

// per work item: first row of its segment in the packed arrays, rows of the segment, first output frame of the chunk
struct LiftItem {
    int32_t base, len, t0;
};

// one item per (segment, chunk of T frames), segment after segment
inline std::vector<LiftItem> lift_work_table(const int32_t* seg_len, int n_seg, int T) {
    std::vector<LiftItem> items;
    int32_t base = 0;
    for (int i = 0; i < n_seg; ++i) {
        for (int32_t t0 = 0; t0 < seg_len[i]; t0 += T) items.push_back({base, seg_len[i], t0});
        base += seg_len[i];
    }
    return items;
}

// everything of one call up to, not including, the final synchronisation; `items` must outlive that synchronisation
//   pack(stream, src, items of the group, b, program input)       launches the kernel that writes the b * samples input samples
//   unpack(stream, program output, items of the group, b, dst)    launches the kernel that writes the items' frames into the result
// both return PP_OK or the status of a refusal of their own; src / dst: the packed tracks / result on the device
template <class Pack, class Unpack>
int chunked_lift_enqueue(pp_net* net, pp_ctx* ctx, int in_buf, int out_buf, const float* src, const std::vector<LiftItem>& items,
                         size_t rows, int samples, int in_row, int out_row, float* out, int mem, Pack& pack, Unpack& unpack) {
    hipStream_t s = ctx->stream;
    const int per_group = pp_net_max_batch(net) / samples;          // items per batch group
    const bool host = mem == PP_MEM_HOST;
    const size_t in_e = rows * in_row, out_e = rows * out_row;
    int rc = ctx->ensure_scratch(ScratchCursor::align(items.size() * sizeof(LiftItem)) +
                                 (host ? ScratchCursor::align(in_e * sizeof(float)) + ScratchCursor::align(out_e * sizeof(float)) : 0));
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    LiftItem* d_items = cur.take<LiftItem>(items.size());
    const float* d_src = src;
    float* d_dst = out;
    if (host) {
        float* staged = cur.take<float>(in_e);
        d_dst = cur.take<float>(out_e);
        PP_HIP_CHECK(hipMemcpyAsync(staged, src, in_e * sizeof(float), hipMemcpyHostToDevice, s));
        d_src = staged;
    }
    PP_HIP_CHECK(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(LiftItem), hipMemcpyHostToDevice, s));
    void *in_ptr = nullptr, *out_ptr = nullptr;
    rc = pp_net_buffer(net, in_buf, &in_ptr, nullptr);
    if (rc == PP_OK) rc = pp_net_buffer(net, out_buf, &out_ptr, nullptr);
    if (rc != PP_OK) return rc;
    const int n_items = (int)items.size();
    for (int c0 = 0; c0 < n_items; c0 += per_group) {
        const int b = std::min(per_group, n_items - c0);
        rc = pack(s, d_src, d_items + c0, b, in_ptr);
        if (rc != PP_OK) return rc;
        PP_HIP_CHECK(hipGetLastError());
        pp_net_void_input_amax(net, in_buf);      // the input was just overwritten here, not by pp_net_forward: the net takes its maxima
        rc = pp_net_run(net, b * samples, 0, -1);
        if (rc != PP_OK) return rc;
        rc = unpack(s, static_cast<const float*>(out_ptr), d_items + c0, b, d_dst);
        if (rc != PP_OK) return rc;
        PP_HIP_CHECK(hipGetLastError());
    }
    if (host) PP_HIP_CHECK(hipMemcpyAsync(out, d_dst, out_e * sizeof(float), hipMemcpyDeviceToHost, s));
    return PP_OK;
}

// One call: the tracks `src` ([rows][in_row] floats, segment after segment, `mem` says where they and `out` live) through the net in
// chunks of T frames into `out` ([rows][out_row] floats).  The caller has checked its arguments and the program's shape.
template <class Pack, class Unpack>
int chunked_lift(pp_net* net, int in_buf, int out_buf, const float* src, const int32_t* seg_len, int n_seg, size_t rows, int T,
                 int samples, int in_row, int out_row, float* out, int mem, Pack pack, Unpack unpack) {
    const std::vector<LiftItem> items = lift_work_table(seg_len, n_seg, T);
    pp_ctx* ctx = pp_net_ctx(net);
    const int rc = chunked_lift_enqueue(net, ctx, in_buf, out_buf, src, items, rows, samples, in_row, out_row, out, mem, pack, unpack);
    return pp_sync_after(ctx->stream, rc);        // `items` and the caller's host arrays are read by queued copies
}
