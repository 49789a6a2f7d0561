// Context, memory and upload helpers and the single-conv entry point (layer programs, pp_net_*: net.hip).
#include <dlfcn.h>

#include <algorithm>
#include <memory>

#include "pp_internal.h"

#include <atomic>
extern std::atomic<int> g_decode_generic, g_split_gemm_epi, g_split_gemm_tile;      // dark_decode.hip, conv_split_gemm.hip (two)

static thread_local std::string g_last_error;

void pp_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char* lib : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            void* h = dlopen(lib, RTLD_LAZY | RTLD_LOCAL);
            if (!h) continue;
            push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
const Roctx& roctx() {
    static const Roctx r;
    return r;
}
}  // namespace

void pp_range_push(const char* name) {
    if (roctx().push) (void)roctx().push(name);
}
void pp_range_pop() {
    if (roctx().pop) (void)roctx().pop();
}

int pp_ctx::ensure_scratch(size_t bytes) {
    if (bytes <= scratch_bytes) return PP_OK;
    if (scratch) {
        PP_HIP_CHECK(hipStreamSynchronize(stream));
        PP_HIP_CHECK(hipFree(scratch));
        scratch = nullptr;
        scratch_bytes = 0;
    }
    size_t want = std::max(bytes, size_t(1) << 20);
    PP_HIP_CHECK(hipMalloc(&scratch, want));
    scratch_bytes = want;
    return PP_OK;
}

extern "C" {

int pp_abi_version(void) { return PP_ABI_VERSION; }

int pp_debug_knob(const char* name, int value) {
    PP_REQUIRE(name && value >= -1 && value <= 1, "pp_debug_knob: name and a value in {-1, 0, 1}");
    if (!strcmp(name, "decode_generic")) g_decode_generic.store(value, std::memory_order_relaxed);
    else if (!strcmp(name, "split_gemm_epilogue")) g_split_gemm_epi.store(value, std::memory_order_relaxed);
    else if (!strcmp(name, "split_gemm_wave_tile")) g_split_gemm_tile.store(value, std::memory_order_relaxed);
    else {
        pp_set_error("pp_debug_knob: unknown knob '%s' (decode_generic, split_gemm_epilogue, split_gemm_wave_tile)", name);
        return PP_ERR_ARG;
    }
    return PP_OK;
}

const char* pp_last_error(void) { return g_last_error.c_str(); }

int pp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int pp_ctx_create(int device, pp_ctx** out) {
    PP_REQUIRE(out != nullptr, "pp_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        pp_set_error("pp_ctx_create: no HIP device visible (%s) -- this library has no CPU fallback",
                     e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return PP_ERR_HIP;
    }
    PP_REQUIRE(device >= 0 && device < n, "pp_ctx_create: device %d out of range [0,%d)", device, n);
    PP_HIP_CHECK(hipSetDevice(device));
    std::unique_ptr<pp_ctx> c(new pp_ctx());
    c->device = device;
    PP_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    PP_HIP_CHECK(hipEventCreate(&c->ev_start));
    PP_HIP_CHECK(hipEventCreate(&c->ev_stop));
    PP_HIP_CHECK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    PP_HIP_CHECK(hipEventCreateWithFlags(&c->ev_upload, hipEventDisableTiming));
    PP_HIP_CHECK(hipEventCreateWithFlags(&c->ev_consumed, hipEventDisableTiming));
    *out = c.release();
    return PP_OK;
}

void pp_ctx_destroy(pp_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
    if (ctx->ev_stop) (void)hipEventDestroy(ctx->ev_stop);
    if (ctx->copy_stream) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamDestroy(ctx->copy_stream);
    }
    if (ctx->ev_upload) (void)hipEventDestroy(ctx->ev_upload);
    if (ctx->ev_consumed) (void)hipEventDestroy(ctx->ev_consumed);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int pp_ctx_set_stream(pp_ctx* ctx, void* hip_stream) {
    PP_REQUIRE(ctx, "pp_ctx_set_stream: ctx is NULL");
    PP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) PP_HIP_CHECK(hipStreamDestroy(ctx->stream));
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    ctx->own_stream = false;
    return PP_OK;
}

int pp_ctx_synchronize(pp_ctx* ctx) {
    PP_REQUIRE(ctx, "pp_ctx_synchronize: ctx is NULL");
    PP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PP_OK;
}

int pp_timer_start(pp_ctx* ctx) {
    PP_REQUIRE(ctx, "pp_timer_start: ctx is NULL");
    PP_HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
    return PP_OK;
}

int pp_timer_stop(pp_ctx* ctx, float* elapsed_ms) {
    PP_REQUIRE(ctx && elapsed_ms, "pp_timer_stop: NULL argument");
    PP_HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
    PP_HIP_CHECK(hipEventSynchronize(ctx->ev_stop));
    PP_HIP_CHECK(hipEventElapsedTime(elapsed_ms, ctx->ev_start, ctx->ev_stop));
    return PP_OK;
}

int pp_malloc(pp_ctx* ctx, size_t bytes, void** dptr) {
    PP_REQUIRE(ctx && dptr, "pp_malloc: NULL argument");
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    PP_HIP_CHECK(hipMalloc(dptr, bytes ? bytes : 1));
    return PP_OK;
}

int pp_free(pp_ctx* ctx, void* dptr) {
    PP_REQUIRE(ctx, "pp_free: ctx is NULL");
    if (!dptr) return PP_OK;
    PP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    PP_HIP_CHECK(hipFree(dptr));
    return PP_OK;
}

int pp_memcpy_h2d(pp_ctx* ctx, void* dst, const void* src, size_t bytes) {
    PP_REQUIRE(ctx && (bytes == 0 || (dst && src)), "pp_memcpy_h2d: NULL argument");
    PP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    PP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PP_OK;
}

int pp_host_alloc(pp_ctx* ctx, size_t bytes, void** out) {
    PP_REQUIRE(ctx && out, "pp_host_alloc: NULL argument");
    *out = nullptr;
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    PP_HIP_CHECK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return PP_OK;
}

int pp_host_free(pp_ctx* ctx, void* p) {
    PP_REQUIRE(ctx != nullptr, "pp_host_free: ctx is NULL");
    if (p) PP_HIP_CHECK(hipHostFree(p));
    return PP_OK;
}

int pp_upload_begin(pp_ctx* ctx, void* dst, const void* src, size_t bytes) {
    PP_REQUIRE(ctx && (bytes == 0 || (dst && src)), "pp_upload_begin: NULL argument");
    // the destination may still be read by compute work enqueued before the last pp_upload_release
    PP_HIP_CHECK(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_consumed, 0));
    PP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
    PP_HIP_CHECK(hipEventRecord(ctx->ev_upload, ctx->copy_stream));
    return PP_OK;
}

int pp_upload_begin_nv12(pp_ctx* ctx, void* dst_bgr, void* tmp_nv12, const void* src_host, int frames, int height, int width) {
    PP_REQUIRE(ctx && (frames == 0 || (dst_bgr && tmp_nv12 && src_host)), "pp_upload_begin_nv12: NULL argument");
    PP_REQUIRE(frames >= 0 && height > 0 && width > 0, "pp_upload_begin_nv12: bad shape");
    PP_HIP_CHECK(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_consumed, 0));
    const size_t bytes = (size_t)frames * height * width * 3 / 2;
    if (bytes) PP_HIP_CHECK(hipMemcpyAsync(tmp_nv12, src_host, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
    // the conversion rides the copy stream: `ev_upload` then covers the BGR frames, and the (in-order) copy stream does not
    // overwrite tmp_nv12 with the next chunk before this kernel has read it
    const int r = pp_launch_nv12_to_bgr((const unsigned char*)tmp_nv12, (unsigned char*)dst_bgr, frames, height, width, ctx->copy_stream);
    if (r != PP_OK) return r;
    PP_HIP_CHECK(hipEventRecord(ctx->ev_upload, ctx->copy_stream));
    return PP_OK;
}

int pp_nv12_to_bgr(pp_ctx* ctx, const uint8_t* nv12, int frames, int height, int width, uint8_t* bgr) {
    PP_REQUIRE(ctx && (frames == 0 || (nv12 && bgr)), "pp_nv12_to_bgr: NULL argument");
    return pp_launch_nv12_to_bgr(nv12, bgr, frames, height, width, ctx->stream);
}

int pp_upload_wait(pp_ctx* ctx, int host_sync) {
    PP_REQUIRE(ctx != nullptr, "pp_upload_wait: ctx is NULL");
    PP_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_upload, 0));
    if (host_sync) PP_HIP_CHECK(hipEventSynchronize(ctx->ev_upload));
    return PP_OK;
}

int pp_upload_release(pp_ctx* ctx) {
    PP_REQUIRE(ctx != nullptr, "pp_upload_release: ctx is NULL");
    PP_HIP_CHECK(hipEventRecord(ctx->ev_consumed, ctx->stream));
    return PP_OK;
}

int pp_memcpy_d2h(pp_ctx* ctx, void* dst, const void* src, size_t bytes) {
    PP_REQUIRE(ctx && (bytes == 0 || (dst && src)), "pp_memcpy_d2h: NULL argument");
    PP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PP_OK;
}

int pp_memcpy_d2d(pp_ctx* ctx, void* dst, const void* src, size_t bytes) {
    PP_REQUIRE(ctx && (bytes == 0 || (dst && src)), "pp_memcpy_d2d: NULL argument");
    PP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return PP_OK;
}

int pp_conv2d(pp_ctx* ctx, const pp_op* op, int n, int hin, int win, const float* x, const float* w,
              const float* bias, const float* res1, const float* res2, float* y, int res1_h, int res1_w,
              int mem) {
    PP_REQUIRE(ctx && op && x && w && bias && y, "pp_conv2d: NULL argument");
    PP_REQUIRE(op->type == PP_OP_CONV, "pp_conv2d: op is not a conv");
    PP_REQUIRE(n > 0 && hin > 0 && win > 0, "pp_conv2d: empty input");
    ConvArgs a{};
    a.N = n; a.Hin = hin; a.Win = win; a.Cin = op->cin;
    a.Hout = pp_conv_out_dim(hin + (op->pad_end & 1), op->kh, op->stride, op->pad_h, op->dil_h) - ((op->pad_end >> 2) & 1);
    a.Wout = pp_conv_out_dim(win + ((op->pad_end >> 1) & 1), op->kw, op->stride, op->pad_w, op->dil_w) - ((op->pad_end >> 3) & 1);
    PP_REQUIRE(a.Hout > 0 && a.Wout > 0, "pp_conv2d: empty output");
    a.Cout = op->cout; a.CoutPad = (op->cout + 15) / 16 * 16;
    a.KH = op->kh; a.KW = op->kw; a.stride = op->stride; a.pad_h = op->pad_h; a.pad_w = op->pad_w;
    a.dil_h = op->dil_h; a.dil_w = op->dil_w;
    a.K = op->kh * op->kw * op->cin; a.Kpad = (a.K + 31) / 32 * 32;
    a.HWout = a.Hout * a.Wout; a.M = n * a.HWout;
    a.relu = op->relu; a.up_log2 = op->up_log2; a.out_nchw = op->out_nchw;
    a.res1_shift = op->res1_shift; a.res1_off_w = op->res1_off_w;
    const int Ho2 = a.Hout << op->up_log2, Wo2 = a.Wout << op->up_log2;
    a.res1_H = res1 ? (res1_h > 0 ? res1_h : Ho2) : 0;
    a.res1_W = res1 ? (res1_w > 0 ? res1_w : Wo2) : 0;
    a.y_stride = op->cout; a.y_coff = 0;
    PP_REQUIRE(op->out_c_off == 0 && op->in_c_off == 0, "pp_conv2d: channel slices need a layer program");
    const size_t x_e = (size_t)n * hin * win * op->cin;
    const size_t w_e = (size_t)a.Kpad * a.CoutPad;
    const size_t b_e = a.CoutPad;
    const size_t y_e = (size_t)n * Ho2 * Wo2 * op->cout;
    const size_t r1_e = res1 ? (size_t)n * a.res1_H * a.res1_W * op->cout : 0;
    const size_t r2_e = res2 ? y_e : 0;
    if (mem == PP_MEM_DEVICE) {
        a.x = x; a.w = w; a.bias = bias; a.res1 = res1; a.res2 = res2; a.y = y;
        return pp_launch_conv(a, nullptr, ctx->stream);
    }
    size_t total = 0;
    for (size_t e : {x_e, w_e, b_e, y_e, r1_e, r2_e}) total += ScratchCursor::align(e * sizeof(float));
    int rc = ctx->ensure_scratch(total);
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    float* dx = cur.take<float>(x_e);
    float* dw = cur.take<float>(w_e);
    float* db = cur.take<float>(b_e);
    float* dy = cur.take<float>(y_e);
    float* dr1 = cur.take<float>(r1_e);
    float* dr2 = cur.take<float>(r2_e);
    hipStream_t s = ctx->stream;
    PP_HIP_CHECK(hipMemcpyAsync(dx, x, x_e * 4, hipMemcpyHostToDevice, s));
    PP_HIP_CHECK(hipMemcpyAsync(dw, w, w_e * 4, hipMemcpyHostToDevice, s));
    PP_HIP_CHECK(hipMemcpyAsync(db, bias, b_e * 4, hipMemcpyHostToDevice, s));
    if (res1) PP_HIP_CHECK(hipMemcpyAsync(dr1, res1, r1_e * 4, hipMemcpyHostToDevice, s));
    if (res2) PP_HIP_CHECK(hipMemcpyAsync(dr2, res2, r2_e * 4, hipMemcpyHostToDevice, s));
    a.x = dx; a.w = dw; a.bias = db; a.res1 = res1 ? dr1 : nullptr; a.res2 = res2 ? dr2 : nullptr; a.y = dy;
    rc = pp_launch_conv(a, nullptr, s);
    if (rc != PP_OK) return rc;
    PP_HIP_CHECK(hipMemcpyAsync(y, dy, y_e * 4, hipMemcpyDeviceToHost, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));
    return PP_OK;
}

}  // extern "C"
