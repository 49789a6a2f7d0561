/*
 * posepipe_hip.h -- C ABI of libposepipe_hip.so: the MI355X (gfx950) hot path of
 * PosePipe's detect/track -> top-down 2D -> 3D lifting cascade.
 *
 * The reference (peabody124/PosePipeline) has no FFI for this path: its boundary is the
 * Python calling convention between DataJoint `make()` methods and the wrapper functions
 *   pose_pipeline/wrappers/mmtrack.py:8      mmtrack_bounding_boxes(file_path, method)
 *   pose_pipeline/wrappers/mmpose.py:26      mmpose_top_down_person(key, method)
 *   pose_pipeline/wrappers/videopose3d.py:19 process_videopose3d(key, batch_size, transform_coco)
 * whose arithmetic lives in un-vendored third-party packages (mmpose / mmdet / mmtrack /
 * VideoPose3D / OpenCV).  Each entry point below names the reference line(s) or third-party
 * op it replaces.  posepipeline_amd/wrappers/ holds the drop-in Python callables that bind
 * these symbols through ctypes (see INTEGRATION.md for the stub a maintainer would add).
 *
 * Conventions
 *   - every function returns 0 on success, a negative pp_status on failure; the message is
 *     available from pp_last_error() (thread-local).
 *   - all array arguments are caller-owned, contiguous, with explicit dims.  `mem` says whether
 *     the pointers are host (PP_MEM_HOST: the library stages them through its own device
 *     buffers) or device (PP_MEM_DEVICE: used in place, e.g. a torch tensor's data_ptr()).
 *   - one HIP stream per ctx; calls on one ctx are not thread-safe, distinct ctxs are.
 *   - no torch / C++ types cross this boundary.
 */
#ifndef POSEPIPE_HIP_H
#define POSEPIPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_ABI_VERSION 10  /* 2: pp_op gained out_c_off / in_c_off / pad_end; PP_ACT_* activations
                              3: PP_OP_VIT_ENCODER / PP_OP_DEPTH_TO_SPACE, bf16 building blocks, UDP top-down (post 2)
                              4: pp_memcpy_d2d, pp_net_create_mem (weights already on the device, e.g. an RCCL broadcast)
                              5: pp_buf.pad (zero halo of conv-only buffers), PP_OP_AVGPOOL, pp_crop_resize_bilinear,
                                 pp_conv_force / pp_conv_variant
                              6: pp_conv_exact, pp_net_conv_kinds; pp_conv_variant accepts 4 (fp32 convolutions on the bf16 matrix cores by a
                                 three-way operand split are the default where a layer is eligible)
                              7: pp_net_create_ex / pp_net_numerics: the numerics of a program are fixed when it is created (a per-net
                                 property, no longer read from the process-wide switch at launch time); pp_op gained in2 / in3 /
                                 up2_log2 / up3_log2 (sizeof(pp_op) 104 -> 120)
                              8: pp_upload_begin_nv12 / pp_nv12_to_bgr (NV12 frame source)
                              9: PP_NET_NUMERICS_SPLIT_BF16 / _F16, pp_conv_split_kind, pp_net_split_kind: the split convolutions have a
                                 second form -- two float16 terms per operand, three products (conv_split.hip, round 5);
                                 pp_detector_constants
                              10: pp_detector_enable_margins / pp_detector_margins (per-frame decision margins of the detection path);
                                 pp_net_input_amax is a one-shot promise; PP_OP_BILINEAR_ADD (an added op type over existing pp_op
                                 fields: no struct or signature changed, so the version stays 10);
                                 PP_OP_DWCONV3X3 / PP_OP_LAYERNORM / PP_OP_WINDOW_ATTN / PP_OP_GELU_ADD and PP_ACT_GELU (the HRFormer
                                 blocks) were added the same way, and so were PP_OP_ATTENTION and the pp_poseformer_* / pp_attention_f32
                                 entry points (added functions only) */

typedef enum {
    PP_OK = 0,
    PP_ERR_ARG = -1,      /* bad argument */
    PP_ERR_HIP = -2,      /* HIP runtime error (no GPU, launch failure, OOM ...) */
    PP_ERR_STATE = -3,    /* object used in the wrong state */
    PP_ERR_UNSUPPORTED = -4
} pp_status;

typedef enum { PP_MEM_HOST = 0, PP_MEM_DEVICE = 1 } pp_mem_kind;

typedef struct pp_ctx pp_ctx;   /* device + stream + scratch */
typedef struct pp_net pp_net;   /* a compiled layer program + resident weights/activations */
typedef struct pp_tracker pp_tracker; /* host-side multi-object tracker state */
typedef struct pp_topdown pp_topdown; /* fused top-down 2D stage (crop -> backbone -> decode) */

/* ---- library / context ------------------------------------------------------------------ */
int pp_abi_version(void);
const char* pp_last_error(void);
int pp_device_count(void);                         /* 0 when no HIP device is visible */
int pp_ctx_create(int device, pp_ctx** out);       /* fails with PP_ERR_HIP when there is no GPU */
void pp_ctx_destroy(pp_ctx* ctx);
int pp_ctx_set_stream(pp_ctx* ctx, void* hip_stream); /* adopt an external hipStream_t (e.g. torch's) */
int pp_ctx_synchronize(pp_ctx* ctx);
/* HIP-event timer on the ctx stream (bench.py's roofline leg): start/stop bracket launches. */
int pp_timer_start(pp_ctx* ctx);
int pp_timer_stop(pp_ctx* ctx, float* elapsed_ms); /* synchronises on the stop event */
/* A/B knobs of tests and profiles that select between two kernels giving IDENTICAL bits (never numerics): "decode_generic"
 * (1: the generic flip-merge / decode kernel instead of the fast one), "split_gemm_epilogue" (1: the product kernel's epilogue
 * transposed through LDS, 0: from registers), "split_gemm_wave_tile" (1: the fp16-form product kernel's four waves 4 x 1 with wave
 * tiles of 64 pixels x 128 channels, 0: 2 x 2 with 128 x 64).  value -1: back to the environment's choice (POSEPIPE_DECODE_GENERIC /
 * POSEPIPE_SPLIT_GEMM_EPI / POSEPIPE_SPLIT_GEMM_TILE, read once per process).  Process-wide, thread-safe. */
int pp_debug_knob(const char* name, int value);
/* raw device memory helpers so that a host language without a HIP binding can keep data resident */
int pp_malloc(pp_ctx* ctx, size_t bytes, void** dptr);
int pp_free(pp_ctx* ctx, void* dptr);
int pp_memcpy_h2d(pp_ctx* ctx, void* dst, const void* src, size_t bytes);
int pp_memcpy_d2h(pp_ctx* ctx, void* dst, const void* src, size_t bytes);
/* device -> device on the ctx stream, asynchronous (ordered with the other work of the ctx) */
int pp_memcpy_d2d(pp_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Frame upload path (replaces the per-frame cv2.VideoCapture.read() -> model H2D of wrappers/mmtrack.py:38-45 and
 * wrappers/mmpose.py:60-75 with a chunked, double-buffered transfer): page-locked host staging buffers and an
 * asynchronous host->device copy on the context's copy stream, so chunk k+1 is uploaded while chunk k computes.
 *   pp_upload_begin   enqueue the copy (waits, on the device, for the last pp_upload_release);
 *   pp_upload_wait    make the compute stream wait for the last upload (host_sync != 0: also block the host);
 *   pp_upload_release mark, in compute-stream order, that the device buffer may be overwritten again. */
int pp_host_alloc(pp_ctx* ctx, size_t bytes, void** host_ptr);
int pp_host_free(pp_ctx* ctx, void* host_ptr);
int pp_upload_begin(pp_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);
/* ABI 8 -- NV12 frame source (a decoder's native output: Y plane [h][w], then interleaved UV [h/2][w]; half the bytes of
 * the BGR frames cv2.VideoCapture.read() hands the reference at pose_pipeline/pipeline.py:47-87, wrappers/mmtrack.py:38-45,
 * wrappers/mmpose.py:55-75).  h and w even.  The conversion is OpenCV's cvtColor(COLOR_YUV2BGR_NV12) bit for
 * bit (ITU-R BT.601 limited range, 20-bit fixed point; oracle/nv12.py).
 *   pp_upload_begin_nv12  pp_upload_begin for `frames` NV12 frames: host -> tmp_nv12_device on the copy stream, then the
 *                         conversion into dst_bgr_device ([frames][h][w][3] u8) on the same stream; pp_upload_wait /
 *                         pp_upload_release as for pp_upload_begin.  tmp_nv12_device: frames * h * w * 3 / 2 bytes, may be
 *                         the same buffer for every call (the copy stream is in order).
 *   pp_nv12_to_bgr        the conversion alone, device -> device on the ctx stream. */
int pp_upload_begin_nv12(pp_ctx* ctx, void* dst_bgr_device, void* tmp_nv12_device, const void* src_nv12_host, int frames,
                         int height, int width);
int pp_nv12_to_bgr(pp_ctx* ctx, const uint8_t* nv12_device, int frames, int height, int width, uint8_t* bgr_device);
int pp_upload_wait(pp_ctx* ctx, int host_sync);
int pp_upload_release(pp_ctx* ctx);

/* ---- layer programs (backbones) ----------------------------------------------------------
 * A network is a straight-line program of ops over numbered NHWC fp32 activation buffers.
 * Replaces the third-party forward passes reached from
 *   wrappers/mmpose.py:75  (mmpose TopDown.forward_test -> HRNet, arch spec
 *                           3rdparty/mmpose/config/top_down/darkpose/coco/hrnet_w48_coco_384x288_dark.py:44-79)
 *   wrappers/mmtrack.py:45 (mmdet FasterRCNN, 3rdparty/mmtracking/_base_/models/faster_rcnn_r50_fpn.py:1-112)
 *   wrappers/videopose3d.py:82 (VideoPose3D TemporalModel, wrappers/videopose3d.py:46-50)
 * Convolutions run as implicit GEMM on v_mfma_f32_16x16x4_f32 with BatchNorm folded into
 * (weight, bias) and bias / residual adds / ReLU / nearest-upsample-accumulate fused in the
 * epilogue.  The fp32 MFMA accumulates each output as a k-ordered fmaf chain over
 * k = (kh, kw, cin), which is exactly what oracle/conv_ref.c does, so results are bit-exact.
 */
typedef enum {
    PP_OP_CONV = 1,      /* conv2d (conv1d when H == 1), see pp_op fields */
    PP_OP_MAXPOOL = 2,   /* kh x kw max pool, -inf padding (ResNet stem 3x3 s2 p1; FPN P6 1x1 s2) */
    PP_OP_ROIALIGN = 3,  /* reserved for the detector program */
    PP_OP_COPY = 4,      /* buffer copy (same dims) */
    PP_OP_VIT_ENCODER = 5,   /* ViT encoder on the bf16 matrix cores, see "ViT encoder" below */
    PP_OP_DEPTH_TO_SPACE = 6,/* in [h][w][4*cout] (channel groups g = 2*dy + dx) -> out [2h][2w][cout]; with four 2x2
                                convolutions writing the groups this is ConvTranspose2d(k=4, s=2, p=1) */
    PP_OP_DECONV_BF16 = 8,   /* ConvTranspose2d(4, 2, 1) + bias + act on the bf16 matrix cores: in [h][w][cin] fp32 ->
                                out [2h][2w][cout] fp32; w_off: fp32 W_all[16][cout][cin], block ((a*2+b)*2+r)*2+s =
                                w[:, :, 3-a-2r, 3-b-2s]^T (output parity (a, b), tap (r, s)); b_off: bias[cout];
                                cin % 64 == 0, cout % 8 == 0; relu PP_RELU_NONE / PP_RELU_LAST.  One GEMM with N = 16 cout
                                and a 4-term gather; operands rounded to bf16, fp32 accumulation (tolerance-based parity) */
    PP_OP_AVGPOOL = 9,       /* nn.AvgPool2d((kh, kw), stride), no padding: float32 sum in (kh, kw) order / (kh * kw)  (the
                                GlobalAveragePooling neck of mmtrack's ReID model, mot/deepsort/deepsort_*.py:27) */
    PP_OP_UPSAMPLE_ADD = 7,  /* out[y][x] = act(((((res1[y][x] + in[y >> up_log2][x >> up_log2]) + in2[y >> up2_log2][x >> up2_log2])
                                + in3[y >> up3_log2][x >> up3_log2]) + res2[y][x]): nearest upsample + accumulate of an HRNet
                                fuse layer in mmpose's summation order (res1, in2, in3, res2 optional; relu: PP_RELU_NONE /
                                PP_RELU_LAST); same additions, same order as a chain of convs with up_log2, in one pass */
    PP_OP_BILINEAR_ADD = 10, /* out[y][x][out_c_off + c] = act(((res1[y][x][c] + B(in)) + B(in2)) + B(in3)), B = bilinear upsampling by
                                2^up_log2 / 2^up2_log2 / 2^up3_log2 with half-pixel centres (F.interpolate(mode='bilinear',
                                align_corners=False)): sy = max((y + 0.5) / s - 0.5, 0), y0 = floor(sy), y1 = min(y0 + 1, h - 1), ly1 = sy -
                                y0, ly0 = 1 - ly1 (the same in x); B = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11), every
                                product and sum rounded to float32 (no FMA).  The fuse layers of HRNetv2 (res1, in2, in3 optional; relu:
                                PP_RELU_NONE / PP_RELU_LAST) and, with out_c_off, the resize + concatenate in front of its head: channels
                                [out_c_off, out_c_off + cout) of a wider NHWC `out`, the others untouched.  cin == cout, % 4 == 0.
                                Uses existing pp_op fields only: sizeof(pp_op) and PP_ABI_VERSION are unchanged */
    /* The ops of an HRFormer block (mmpose 0.x backbones/hrformer.py; models/hrformer.py), float32 on the vector ALU (hrformer.hip).
     * They use existing pp_op fields only -- sizeof(pp_op) and PP_ABI_VERSION are unchanged -- and every field not named below keeps
     * its neutral value (res1 / res2 / in2 / in3 = -1, offsets 0).  erf and exp are evaluated in double and rounded once. */
    PP_OP_DWCONV3X3 = 11,    /* depthwise 3x3 convolution, padding 1: in [h][w][c] -> out [(h - 1) / s + 1][(w - 1) / s + 1][c];
                                cin = cout = c (the buffers' channels, % 4 == 0), kh = kw = 3, stride = s in {1, 2}, pad_h = pad_w = 1;
                                w_off: w[9][c] (tap ky * 3 + kx major, BN folded), b_off: bias[c].
                                out = act(bias + sum over (ky, kx) in that order of g(in) * w): acc = bias, then acc = acc + x * w with the
                                product and the sum each rounded to float32 (no FMA); taps outside the map are skipped.
                                relu: the output's activation, PP_RELU_NONE / PP_RELU_LAST / PP_ACT_GELU;
                                pad_end bit 0 (PP_DW_GELU_IN): g = GELU applied to every input value read (stride 1 only; CrossFFN's
                                fc1 activation lives here, not in the convolution kernels), else g = identity */
    PP_OP_LAYERNORM = 12,    /* LayerNorm over the channels of every pixel: in, out [h][w][cout] (distinct buffers); cin = c_real <= cout =
                                the buffers' channels (% 4 == 0, <= 1024); w_off: gamma[cout], b_off: beta[cout] followed by eps (one
                                float).  mean and the biased variance run over the first c_real channels (two passes: sum, then sum of
                                squared deviations), out = (x - mean) / sqrt(var + eps) * gamma + beta; channels >= c_real are written as
                                exact zeros whatever `in` holds there */
    PP_OP_WINDOW_ATTN = 13,  /* 7x7 local-window multi-head self-attention with a relative-position bias (LocalWindowSelfAttention +
                                WindowMSA, with_rpe, no pad mask).  in [h][w][3 * cout] = the qkv map, a 1x1 PP_OP_CONV of the LayerNorm
                                output: channel s * cout + head * hd + d holds (q, k, v)[s] of head `head`, s = 0, 1, 2, hd = cin / heads;
                                channels [cin, cout) of each third are padding.  out [h][w][cout].  cin = c_real = heads * hd (hd <= 64),
                                cout = the out buffer's channels (% 4 == 0), kh = kw = 7, stride = heads;
                                w_off: table[169][heads] (relative_position_bias_table), b_off: the qkv bias in the layout of `in`
                                ([3 * cout]; the k and v thirds are read).
                                The map is zero-padded to multiples of 7 with pad / 2 rows (columns) in front and the rest behind, and cut
                                into 7x7 windows.  Per window and head, over its 49 tokens i, j = (y, x) row-major:
                                  attn[i][j] = (q_i * hd^-0.5) . k_j + table[(y_i - y_j + 6) * 13 + (x_i - x_j + 6)][head],
                                  out_i = sum_j softmax_j(attn[i][j]) v_j.
                                A padded token takes part as a key with k = b_k, v = b_v (mmpose pads BEFORE the qkv Linear, and
                                0 . W + b = b exactly); its own output is cropped away.  Channels [cin, cout) of `out` are exact zeros */
    PP_OP_GELU_ADD = 14,     /* out = res1 + gelu(in) (res1 = -1: out = gelu(in)); in, res1, out [h][w][c], cin = cout = c % 4 == 0, out
                                distinct from in and res1.  The last GELU of CrossFFN and the block's residual add in one pass */
    PP_OP_ATTENTION = 15     /* global multi-head self-attention in float32 (poseformer.hip; the temporal stage of PoseFormer), one sample =
                                one sequence of h * w <= 128 tokens.  in [h][w][3 * cout] = the qkv map, a 1x1 PP_OP_CONV of the LayerNorm
                                output: channel s * cout + head * hd + d holds (q, k, v)[s] of head `head`, s = 0, 1, 2, hd = cin / heads;
                                channels [cin, cout) of each third are padding and are not read.  out [h][w][cout].  cin = c_real = heads * hd
                                (hd % 4 == 0, hd <= 128), cout = the out buffer's channels (% 4 == 0), stride = heads (as PP_OP_WINDOW_ATTN);
                                no parameters.  Per sample and head, over the tokens i, j:
                                  out_i = sum_j softmax_j((q_i . k_j) * hd^-0.5) v_j,
                                each dot product one fmaf chain over d, the row maximum subtracted before exp, the sum over j one fmaf
                                chain in token order; no atomics.  Channels [cin, cout) of `out` are exact zeros.  Existing pp_op fields
                                only: sizeof(pp_op) and PP_ABI_VERSION are unchanged */
    /* PP_OP_DCN3X3 = 16 and PP_OP_DWDECONV = 17 (the DCN up-sampling head of DLA-34, fairmot.hip) are #defined at the end of this
     * header, with the FairMOT entry points: the header grows only at its end */
} pp_op_type;

#define PP_RELU_NONE 0
#define PP_RELU_LAST 1   /* y = relu(conv + bias + res...) */
#define PP_RELU_FIRST 2  /* y = res + relu(conv + bias)   (VideoPose3D blocks) */
/* activations of the DeepSortYOLOv4 path (wrappers/deep_sort_yolov4/yolo4/model.py:25-75, tools/freeze_model.py),
 * applied like PP_RELU_FIRST: y = res + act(conv + bias).  Transcendentals are evaluated in double precision and
 * rounded to float once (Mish: tanh(softplus(x)) in double, rounded, then a float product with x). */
#define PP_ACT_LEAKY 3   /* LeakyReLU(alpha = 0.1f) */
#define PP_ACT_MISH 4    /* x * tanh(softplus(x)) */
#define PP_ACT_ELU 5     /* x > 0 ? x : exp(x) - 1 */
#define PP_ACT_SWISH 6   /* x * sigmoid(x)  (mmcv Swish: YOLOX of the ByteTrack config, _base_/models/yolox_x_8x8.py) */
/* PP_OP_DWCONV3X3 only (the convolution kernels have no GELU): 0.5 x (1 + erf(x / sqrt 2)) in double, rounded once */
#define PP_ACT_GELU 7
#define PP_DW_GELU_IN 1  /* pp_op.pad_end of a PP_OP_DWCONV3X3: GELU on the input values */

typedef struct pp_op {
    int32_t type;
    int32_t in, out;          /* buffer ids */
    int32_t res1, res2;       /* residual buffer ids, -1 = none; order: ((acc+bias) + res1) + res2 */
    int32_t cin, cout;        /* cin % 4 == 0 (pad the blob); cout arbitrary */
    int32_t kh, kw, stride, pad_h, pad_w, dil_h, dil_w;
    int32_t relu;             /* PP_RELU_* */
    int32_t up_log2;          /* write each output to a 2^up x 2^up patch of `out` (nearest upsample) */
    int32_t out_nchw;         /* 1: write `out` as [n][cout][H][W] planes (heatmaps) */
    int32_t res1_shift;       /* read res1 at (h >> s, w >> s)  (FPN top-down add) */
    int32_t res1_off_w;       /* read res1 at w + off (VideoPose3D centre-cropped residual) */
    int32_t out_c_off;        /* write channels [out_c_off, out_c_off + cout) of a wider `out` buffer (Concatenate) */
    int32_t in_c_off;         /* max pool only: read channels [in_c_off, in_c_off + cin) of `in` */
    int32_t pad_end;          /* bit 0 / 1: one extra zero row at the bottom / column at the right (TensorFlow SAME);
                                 bit 2 / 3: pad_h / pad_w apply in front only: the last output row / column of the
                                 symmetric-padding result is not computed (the 2x2 sub-convolutions of a deconvolution) */
    int64_t w_off, b_off;     /* float offsets into the weight blob: W (layout below), bias[cout_pad16] */
    /* ABI 7 -- PP_OP_UPSAMPLE_ADD and PP_OP_BILINEAR_ADD only (every other op: -1 / 0): two more coarse inputs, so that a whole HRNet fuse sum
     * y_i = relu(((partial + up(t_a)) + up(t_b)) + up(t_c)) is ONE pass over the fine map (mmpose's `y += ...` order) */
    int32_t in2, in3;         /* buffer ids, -1 = none */
    int32_t up2_log2, up3_log2;
} pp_op;

typedef struct pp_buf {
    int32_t h, w, c;          /* per-sample dims */
    int32_t pad;              /* > 0: the buffer is stored [h + pad][w + pad][c] per sample with `pad` ZERO columns at the right of
                                 every row and `pad` zero rows below every image (never written).  A padded 3x3 convolution
                                 reading it needs no bounds test: a tap left of column 0 lands in the previous row's zero
                                 columns, a tap above row 0 in the previous image's zero rows (or before the buffer, where the
                                 buffer descriptor returns zeros).  Only PP_OP_CONV may touch a padded buffer; buffers that
                                 pp_net_buffer / pp_net_forward expose must have pad = 0. */
} pp_buf;

/* weights: host pointer to the flat fp32 blob (copied to the device once).  max_batch fixes the
 * size of the resident activation arena. */
int pp_net_create(pp_ctx* ctx, const pp_op* ops, int n_ops, const pp_buf* bufs, int n_bufs,
                  const float* weights, size_t n_weights, int max_batch, pp_net** out);
/* same, with `weights` in `weights_mem` memory: PP_MEM_DEVICE takes a blob that is already resident (the tensor an
 * RCCL broadcast delivered -- wrappers/mmtrack.py:30 / wrappers/mmpose.py:57 load a checkpoint file per process instead)
 * and copies it device-to-device into the program's own allocation; no host round trip. */
int pp_net_create_mem(pp_ctx* ctx, const pp_op* ops, int n_ops, const pp_buf* bufs, int n_bufs,
                      const float* weights, size_t n_weights, int weights_mem, int max_batch, pp_net** out);
/* same, with the program's convolution numerics chosen explicitly (they are a property of the net, fixed here: split weights
 * are built at creation, and every later launch of this net -- from any thread, under any later pp_conv_exact call -- runs the
 * same kernels):  PP_NET_NUMERICS_DEFAULT = what pp_conv_exact / POSEPIPE_CONV_EXACT select at this moment (what pp_net_create
 * and pp_net_create_mem do), PP_NET_NUMERICS_EXACT = every layer on the float32 MFMA kernels (bit-identical to
 * oracle/conv_ref.c), PP_NET_NUMERICS_SPLIT = eligible layers on the bf16 matrix cores (three-way split, see pp_conv_exact). */
#define PP_NET_NUMERICS_DEFAULT 0
#define PP_NET_NUMERICS_EXACT 1
#define PP_NET_NUMERICS_SPLIT 2        /* the split form pp_conv_split_kind selects at this moment */
#define PP_NET_NUMERICS_SPLIT_BF16 3   /* three bfloat16 terms per operand, six products (rounds 2 - 4) */
#define PP_NET_NUMERICS_SPLIT_F16 4    /* two float16 terms per operand (per-channel / per-sample power-of-two scales), three products */
int pp_net_create_ex(pp_ctx* ctx, const pp_op* ops, int n_ops, const pp_buf* bufs, int n_bufs,
                     const float* weights, size_t n_weights, int weights_mem, int max_batch, int numerics, pp_net** out);
/* PP_NET_NUMERICS_EXACT or PP_NET_NUMERICS_SPLIT: what the net was created with (never DEFAULT) */
int pp_net_numerics(pp_net* net);
/* which split form a PP_NET_NUMERICS_SPLIT net runs (fixed at creation): PP_NET_NUMERICS_SPLIT_BF16 or PP_NET_NUMERICS_SPLIT_F16;
 * PP_NET_NUMERICS_EXACT for an exact net */
int pp_net_split_kind(pp_net* net);
void pp_net_destroy(pp_net* net);
/* device address of activation buffer `buf` (batch-major, then the pp_buf layout) */
int pp_net_buffer(pp_net* net, int buf, void** dptr, size_t* bytes_per_sample);
/* fp16-form programs scale every convolution input per sample by a power of two taken from the running maximum of the tensor
 * (pp_conv_split_kind).  For tensors produced inside the program the producing kernels track it; for a program INPUT the run takes
 * one extra pass over the buffer -- unless the caller's own producer supplies the maxima: *dptr receives the device array
 * (max_batch uint32: the bit pattern of max |x| over sample n, any upper bound >= it is valid), or NULL when no fp16-form
 * convolution reads `buf` (nothing to do).  The call is a ONE-SHOT promise: it covers the NEXT pp_net_run / pp_net_profile /
 * pp_net_capture whose op range reads `buf` -- the caller fills the array on the ctx stream before that run and calls this again
 * before every further one; an eager (not replayed) run without a fresh promise takes the maxima itself, and pp_net_forward
 * (which overwrites the buffer) voids a pending promise.
 * A captured graph fixes "promised / not promised" at CAPTURE time, not at replay:
 *  - captured with no promise pending, the graph holds the maxima pass, and every replay takes the maxima itself.  A promise made
 *    before such a replay changes nothing in it and is consumed by it: it never carries over to a later run;
 *  - captured under a promise, the graph holds NO maxima pass, and EVERY replay reads the caller's array as it stands then: the
 *    caller refills it on the ctx stream before each replay.  No further call of this function is needed for a replay (one made is
 *    consumed by it), and a run that is not a replay (another batch, an op range) still takes the maxima itself.
 * The address is stable for the life of the net.  (The detector's preprocess kernel and RoIAlign do this.) */
int pp_net_input_amax(pp_net* net, int buf, void** dptr);
/* run ops [first, last) for `batch` samples (last < 0: to the end); inputs must already be in their buffers */
int pp_net_run(pp_net* net, int batch, int first_op, int last_op);
/* convenience: copy `in` into buffer in_buf, run everything, copy buffer out_buf to `out` */
int pp_net_forward(pp_net* net, int batch, int in_buf, const float* in, int out_buf, float* out,
                   int mem);
/* Programs with >= 8 ops run on 4 HIP streams ("lanes"): independent ops (HRNet branches, FPN / RPN levels)
 * overlap, dependencies become event waits.  enable = 0 launches every op on the ctx stream in program order
 * (profiling: per-kernel durations are additive only then).  Results are identical either way. */
int pp_net_set_lanes(pp_net* net, int enable);
/* number of lanes (default 4, POSEPIPE_NET_LANES): re-plans the op -> stream assignment of an existing net (synchronises; a captured
 * graph is dropped).  1 = every op on the ctx stream.  How many pays depends on the program: branches of small maps fill each other's
 * tails (HRNet at 256x192), large maps that fill the chip on their own only disturb each other (measured round 6: the 1080p cascade
 * runs 3 % faster on 2 lanes than on 4).  Results are identical for any count. */
int pp_net_set_lane_count(pp_net* net, int n_lanes);
/* capture ops [0, n_ops) at `batch` into a hipGraph and replay it on later pp_net_run calls of the whole program at that batch (any
 * other batch or op range runs eagerly).  The capture counts as the run a pending pp_net_input_amax promise covers, and it fixes
 * that choice for every replay: captured under a promise, the graph has no maxima pass for that input and each replay reads the
 * caller's array; captured without one, each replay takes the maxima itself whatever is promised later. */
int pp_net_capture(pp_net* net, int batch);
/* per-op elapsed time of the last profiled run (HIP events around each op), ms; NULL-safe */
int pp_net_profile(pp_net* net, int batch, float* ms_per_op);
/* which kernel family each op of this net launches (fixed at creation): 0 = not a convolution, 1 = float32 MFMA kernels
 * (conv_igemm*.hip), 2 = bf16-split kernel (conv_split*.hip).  kinds: n_ops ints.  (bench.py prices the two families
 * against their own peaks.) */
int pp_net_conv_kinds(pp_net* net, int* kinds);
/* Folded projection shortcuts (fp16-form nets only; fixed at creation).  A 1x1 convolution A (any stride; no activation, no
 * residuals) whose output is read exactly once, as the plain res1 of a 1x1 / stride-1 convolution B that runs on the product kernel,
 * is not launched: B evaluates act(W_B h + W_A x + (b_B + b_A)) as ONE product over the concatenated input channels, under one
 * activation scale per sample (from the larger of the two inputs' maxima) and one weight scale per output channel (over both
 * weights).  A's output buffer is then never written.  The op numbering is the caller's: into[i] (n_ops ints) = the op that carries
 * op i, or -1 for an op that is launched; pp_net_profile reports 0 ms for a folded op, and pp_net_conv_kinds 2 (its product runs on
 * the split kernel).  POSEPIPE_SPLIT_FOLD=0 (read when a net is created) folds nothing; POSEPIPE_SPLIT_FOLD_OFF lists layer classes
 * that keep their two launches, as comma-separated "<B's cin>+<A's cin>" or "<B's cin>+<A's cin>@<out h>x<out w>" (setting it replaces
 * the built-in list).  Exact and bf16-form nets are never rewritten.  Added function only: PP_ABI_VERSION stays 10. */
int pp_net_folded_into(pp_net* net, int* into);

/* Tile configuration of the convolution kernel for all later launches of this process: ct = output-channel tile / 16
 * (1..4), pt = pixel tile / 64 (1, 2); 0 = automatic (posepipeline_amd/conv_tuning.txt, then the built-in heuristic).
 * Results do not depend on it; tools/autotune_conv.py uses it to measure every configuration per layer. */
int pp_conv_force(int ct, int pt);
/* Kernel variant for all later launches: 0 = two-barrier K step (conv_igemm.hip), 1 = three-stage software pipeline
 * (conv_igemm_p3.hip), 3 = 1 with per-geometry tap tables, 4 = the split kernel below where eligible,
 * -1 = default (POSEPIPE_CONV_VARIANT, else: the split kernel where eligible, 0 / 3 elsewhere).
 * 0, 1 and 3 give bit-identical results (the k-ordered float32 FMA chain of oracle/conv_ref.c). */
int pp_conv_variant(int variant);
/* Process-wide DEFAULT numerics: what nets created LATER with PP_NET_NUMERICS_DEFAULT get, and what the single-op entry point
 * pp_conv2d uses.  Nets that already exist are not affected (ABI 7: their numerics were fixed at creation); safe to call from
 * any thread.
 * Default (0, or -1 with POSEPIPE_CONV_EXACT unset): 3x3 / stride-1 convolutions, 1x1 convolutions from 256 input channels with
 * a multiple of 128 output channels (any from 1024), and full-cover 'valid' convolutions (the RoI head's FCs) run on
 * v_mfma_f32_32x32x16_bf16 -- every float32 operand is split EXACTLY into three bfloat16 values and the six
 * partial products down to 2^-16 relative weight are accumulated in float32 (conv_split.hip).  The dropped terms are <= 2^-23
 * of a product, one float32 rounding; measured against a float64 convolution the result is as accurate as the float32 FMA
 * chain (tests/test_gpu_split.py), but it is not bit-identical to it.
 * exact = 1 (or POSEPIPE_CONV_EXACT=1): every layer on the float32 MFMA kernels, bit-identical to oracle/conv_ref.c.
 * exact = -1: back to the environment's choice. */
int pp_conv_exact(int exact);
/* Process-wide DEFAULT split form: what PP_NET_NUMERICS_SPLIT (and DEFAULT, when it resolves to split) nets created LATER and the
 * single-op entry point get.  f16 = 1 (the default since round 5): two float16 terms per operand and three
 * v_mfma_f32_32x32x16_f16 products per term (half the matrix work of the six-product form; same float32 accumulation).  Weights are
 * normalised per output channel, activations PER SAMPLE by a power of two taken from the running maximum of the tensor -- tracked by
 * the kernel that produces it, or by one extra pass for tensors that come from outside the program -- so nothing saturates at any
 * magnitude of the data and a sample's result does not depend on what else is in the batch.  The precision is RELATIVE TO THE
 * SAMPLE'S MAXIMUM m (one scale per sample of the whole tensor, not per channel): elements down to 2^-17 m keep 22 significand
 * bits; below that the residual term is a float16 subnormal and the absolute error is <= 2^-39 m -- a large RELATIVE error for a
 * channel or pixel whose values are all below ~1e-5 of the sample's maximum (BN-folded nets can have such channels; the bf16 form
 * below has no such range limit, and PP_NET_NUMERICS_EXACT none at all).  Error against a float64 convolution: that of the float32
 * FMA chain or lower on inputs of one magnitude per sample, 1e-30 to 1e7 (tests/test_gpu_split.py; the test with channel ranges
 * spread over 2^20 holds the absolute bound above).  0: three bfloat16 terms, six products (rounds 2 - 4); -1: the environment's choice
 * (POSEPIPE_SPLIT_F16, default 1). */
int pp_conv_split_kind(int f16);

/* single convolution on caller-provided device/host buffers (tests, VideoPose3D, FC layers).
 * x: [n][hin][win][cin]; bias: [cout_pad16]; y per op flags.
 * w: [ceil(K/32)][cout_pad16][32], K = kh*kw*cin, k = (kh_i*kw + kw_i)*cin + c; within a chunk of 32 k's the
 * element 8*g + s of an output channel holds k = 32*chunk + 4*s + g (MFMA operand order; zero padded). */
int pp_conv2d(pp_ctx* ctx, const pp_op* op, int n, int hin, int win, const float* x,
              const float* w, const float* bias, const float* res1, const float* res2, float* y,
              int res1_h, int res1_w, int mem);

/* Crops for mmtrack's ReID branch (SortTracker.crop_imgs: `F.interpolate(img[:, :, y1:y2, x1:x2], (256, 128), 'bilinear',
 * align_corners=False)` on the DETECTOR's normalised input tensor, mot/deepsort/deepsort_*.py:43-49).  src: DEVICE [n_src][src_h]
 * [src_w][4] float32; rects5: HOST int32 [n][5] = (source image, x1, y1, x2, y2), x2 > x1, y2 > y1, inside the image;
 * out: DEVICE [n][out_h][out_w][4].  PyTorch's float32 upsample_bilinear2d arithmetic. */
int pp_crop_resize_bilinear(pp_ctx* ctx, const float* src_nhwc4, int n_src, int src_h, int src_w, const int32_t* rects5, int n,
                            int out_h, int out_w, float* out_nhwc4);

/* ---- ViT encoder (bf16 MFMA path) -----------------------------------------------------------
 * BASELINE.json configs[4] "ViTPose-H backbone (bf16 MFMA path)".  ViTPose is NOT in the reference tree; it fills the
 * same slot as the HRNet programs (the model `init_pose_model` builds at wrappers/mmpose.py:57 and
 * `inference_top_down_pose_model` runs at :75).  Architecture as published for ViTPose (mmpose 0.x fork): ViT with
 * patch 16 / padding 2, learned position embedding (cls slot folded in), pre-norm blocks (LayerNorm eps 1e-6, qkv bias,
 * erf GELU), final LayerNorm; head: two ConvTranspose2d(k4, s2, p1) + BN + ReLU and a 1x1 conv.
 *
 * PP_OP_VIT_ENCODER: `in`  [h][w][dim] fp32 = patch embeddings (a PP_OP_CONV with kh = kw = stride = 16, pad 2),
 *                    `out` [h][w][dim] fp32 = tokens after the final LayerNorm;  h * w = tokens (192 = 16 x 12).
 *   cin = cout = dim, kh = depth, kw = heads, stride = hidden / dim (MLP ratio); dim / heads in {64, 80}.
 *   w_off: fp32 parameter block  pos[tokens][dim],
 *          depth x { ln1_g[dim], ln1_b[dim], Wqkv[3 dim][dim], bqkv[3 dim], Wproj[dim][dim], bproj[dim],
 *                    ln2_g[dim], ln2_b[dim], W1[hidden][dim], b1[hidden], W2[dim][hidden], b2[dim] },
 *          lnf_g[dim], lnf_b[dim]          (matrices in nn.Linear layout [out][in]; qkv rows = (q|k|v, head, head_dim)).
 *   The matrices are converted to bf16 (RNE) once at pp_net_create.  Numerics: fp32 residual stream; LayerNorm
 *   output, qkv, softmax numerators exp(s - max), attention output and GELU output are rounded to bf16; every
 *   contraction accumulates in fp32 (v_mfma_f32_16x16x32_bf16).  Not bit-reproducible against a CPU restatement
 *   (the MFMA's internal summation order is not architected): parity tolerance is stated in tests/test_gpu_vit.py.
 *
 * The building blocks are exported on their own (tests, other callers); ALL pointers are device pointers:
 *   pp_gemm_bf16      C[m][n] = act(A[m][k] . W[n][k]^T + bias[n]) + res[row][n];  A, W bf16; bias / res fp32 or NULL;
 *                     act 0 none / 1 GELU(erf); res row = m % res_mod when res_mod > 0; C fp32 or bf16 (out_bf16);
 *                     k % 64 == 0, n % 128 == 0.
 *   pp_layernorm      y = (x - mean) * rsqrt(var + eps) * gamma + beta over the last dim (biased variance), x fp32
 *   pp_attention_bf16 qkv [batch * tokens][3][heads][head_dim] bf16 -> out [batch * tokens][heads * head_dim] bf16,
 *                     softmax(q k^T / sqrt(head_dim)) v;  (tokens, head_dim) in {(192, 80), (192, 64)}
 *   pp_f32_to_bf16    round-to-nearest-even conversion
 */
/* HIP-event timing of the encoder's kernel families (bench.py's roofline leg).  enable != 0: record one event after
 * every launch of later runs.  ms3 (may be NULL): {bf16 GEMMs, LayerNorms, attention} milliseconds of the last recorded
 * run, n_gemm its GEMM launch count; synchronises the ctx stream. */
int pp_net_vit_timing(pp_net* net, int enable, float* ms3, int* n_gemm);
int pp_f32_to_bf16(pp_ctx* ctx, const float* x, uint16_t* y, size_t n);
int pp_gemm_bf16(pp_ctx* ctx, const uint16_t* a, const uint16_t* w, const float* bias, const float* res, int res_mod,
                 void* c, int m, int n, int k, int act, int out_bf16);
int pp_layernorm(pp_ctx* ctx, const float* x, const float* gamma, const float* beta, int rows, int dim, float eps,
                 void* y, int out_bf16);
int pp_attention_bf16(pp_ctx* ctx, const uint16_t* qkv, int batch, int tokens, int heads, int head_dim, uint16_t* out);

/* ---- top-down pre-processing --------------------------------------------------------------
 * Replaces mmpose `_box2cs` + `TopDownAffine` (cv2.warpAffine INTER_LINEAR, border 0) + ToTensor +
 * NormalizeTensor reached from wrappers/mmpose.py:75 (pipeline spec
 * hrnet_w48_coco_384x288_dark.py:87-90,129-144); in-tree twin utils/bounding_box.py:32-53.
 * frames: [n_frames][h][w][3] u8.  For person i: frame_idx[i], bbox_tlwh[i] (x,y,w,h doubles;
 * NaN = absent -> the output sample is all zeros and valid[i] = 0).
 * lut: [3][256] fp32 = ((v/255) - mean[c]) / std[c] computed by the caller in fp32.
 * chan_map[c] = source channel feeding output channel c (reproduces the reference's double
 * BGR<->RGB swap, wrappers/mmpose.py:73).
 * out: [n_out][out_h][out_w][4] fp32 NHWC (4th channel 0); with flip != 0, n_out = 2*n_person and
 * sample n_person+i is sample i mirrored in W (`img.flip(3)` of flip_test).
 * center_scale: [n_person][4] fp32 = (cx, cy, sx, sy) as mmpose `_box2cs` returns them.
 * crop_u8 (optional, may be NULL): [n_person][out_h][out_w][3] the warped u8 crop (parity tests).
 */
int pp_crop_affine_normalize(pp_ctx* ctx, const uint8_t* frames, int n_frames, int h, int w,
                             const int32_t* frame_idx, const double* bbox_tlwh, int n_person,
                             int out_w, int out_h, const float* lut, const int32_t* chan_map,
                             int flip, float* out, float* center_scale, uint8_t* crop_u8,
                             int32_t* valid, int mem);

/* ---- flip-merge + heatmap decode ------------------------------------------------------------
 * Replaces mmpose head `inference_model` flip_back/shift/average (test_cfg
 * hrnet_w48_coco_384x288_dark.py:81-85) and `keypoints_from_heatmaps` reached from
 * wrappers/mmpose.py:75; in-tree statement of the DARK maths: utils/inference.py:27-114.
 * hm: [n][k][h][w] fp32; hm_flip: same for the mirrored input or NULL (no flip test).
 * flip_perm: [k] channel permutation applied to hm_flip (COCO left/right pairs).
 * post: 0 = 'default' (+-0.25 px), 1 = 'unbiased' (DARK, blur_kernel e.g. 17),
 *       2 = UDP (`use_udp=True`, ViTPose configs; not in the reference tree): post_dark_udp (cv2.GaussianBlur with
 *       modulate kernel e.g. 11 and reflect-101 borders, clip [0.001, 50], log, edge-replicated stencil, Newton step
 *       with inv(Hessian + eps I)) and the UDP back-mapping x * scale * 200 / (w - 1).  In pp_topdown_* post 2 also
 *       selects the UDP crop (TopDownAffine(use_udp=True)); pp_crop_affine_normalize takes it as bit 1 of `flip`.
 * center_scale: [n][4] as above.  kpts: [n][k][3] fp32 = (x_px, y_px, maxval).
 * merged (optional): [n][k][h][w] the averaged heatmap (parity tests).
 */
int pp_flip_merge_decode(pp_ctx* ctx, const float* hm, const float* hm_flip, int n, int k, int h,
                         int w, const int32_t* flip_perm, int shift_heatmap, int post,
                         int blur_kernel, const float* center_scale, float* kpts, float* merged,
                         int mem);

/* ---- fused top-down 2D stage -------------------------------------------------------------------
 * The batched body of the per-frame loop at pose_pipeline/wrappers/mmpose.py:60-76: for every
 * (frame, bbox) pair crop + normalise (+ mirrored copy), run the backbone program `net`, flip-merge
 * and decode.  All parameters stay resident; one stream synchronisation per call.
 * flip_perm == NULL disables flip_test.  Absent persons (NaN bbox) produce zero rows
 * (wrappers/mmpose.py:67-69) and valid[i] = 0.
 */
int pp_topdown_create(pp_net* net, int in_buf, int out_buf, int num_joints, const int32_t* flip_perm,
                      int shift_heatmap, int post, int blur_kernel, const float* lut,
                      const int32_t* chan_map, pp_topdown** out);
void pp_topdown_destroy(pp_topdown* t);
/* frames [n_frames][h][w][3] u8 (host or device per frames_mem); kpts [n_person][K][3] fp32 */
int pp_topdown_run(pp_topdown* t, const uint8_t* frames, int n_frames, int h, int w, int frames_mem,
                   const int32_t* frame_idx, const double* bbox_tlwh, int n_person, float* kpts,
                   int kpts_mem, int32_t* valid);
/* BASELINE config 2: the person crops are already normalised tensors [n][in_h][in_w][4] fp32;
 * center_scale [n][4] is a host array. */
int pp_topdown_run_precropped(pp_topdown* t, const float* x_nhwc4, int x_mem, const float* center_scale,
                              int n_person, float* kpts, int kpts_mem);

/* HIP-event stage times of the last pp_topdown_run*: ms3 = {pre (copies, crop / mirror), backbone program,
 * flip-merge + decode}, measured on the ctx stream. */
int pp_topdown_timing(pp_topdown* t, float* ms3);

/* ---- NMS -------------------------------------------------------------------------------------
 * Replaces mmcv-full `nms` / `batched_nms` reached from the Faster-RCNN RPN and RoI head
 * (faster_rcnn_r50_fpn.py:101-109) -- convention 0: boxes [n][4] x1y1x2y2 float32, scores [n]
 * float32; suppress IoU > thr, area = w*h.
 * convention 1 = in-tree deep_sort preprocessing.non_max_suppression
 * (wrappers/deep_sort_yolov4/deep_sort/preprocessing.py:5-70): boxes [n][4] (x, y, w, h) FLOAT64,
 * scores [n] FLOAT64, +1 areas, overlap = inter / area_other.
 * convention 2 = tf.image.non_max_suppression as called by wrappers/deep_sort_yolov4/yolo4/model.py:278-281:
 * boxes [n][4] (y1, x1, y2, x2) float32 with corners in any order, IoU = inter / (Sa + Sb - inter), 0 when an
 * area is <= 0; the caller truncates to max_output_size.
 * keep[n] receives the surviving indices in descending score order, *n_keep their count; n <= 8192.
 */
int pp_nms(pp_ctx* ctx, const void* boxes, const void* scores, int n, double iou_thr, int convention,
           int32_t* keep, int32_t* n_keep, int mem);

/* ---- tracker (host) ---------------------------------------------------------------------------
 * Replaces the association stage of wrappers/mmtrack.py:45 (mmtrack SortTracker) with the one
 * tracker whose source is in the reference tree: wrappers/deep_sort_yolov4/deep_sort/
 * (tracker.py:10-131, track.py, kalman_filter.py:14-217, linear_assignment.py:14-186,
 * iou_matching.py:7-84).  float64 throughout, scipy-compatible Hungarian tie-breaking.
 * mode 0 = in-tree DeepSORT semantics without appearance features (IoU-only association);
 * mode 1 = mmtrack-style SORT (ids from 0, tentative handling as SURVEY.md A6; unpinned).
 */
/* mode 0: (feat_dim >= 1, max_iou_distance .7, max_cosine_distance .3, max_age 30, n_init 3) are the
 * defaults of tracker.py:40 / parser.py:35-47.  mode 1: max_iou_distance carries match_iou_thr (.5)
 * and max_cosine_distance carries obj_score_thr (.5); feat_dim, max_age, n_init are ignored. */
int pp_tracker_create(int mode, int feat_dim, double max_iou_distance, double max_cosine_distance,
                      int max_age, int n_init, pp_tracker** out);
void pp_tracker_destroy(pp_tracker* t);
/* One frame.  dets_tlwh: [n_det][4] float64 (x, y, w, h), conf: [n_det], feats: [n_det][feat_dim]
 * (mode 0 only, may be NULL in mode 1).  Outputs (capacity cap):
 *   mode 0: every live track after the update, as parser.py:76-86 emits them: track_id, tlwh (from the
 *           Kalman mean), info[4] = (state, hits, age, time_since_update);
 *   mode 1: boxes are the detector's (x1, y1, x2, y2) rows (float32 values widened to double); every kept
 *           detection (score > thr) comes back with its id: tlwh = the input row, info[1] = its index. */
int pp_tracker_step(pp_tracker* t, const double* dets_tlwh, const double* conf, const double* feats,
                    int n_det, int cap, int64_t* track_id, double* tlwh, int32_t* info, int32_t* n_out);
/* debugging / parity: dump all live tracks (id, state, hits, age, time_since_update, mean[8], cov[64]) */
int pp_tracker_dump(pp_tracker* t, int cap, int64_t* ids, int32_t* state4, double* mean8,
                    double* cov64, int32_t* n_out);
/* kalman_filter.py:31-217 entry points on their own (float64; mean[8], cov[8][8], z = (x, y, a, h)) */
int pp_kalman_initiate(const double* z4, double* mean8, double* cov64);
int pp_kalman_predict(double* mean8, double* cov64);
int pp_kalman_update(double* mean8, double* cov64, const double* z4);
int pp_kalman_gating_distance(const double* mean8, const double* cov64, const double* z4, int n,
                              double* out);
/* scipy.optimize.linear_sum_assignment restated (rectangular, float64); row4col/col4row sized
 * by n_rows / n_cols; returns assignment pairs sorted by row like scipy. */
int pp_linear_sum_assignment(const double* cost, int n_rows, int n_cols, int32_t* rows,
                             int32_t* cols, int32_t* n_pairs);

/* ---- detector ------------------------------------------------------------------------------------
 * Faster-RCNN R50-FPN person detector = the detection half of `mmtrack.apis.inference_mot`
 * (wrappers/mmtrack.py:45), batched over frames.  net_a: image program (input [Hp][Wp][4]; outputs:
 * 5 RPN objectness maps [H][W][3], 5 RPN delta maps [H][W][12], FPN P2..P5 [H][W][256]); net_b: RoI-head
 * program (input [7][7][256] per RoI; outputs cls [1][1][2], reg [1][1][4]; max_batch >= 1000 per frame).
 * bufs_a = {input, cls0..4, reg0..4, p2..p5} (15 ids), bufs_b = {roi_in, cls, reg}.  cls_l == reg_l (all levels) selects the fused
 * head layout: ONE map [H][W][16] per level, objectness in channels 0 - 2, deltas in 3 - 14 (rpn_cls and rpn_reg as one convolution).
 * lut: [3][256] fp32 = (v - mean[c]) * (1/std[c]) (mmcv imnormalize); channel c of the decoded BGR frame
 * feeds tensor channel c (the reference's double BGR<->RGB swap, wrappers/mmtrack.py:43 + to_rgb=True).
 * base_anchors: [5][3][4] fp32 (AnchorGenerator scales [8], ratios [.5,1,2], strides 4..64).
 * Test-time constants are those of faster_rcnn_r50_fpn.py:101-109.
 */
typedef struct pp_detector pp_detector;
/* mmcv rescale_size for img_scale (1088,1088) + Pad(size_divisor=32): resized and padded input dims */
int pp_detector_input_size(int src_h, int src_w, int32_t* nh, int32_t* nw, int32_t* hp, int32_t* wp);
/* The same mmcv test pipeline on its own (Resize keep_ratio -> Normalize -> Pad(size_divisor, pad_val)), used by the
 * YOLOX detector of the ByteTrack config (mot/bytetrack/ *.py: img_scale (800, 1440), mean 0 / std 1, pad 114):
 * pp_rescale_size = mmcv.rescale_size + the padded dims; pp_resize_pad_normalize writes device [n][hp][wp][4] fp32
 * (lut[c][v] applied to channel c of the BGR frame, 4th channel 0, padding = pad_val). */
int pp_rescale_size(int src_h, int src_w, int max_long, int max_short, int divisor, int32_t* nh, int32_t* nw,
                    int32_t* hp, int32_t* wp);
int pp_resize_pad_normalize(pp_ctx* ctx, const uint8_t* frames, int n, int src_h, int src_w, int frames_mem, int nh,
                            int nw, int hp, int wp, const float* lut, float pad_val, float* out_device);
/* The detector's test-time constants, for pinning against the vendored configs (faster_rcnn_r50_fpn.py:101-109, mot_challenge.py:33-47):
 * out[15] = {rpn nms_pre, rpn NMS IoU, rpn max_per_img, rcnn score_thr, rcnn NMS IoU, rcnn max_per_img, img_scale long, img_scale
 * short, Pad size_divisor, RoIAlign output_size, SingleRoIExtractor finest_scale, bbox_head target_stds[4]}.  Returns 15. */
int pp_detector_constants(double* out, int cap);
int pp_detector_create(pp_net* net_a, pp_net* net_b, const int32_t* bufs_a, const int32_t* bufs_b, int src_h,
                       int src_w, const float* lut, const float* base_anchors, pp_detector** out);
void pp_detector_destroy(pp_detector* d);
/* frames: [n_frames][src_h][src_w][3] u8 BGR (host or device per frames_mem; NULL = the program input
 * buffer was filled by the caller).  dets: host [n_frames][100][5] = (x1, y1, x2, y2, score) in source
 * pixels, n_dets: host [n_frames].  proposals / n_proposals (optional, host): [n_frames][1000][4], [n_frames]. */
int pp_detector_run(pp_detector* d, const uint8_t* frames, int n_frames, int frames_mem, float* dets,
                    int32_t* n_dets, float* proposals, int32_t* n_proposals);
/* HIP-event stage times of the last run, ms6 = {preprocess, image program, RPN proposals + NMS, RoIAlign,
 * RoI-head program, final decode + NMS} */
int pp_detector_timing(pp_detector* d, float* ms6);
/* The same pass in two halves (ABI 10): pp_detector_enqueue queues everything on the ctx stream -- resize, both programs, RPN / NMS /
 * RoIAlign, the copies of the results into the detector's page-locked staging -- and returns; pp_detector_collect waits for that pass
 * (an event: work queued BEHIND it on the stream is not waited for) and hands the results over.  One pass in flight per detector.
 * A caller that enqueues chunk k + 1 before it processes chunk k's detections on the host keeps the stream fed across its own host
 * work (tracker, bookkeeping) without a second stream or thread: posepipeline_amd/cascade.py.  Host frames (PP_MEM_HOST) must stay
 * valid until the collect.  pp_detector_run = enqueue + collect. */
int pp_detector_enqueue(pp_detector* d, const uint8_t* frames, int n_frames, int frames_mem, int want_proposals);
int pp_detector_collect(pp_detector* d, float* dets, int32_t* n_dets, float* proposals, int32_t* n_proposals);
/* Decision margins (round 6): how far every INTEGER decision of the detection path is from flipping, per frame.  The path takes
 * thousands of discrete decisions on float32 values (top-1000 per level, NMS 0.7, top-1000, RoI level, score > 0.05, NMS 0.5,
 * top-100: faster_rcnn_r50_fpn.py:101-109); an evaluation that is as accurate but not bit-identical -- this library's default
 * convolution numerics, or the reference's own cuDNN kernels -- may legitimately flip one that sits on its threshold.  With margins
 * enabled every pp_detector_run also returns, per frame, the distance of the CLOSEST decision of each class to its threshold, so the
 * caller knows which frames are decided (every margin above the evaluation's error) and which are not (re-run those on a
 * PP_NET_NUMERICS_EXACT detector: posepipeline_amd/cascade.py id_numerics="certified").  +inf = no decision of that class.
 *   PP_DET_MARGIN_RPN_CUT    score gap across the per-level top-k cut (min over the levels that have one)
 *   PP_DET_MARGIN_RPN_NMS    NMS 0.7, IoU units: min over kept proposals of (thr - IoU) to every kept predecessor, over suppressed
 *                            ones of their BEST suppressor's min(IoU - thr, score_weight * its score lead)
 *   PP_DET_MARGIN_RPN_TOP    score gap across the max_per_img cut of the kept proposals
 *   PP_DET_MARGIN_ROI_LEVEL  min |log2(sqrt(w h) / 56 + 1e-6) - b|, b in {1, 2, 3}, over the RoIs (which FPN level is sampled)
 *   PP_DET_MARGIN_SCORE_THR  min |score - 0.05| over the RoIs
 *   PP_DET_MARGIN_DET_NMS    NMS 0.5 on the scored boxes, as RPN_NMS
 *   PP_DET_MARGIN_DET_TOP    score gap across the top-100 cut
 *   PP_DET_MARGIN_DET_ORDER  smallest score gap between neighbouring OUTPUT rows (the tracker numbers new tracks in row order)
 * score_weight converts a score lead into IoU units inside the two NMS margins (a suppressor only counts while it stays ahead of
 * the box it suppresses): (IoU error bound) / (2 x score error bound) of the evaluation to be certified.  Costs ~1 ms per 64 frames;
 * off by default. */
#define PP_DET_N_MARGINS 8
#define PP_DET_MARGIN_RPN_CUT 0
#define PP_DET_MARGIN_RPN_NMS 1
#define PP_DET_MARGIN_RPN_TOP 2
#define PP_DET_MARGIN_ROI_LEVEL 3
#define PP_DET_MARGIN_SCORE_THR 4
#define PP_DET_MARGIN_DET_NMS 5
#define PP_DET_MARGIN_DET_TOP 6
#define PP_DET_MARGIN_DET_ORDER 7
int pp_detector_enable_margins(pp_detector* d, int enable, float score_weight);
/* margins [n_frames][PP_DET_N_MARGINS] of the most recent pp_detector_run / collected pass (n_frames = that pass's).  Refused
 * while a pass is in flight (between pp_detector_enqueue and pp_detector_collect): its margins are published by the collect. */
int pp_detector_margins(pp_detector* d, int n_frames, float* margins);

/* Regression of caller-supplied boxes through the RoI head (Tracktor's track propagation: mmtrack TracktorTracker.regress_tracks ->
 * roi_head.simple_test_bboxes(rescale=True) with rcnn_test_cfg None).  Valid after a COLLECTED pass that contained `frame` and
 * before the next pass (the frame's FPN maps are resident in the image program's buffers); 0 < n <= the detector's RoI capacity
 * (1000).  boxes_src_px: host [n][4] x1 y1 x2 y2 in source pixels; they are multiplied by the detector's scale factor (float32),
 * mapped to their FPN level and RoI-aligned like proposals, run through the RoI program with batch n, decoded (delta2bbox, no
 * clipping) and divided by the scale factor.  out_boxes host [n][4], out_scores host [n] (foreground softmax): row i belongs to
 * input row i -- no score threshold and no NMS.  Synchronises the ctx stream.  The pass's own outputs are not touched. */
int pp_detector_regress(pp_detector* d, int frame, const float* boxes_src_px, int n, float* out_boxes, float* out_scores);

/* ---- ECC image alignment (camera-motion compensation of the Tracktor configuration; csrc/ecc.hip) -----------------------
 * pp_gray_from_nhwc4: gray = (0.299 x[r] + 0.587 x[g]) + 0.114 x[b] in float32 (cv2.COLOR_RGB2GRAY on a float image) of a device
 *   [n][h][w][4] tensor -> device [n][h][w]; queued on the ctx stream, no synchronisation.
 * pp_ecc_euclidean: cv2.findTransformECC(template, input, identity, MOTION_EUCLIDEAN, (num_iters, stop_eps), None, 1) of n_pairs
 *   image pairs at once (the algorithm is restated in csrc/ecc.hip).  gray: device [n_images][h][w] float32 (NOT inside the ctx
 *   scratch); pairs: host [n_pairs][2] = (template image, input image).  Outputs (host): warp [n_pairs][6] row-major 2 x 3 map in
 *   float64, rho [n_pairs], iters [n_pairs] loop bodies executed, status [n_pairs] PP_ECC_*.  A pair whose status is not PP_ECC_OK
 *   (OpenCV raises cv2.error there) keeps the map it had when the failing iteration began; the other pairs are unaffected.
 *   Deterministic: two calls on the same inputs return the same bits.  One stream synchronisation, at the end. */
enum { PP_ECC_OK = 0, PP_ECC_NAN = 1 /* rho is NaN */, PP_ECC_DIVERGED = 2 /* non-positive denominator of lambda */ };
int pp_gray_from_nhwc4(pp_ctx* ctx, const float* x_nhwc4, int n, int h, int w, int r, int g, int b, float* gray);
int pp_ecc_euclidean(pp_ctx* ctx, const float* gray, int n_images, int h, int w, const int32_t* pairs, int n_pairs, int num_iters,
                     double stop_eps, double* warp, double* rho, int32_t* iters, int32_t* status);

/* ---- DeepSortYOLOv4 pre / post-processing ------------------------------------------------------------
 * tracking_method 0 (pipeline.py:519-523 -> wrappers/deep_sort_yolov4/parser.py:21): YOLOv4 detector + mars-small128
 * appearance encoder + the in-tree DeepSORT tracker (pp_tracker mode 0).  The two networks are layer programs
 * (posepipeline_amd/models/yolov4.py, mars.py); these entry points are the image and box arithmetic around them.
 *
 * pp_letterbox_bicubic: letterbox_image (yolo4/utils.py:21-32: PIL Image.resize BICUBIC = Pillow's 8-bit two-pass
 *   resampler, then paste on a (128,128,128) canvas) + yolo.py:93-95 float32 / 255, with the BGR->RGB swap of
 *   parser.py:55 folded in.  frames [n][src_h][src_w][3] u8 BGR; out: device [n][size_h][size_w][4] fp32 (R,G,B,0).
 *   xtab [nw][2+kx] / ytab [nh][2+ky] int32 (host): per output index (first source index, tap count, coefficients
 *   << 22) as Pillow's precompute_coeffs + normalize_coeffs_8bpc produce them (models/yolov4.py:pil_bicubic_table).
 * pp_yolo_decode: yolo_head + yolo_correct_boxes + box_confidence * class probability of ONE class
 *   (yolo4/model.py:193-254; yolo.py:112 keeps 'person' only).  feats: device [n][gh][gw][3*(5+num_classes)];
 *   boxes [n][gh*gw*3][4] (y1, x1, y2, x2 in image pixels), scores [n][gh*gw*3], host or device per out_mem.
 * pp_reid_patches: the cv2.resize(INTER_LINEAR) of extract_image_patch (tools/generate_detections.py:61-62) + the
 *   encoder graph's uint8->float cast and channel reversal (tools/freeze_model.py:239-255).  rects: host [n][5]
 *   int32 (frame, sx, sy, ex, ey) from the clipped box (:44-60, host side); out: device [n][ph][pw][4] fp32. */
int pp_letterbox_bicubic(pp_ctx* ctx, const uint8_t* frames, int n, int src_h, int src_w, int frames_mem,
                         const int32_t* xtab, int nw, int kx, const int32_t* ytab, int nh, int ky, int size_h,
                         int size_w, float* out_device);
int pp_yolo_decode(pp_ctx* ctx, const float* feats, int n, int gh, int gw, int num_classes, int cls,
                   const float* anchors3x2, int input_h, int input_w, int image_h, int image_w, float* boxes,
                   float* scores, int out_mem);
int pp_reid_patches(pp_ctx* ctx, const uint8_t* frames, int n_frames, int src_h, int src_w, int frames_mem,
                    const int32_t* rects, int n, int ph, int pw, float* out_device);

/* ---- 3D lifting -----------------------------------------------------------------------------
 * Replaces VideoPose3D TemporalModelOptimized1f + ChunkedGenerator windows reached from
 * wrappers/videopose3d.py:66-85, computed in the equivalent whole-clip dilated form.
 * net: a program built for the dilated form (posepipeline_amd.models.videopose3d).
 * in_buf is [1][T + 2*pad][>= in_features], out_buf [1][T][out_features].
 *
 * pp_videopose3d_lift_many lifts n_segs tracks ("segments") in one call.  kpts2d_norm is the packed
 * [sum seg_frames[i]][in_features = 17*2] fp32 array of the tracks, segment after segment, already
 * screen-normalised (videopose3d.py:26-37); seg_frames: host [n_segs], frames per segment, each >= 0;
 * out: packed [sum seg_frames[i]][out_features = 17*3] fp32 in the same row order.
 *   - Every segment is processed in chunks of T frames with a pad-frame halo.  The halo is clamped to
 *     the SEGMENT, not to the packed array (= np.pad mode 'edge' on that track alone): segment i of
 *     `out` is exactly what a call with segment i alone returns.  A segment of 0 frames contributes no
 *     rows; n_segs == 0 or only empty segments: PP_OK, the device is not touched.
 *   - A work item is one (segment, chunk) pair and occupies ONE batch sample, [T + 2*pad][channels]
 *     with the channels >= in_features zero.  Work items of different segments share a batch, in
 *     groups of at most the net's max_batch.  What a sample holds does not depend on the grouping.
 *   - mem = PP_MEM_HOST: kpts2d_norm and out are host arrays; one upload, one download.
 *     mem = PP_MEM_DEVICE: both are device arrays that do not overlap; nothing is copied but the work
 *     table.  Either way everything is queued on the context's stream and the call returns after ONE
 *     stream synchronisation: the results are complete on return.
 * pp_videopose3d_lift is the case n_segs = 1, seg_frames = {n_frames}, PP_MEM_HOST.
 */
int pp_videopose3d_lift_many(pp_net* net, int in_buf, int out_buf, const float* kpts2d_norm,
                             const int32_t* seg_frames, int n_segs, int in_features, int out_features,
                             int pad, float* out, int mem);
int pp_videopose3d_lift(pp_net* net, int in_buf, int out_buf, const float* kpts2d_norm, int n_frames,
                        int in_features, int out_features, int pad, float* out);

/* pp_gastnet_lift_many: the chunk loop, flip test-time augmentation and camera rotation of the GAST-Net lifter
 * (posepipeline_amd/wrappers/gastnet.py: lift_chunks, camera_to_world) for n_seg tracks in one call (gastnet.hip).
 *   net        a program of posepipeline_amd.models.gastnet.  in_buf is its [17][T + 2*pad][4] input, out_buf its
 *              [17][T][3] output; T is read from the buffers.  Any other shape: PP_ERR_ARG.
 *   kpts_norm  packed [sum seg_len[i]][17][2] fp32, segment after segment: the screen-normalised H36M joints of
 *              each track's VALID frames (invalid frames are dropped by the caller), 8-byte aligned.
 *   seg_len    host [n_seg], frames per segment, each >= 1 (a segment of 0 frames: PP_ERR_ARG).
 *              n_seg == 0: PP_OK, nothing is read, written or queued.
 *   pad        (receptive field - 1) / 2 of the program.
 *   flip       != 0: a work item takes TWO batch samples, the window and its mirror image (x negated, left and
 *              right joints swapped); PP_ERR_ARG on a net with max_batch < 2.  0: one sample, no mirror image.
 *   cam_quat   host float[4] (w, x, y, z), or NULL: no rotation.
 *   out        packed [sum seg_len[i]][17][3] fp32 in the same row order; every row is written exactly once.
 *   mem        PP_MEM_HOST: kpts_norm and out are host arrays, one upload and one download.  PP_MEM_DEVICE: both
 *              are device arrays that do not overlap; nothing is copied but the work table.
 *   - A work item is one (segment, chunk of T output frames) pair.  Sample [j][w] of an item holds (x, y, 0, 0)
 *     of joint j of frame clamp(t0 - pad + w, 0, seg_len - 1) of ITS segment: edge replication at both ends of
 *     the track, and the last chunk filled up with its last frame.  Items of different segments share a batch, in
 *     groups of max_batch (/ 2 with flip) items; what a sample holds does not depend on the grouping.
 *   - For the first min(T, seg_len - t0) frames of an item: m = (y0 + mirror(y1)) / 2 (flip; else m = y0), then
 *     m + 2 (q_w (q x m) + q x (q x m)) (cam_quat; else m), every step one rounded float32 operation in the order
 *     of the host formulas: segment i of `out` equals camera_to_world(GastNetLifter.lift(segment i)) bit for bit.
 *   - The input's per-sample maxima (fp16-form convolutions) are taken by the net itself: no promise is made.
 *   - Everything is queued on the context's stream; ONE stream synchronisation; results are complete on return. */
int pp_gastnet_lift_many(pp_net* net, int in_buf, int out_buf, const float* kpts_norm, const int32_t* seg_len,
                         int n_seg, int pad, int flip, const float* cam_quat, float* out, int mem);

/* ---- bottom-up stage (crop_affine.hip, bottomup.hip) -------------------------------------------------
 * HigherHRNet + associative embedding as mmpose 0.x runs it for `mmpose_bottom_up` (wrappers/mmpose.py:84-121; test_cfg of
 * 3rdparty/mmpose/config/bottom_up/higherhrnet/coco/higher_hrnet48_coco_512x512.py).  mmpose is not vendored: the rules below
 * are an UNPINNED restatement.
 *
 * pp_warp_affine_normalize: the sibling of pp_crop_affine_normalize for a transform given by (center, scale) directly
 * (BottomUpResizeAlign: cv2.warpAffine(frame, get_affine_transform(center, scale, 0, (out_w, out_h)), (out_w, out_h)), the same
 * fixed-point bilinear warp, then the 3x256 normalisation table).  center / scale: host double[2], scale in units of 200 px;
 * every frame is warped with the same transform.  out: [n_out][out_h][out_w][4]; with flip != 0, n_out = 2 * n_frames and sample
 * n_frames + i is sample i mirrored in W.  warp_u8 (optional): [n_frames][out_h][out_w][3].  mem: where frames / out / warp_u8 live.
 *
 * The three post-processing calls share these arguments, all maps DEVICE pointers, NCHW fp32:
 *   s0 [2 * n_frames][2 * k][h0][w0]: the first output of the network (channels 0 .. k-1 heat-maps, k .. 2k-1 tags), sample
 *      n_frames + i computed from the mirrored input of sample i;  s1 [2 * n_frames][k][h1][w1]: the second (heat-maps only);
 *   flip_perm: host [k], the left / right channel permutation; (hr, wr): the size the maps are projected to;
 *   align_corners: of the bilinear resize (torch F.interpolate semantics, evaluated in float32).
 * A mirrored map is read at column w - 1 - x and channel flip_perm[c] BEFORE it is resized.
 *   heat-map:  hm[f][c] = ((((0 + R(s0[f][c])) + R(s1[f][c])) + R(flip s0[n_frames + f])) + R(flip s1[n_frames + f])) / 4
 *   tags:      tag[f][c][0] = R(s0[f][k + c]),  tag[f][c][1] = R(flip s0[n_frames + f] tag channel)
 * pp_bottomup_aggregate writes hm [n_frames][k][hr][wr].  The tags are never stored: the two other calls evaluate them where
 * they need them, through the same device function, so the values are bit-equal across calls.
 *
 * pp_bottomup_candidates (HeatmapParser.nms + top_k): a pixel survives when no pixel of its 5x5 neighbourhood (clipped to the map)
 * is larger.  Per frame and joint the max_people (<= 64) largest survivors with a value > 0 are returned in descending order;
 * EQUAL VALUES RANK BY THE LOWER FLAT INDEX y * wr + x (torch.topk leaves that order unspecified).  cand: host
 * [n_frames][k][max_people][8] fp32 = (val, x, y, tag0, tag1, hm[min(hr-1, y+1)][x] > hm[max(0, y-1)][x],
 * hm[y][min(wr-1, x+1)] > hm[y][max(0, x-1)], flat index); unused slots are (0, -1, -1, 0, 0, 0, 0, -1).  (torch fills such
 * slots with zero-valued pixels; the parser drops every candidate whose value is not above detection_threshold > 0.)
 *
 * pp_bottomup_refine (HeatmapParser.refine), all persons of a chunk in one call: for person p (of frame person_frame[p], mean
 * tag mean_tag[p][2]) and every joint c with need[p * k + c] != 0:  the first index of the maximum over the map of
 * hm - rint(sqrt((tag0 - m0)^2 + (tag1 - m1)^2)), in float32.  out: host [n_person][k][4] fp32 = (x, y, hm value there,
 * bits: 1 = the y comparison above, 2 = the x comparison); rows with need == 0 are zeros.
 */
int pp_warp_affine_normalize(pp_ctx* ctx, const uint8_t* frames, int n_frames, int h, int w, const double* center,
                             const double* scale, int out_w, int out_h, const float* lut, const int32_t* chan_map,
                             int flip, float* out, uint8_t* warp_u8, int mem);
int pp_bottomup_aggregate(pp_ctx* ctx, const float* s0, const float* s1, int n_frames, int k, int h0, int w0, int h1,
                          int w1, const int32_t* flip_perm, int hr, int wr, int align_corners, float* hm);
int pp_bottomup_candidates(pp_ctx* ctx, const float* hm, const float* s0, int n_frames, int k, int h0, int w0,
                           const int32_t* flip_perm, int hr, int wr, int align_corners, int max_people, float* cand);
int pp_bottomup_refine(pp_ctx* ctx, const float* hm, const float* s0, int n_frames, int k, int h0, int w0,
                       const int32_t* flip_perm, int hr, int wr, int align_corners, int n_person,
                       const int32_t* person_frame, const float* mean_tag, const int32_t* need, float* out);

/* ---- PoseFormer lifting (poseformer.hip; models/poseformer.py, wrappers/poseformer.py) ------------------------------------------
 * The 81-frame PoseFormer (ICCV 2021) behind pose_pipeline/wrappers/poseformer.py `process_liftformer`: 17 joints, 32 channels per
 * joint, 8 heads, 4 + 4 blocks, mlp ratio 2; inference mode.  An UNPINNED restatement of common/model_poseformer.py.
 *
 * pp_attention_f32: PP_OP_ATTENTION on its own.  qkv [batch][tokens][3 * c_buf] and out [batch][tokens][c_buf] are DEVICE pointers,
 * 16-byte aligned; c_real = heads * head dim real channels per third.  Queued on the context's stream, not synchronised.
 *
 * pp_poseformer_spatial: the spatial transformer, ONE launch for n_frames frames: kpts2d_norm [n_frames][17][2] (kpts_mem: host or
 * device) -> features [n_frames][544] (DEVICE), index joint * 32 + channel.  params: DEVICE pointer, 16-byte aligned, to
 * pp_poseformer_spatial_param_floats() floats in torch layouts:
 *   Spatial_patch_to_embedding.weight [32][2], .bias [32], Spatial_pos_embed [17][32],
 *   4 x { norm1.weight, norm1.bias, attn.qkv.weight [96][32], attn.qkv.bias [96], attn.proj.weight [32][32], attn.proj.bias,
 *         norm2.weight, norm2.bias, mlp.fc1.weight [64][32], mlp.fc1.bias [64], mlp.fc2.weight [32][64], mlp.fc2.bias },
 *   Spatial_norm.weight, Spatial_norm.bias.
 * A frame's features depend on that frame and the parameters only: not on n_frames, not on the frame's position.  With a host input
 * the call returns after one stream synchronisation, with a device input it only queues.
 *
 * pp_poseformer_lift: the whole lifter.  `net` is the temporal program (models/poseformer.py): in_buf [1][81][c], out_buf [1][81][c]
 * = Temporal_norm's output, c >= 544 with channels >= 544 exact zeros.  spatial_off / pos_off / head_off: float offsets (multiples
 * of 4) into the net's weight blob of the spatial parameter block above, of Temporal_pos_embed [81][544], and of the head block of
 * pp_poseformer_head_param_floats() floats: weighted_mean.weight [81] padded to 84, weighted_mean.bias padded to 4, head.0.weight
 * [544], head.0.bias [544], head.1.weight [51][544], head.1.bias [51] padded to 52.
 *   kpts2d_norm [n_frames][17][2], n_frames >= 81 -> out [n_frames - 80][51]: row i is the window [i, i + 81), i.e. frame i + 40.
 * The spatial kernel runs once over the clip; the windows then go, in batches of the net's max_batch, through
 *   win[b][f][:] = features[i_b + f][:] + pos[f][:]  ->  the program  ->  y[c] = sum_f w[f] x[f][c] + b, LayerNorm(eps 1e-5), Linear.
 * What a window's sample holds does not depend on the batch it shares.  mem: where kpts2d_norm and out live (PP_MEM_HOST: one upload,
 * one download).  Everything is queued on the context's stream and the call returns after ONE stream synchronisation.
 * stage_ms (optional, host float[4]): device milliseconds of this call by HIP events, summed over the batches: spatial kernel,
 * gather, temporal program, mean + head.
 */
int pp_attention_f32(pp_ctx* ctx, const float* qkv, int batch, int tokens, int heads, int c_real, int c_buf, float* out);
int pp_poseformer_spatial_param_floats(void);
int pp_poseformer_head_param_floats(void);
int pp_poseformer_spatial(pp_ctx* ctx, const float* params, const float* kpts2d_norm, int n_frames, int kpts_mem, float* features);
int pp_poseformer_lift(pp_net* net, int in_buf, int out_buf, long long spatial_off, long long pos_off, long long head_off,
                       const float* kpts2d_norm, int n_frames, float* out, int mem, float* stage_ms);

/* ---- FairMOT (fairmot.hip; models/dla.py, wrappers/fairmot.py) -------------------------------------------------------------------
 * The one-shot tracker behind pose_pipeline/wrappers/fairmot.py `fairmot_bounding_boxes`: DLA-34 with the DCN up-sampling head
 * (pose_dla_dcn), heads hm 1 / wh 4 / id 128 / reg 2.  FairMOT, DCNv2 and OpenCV are not vendored: UNPINNED restatements
 * (INTEGRATION.md); numpy twins in tests/fairmot_ref.py.  Two op types, added over existing pp_op fields: sizeof(pp_op) and
 * PP_ABI_VERSION are unchanged.
 *
 * PP_OP_DCN3X3: modulated deformable 3x3 convolution (DCNv2; stride 1, padding 1, dilation 1, one deformable group).
 *   in  [h][w][cin] (cin % 4 == 0);  in2 [h][w][>= 27] the offset / mask tensor, written by an ordinary PP_OP_CONV (conv_offset_mask):
 *   channel 2k = dy and 2k + 1 = dx of tap k = 3 i + j, channel 18 + k = the mask LOGIT of tap k (sigmoid applied here, evaluated in
 *   double and rounded once);  out [h][w][cout], cout <= 256.  kh = kw = 3, stride = 1, pad_h = pad_w = 1.
 *   w_off: W[9][cin_p][cout_p] (tap major; cin_p, cout_p = cin, cout rounded up to 32, zero filled), b_off: bias[cout_p].
 *   Sample position of tap k at output (y, x): py = float(y - 1 + i) + dy, px = float(x - 1 + j) + dx (float32).  The sample is 0
 *   unless -1 < py < h and -1 < px < w; else with y0 = floor(py), x0 = floor(px), lh = py - y0, lw = px - x0, hh = 1 - lh, hw = 1 - lw:
 *     sample[ci] = (((hh hw) v00 + (hh lw) v01) + (lh hw) v10) + (lh lw) v11,   v.. = x[y0 + .][x0 + .][ci], 0 outside the map
 *   (DCNv2's dmcn_im2col_bilinear), each product and sum rounded to float32, then column = sample * mask.
 *   out[y][x][co] = act(sum_k sum_ci W[k][ci][co] column_k[ci] + bias[co]): ONE fmaf chain over (k, ci) in that order from 0 (the
 *   float32-input MFMA), then + bias; relu: PP_RELU_NONE / PP_RELU_LAST.  The same kernel in exact and split nets.
 *   The columns of a tile of 64 output pixels exist in LDS only; no column tensor is written to global memory.
 * PP_OP_DWDECONV: depthwise ConvTranspose2d(c, c, 2 s, stride s, padding s / 2, groups = c, bias = False), s = stride even.
 *   in [h][w][c] -> out [h s][w s][c], cin = cout = c % 4 == 0, kh = kw = 2 s, pad_h = pad_w = s / 2; w_off: w[2 s][2 s][c].
 *   out[oy][ox][c] = sum over (ky ascending, kx ascending) with (oy + pad - ky) = s iy, (ox + pad - kx) = s ix inside the map of
 *   in[iy][ix][c] * w[ky][kx][c]: acc = 0, acc = acc + x * w, each rounded to float32 (no FMA); at most 2 x 2 terms.
 *   res1 >= 0: out = acc + res1[oy][ox][c] (one more float32 add: bit-identical to a separate addition).
 */
#define PP_OP_DCN3X3 16
#define PP_OP_DWDECONV 17
/* pp_fairmot_input_size: network size (hp, wp) = (608, 1088), or (1088, 608) when src_h > src_w; every frame is first resized to
 * 1920 x 1080 whatever its size (upstream LoadVideo), then letterboxed: ratio = min(hp / 1080, wp / 1920), (nw, nh) =
 * (round(1920 ratio), round(1080 ratio)), top = round((hp - nh) / 2 - 0.1), left = round((wp - nw) / 2 - 0.1), Python's round.
 *
 * pp_fairmot_preprocess: frames [n][src_h][src_w][3] u8 BGR (frames_mem: host or device) -> out_device [n][hp][wp][4] float32 =
 * (R, G, B, 0) / 255.  Per output pixel inside the letterbox: cv2.resize(INTER_AREA) from the 1920 x 1080 image (float32 tables
 * of computeResizeAreaTab; buf = sum_k S[sx_k] alpha_k from 0 in k order, sum = beta_0 buf_0, sum = sum + beta_j buf_j; stored with
 * round half to even, clamped to [0, 255]), whose pixels are the source's (1920 x 1080 sources) or cv2.resize(INTER_LINEAR)'s 8-bit
 * fixed-point bilinear (11-bit coefficients, (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2), recomputed where needed.
 * Outside: 128 / 255.  Returns after one stream synchronisation.
 *
 * pp_fairmot_decode: head maps, DEVICE pointers, NHWC: hm [n][h][w][1] logits, wh [n][h][w][4], reg [n][h][w][2], id [n][h][w][id_dim].
 *   score = float32 sigmoid (evaluated in double, rounded once); a pixel is a peak when no pixel of its 3x3 neighbourhood (clipped
 *   to the map) has a larger score -- a plateau keeps all its members.  The K (<= h w) largest peaks in descending order; EQUAL
 *   SCORES RANK BY THE LOWER FLAT INDEX y w + x (torch.topk leaves that order unspecified).
 *   dets [n][K][5] = (xs - wh0, ys - wh1, xs + wh2, ys + wh3, score), xs = x + reg0, ys = y + reg1, in heat-map cells;
 *   feats [n][K][id_dim] = id / max(||id||_2, 1e-12); inds [n][K] the flat indices.  Slots beyond the number of peaks hold index -1
 *   and zeros.  mem: where dets / feats / inds live (PP_MEM_HOST: copied back, one stream synchronisation). */
int pp_fairmot_input_size(int src_h, int src_w, int32_t* hp, int32_t* wp, int32_t* nh, int32_t* nw, int32_t* top, int32_t* left);
int pp_fairmot_preprocess(pp_ctx* ctx, const uint8_t* frames, int n, int src_h, int src_w, int frames_mem, int hp, int wp, int nh,
                          int nw, int top, int left, float* out_device);
int pp_fairmot_decode(pp_ctx* ctx, const float* hm, const float* wh, const float* reg, const float* id, int n, int h, int w, int K,
                      int id_dim, float* dets, float* feats, int32_t* inds, int mem);

/* ---- SMPL stage: VIBE (crop_affine.hip, gru.hip, smpl.hip; models/vibe.py, models/smpl.py, wrappers/vibe.py) ----------------------
 * The device side of pose_pipeline/wrappers/vibe.py `process_vibe`.  VIBE, SPIN and smplx are not vendored: UNPINNED restatements
 * (INTEGRATION.md); numpy / torch twins in tests/vibe_ref.py.  Added functions only: PP_ABI_VERSION stays 10.
 *
 * pp_warp_affine_normalize_each: pp_warp_affine_normalize with one FORWARD matrix per output sample (cv2.warpAffine(frame, M, (out_w,
 * out_h), INTER_LINEAR), border 0, then the table): sample i is cut from frame frame_idx[i] with matrices[i] = HOST double[6] (row
 * major 2 x 3), inverted as OpenCV inverts it.  The same fixed-point bilinear kernel.  frames [n_frames][h][w][3] u8, out
 * [n][out_h][out_w][4], crop_u8 (optional) [n][out_h][out_w][3] in the frame's channel order; mem: where frames / out / crop_u8 live.
 *
 * pp_gru_forward: nn.GRU(in, hidden, num_layers = layers, batch_first), unidirectional, zero initial state, gate order r, z, n:
 *   r = s(W_ir x + b_ir + W_hr h + b_hr), z = s(W_iz x + b_iz + W_hz h + b_hz), n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
 *   h' = (1 - z) n + z h.   x [B][T][in] -> y [B][T][hidden] = the top layer's h at every step (mem: where x and y live).
 * params: ONE DEVICE blob, 16-byte aligned, per layer l: W_ih [3 hidden][in_l], W_hh [3 hidden][hidden], b_ih [3 hidden], b_hh
 * [3 hidden] (in_0 = in, in_l = hidden; pp_gru_param_floats gives its length).  Per layer the input projection W_ih x + b_ih of all
 * B T rows is one matrix product outside the recurrence; the recurrence is ONE KERNEL LAUNCH PER (layer, time step) on the context's
 * stream -- no cooperative launch, no grid-wide barrier, no waiting on memory.  Every dot product is one wave's sum: lane q adds its
 * terms k = q, q + 64, ... (input projection) or the 4-blocks k = 4 q, 4 q + 256, ... (recurrence) as one fmaf chain, then the 64 lane sums
 * are added by a fixed butterfly.  The sigmoid and tanh are evaluated in double and rounded once.  Results are bit-identical from
 * run to run and a sequence's result does not depend on B.  hidden % 4 == 0; B, T, in, layers >= 1.  With device memory the call only queues.
 *
 * pp_smpl_model_create: the SMPL body model, resident: v_template [V][3], shapedirs [V][3][10], posedirs [207][3 V], J_regressor
 * [24][V], weights [V][24], J_regressor_extra [9][V] (HOST float32), vertex_ids [21] (the extra joints picked from the mesh, < V),
 * joint_map [49] (indices into the 54 joints below).  The kinematic tree is SMPL's.
 * pp_smpl_forward (smplx `lbs` with pose2rot = False, SPIN's joint set, VIBE's projection), per frame f of F:
 *   v_shaped = v_template + shapedirs . betas;  J = J_regressor . v_shaped;  v_posed = v_shaped + vec(R_1..23 - I) . posedirs;
 *   G_0 = [R_0 | J_0], G_i = G_parent [R_i | J_i - J_parent];  A_i = G_i with G_i J_i taken off its translation;
 *   verts = (sum_i w_vi A_i) [v_posed; 1];  joints54 = (24 chain translations, verts[vertex_ids], J_regressor_extra . verts);
 *   joints3d = joints54[joint_map];  p = joints3d + (cam1, cam2, 2 * 5000 / (224 cam0 + 1e-9));  kp2d = ((p_xy / p_z) * 5000) / 112;
 *   pose_aa = the rotation vector of each R_i through the quaternion (torchgeometry's rotation_matrix_to_quaternion branches on the
 *   transposed matrix with eps 1e-6, then 2 atan2(+-sin, +-cos) / sin, 2 where sin^2 == 0, NaN -> 0), evaluated in double, rounded once.
 * Every sum (10 betas, 207 pose features, V vertices, 24 joints) is an fmaf chain or a fixed tree: no atomics, bit-identical runs.
 * betas [F][10], rotmat [F][24][9] row major, cam [F][3] -> verts [F][V][3] (may be NULL: not returned), joints3d [F][49][3], kp2d
 * [F][49][2], pose_aa [F][72]; mem: where all of them live (PP_MEM_HOST: staged, one stream synchronisation).
 * pp_vibe_head_unpack: DEVICE pointers; pose6d [F][144], shape [F][shape_stride >= 10], cam_in [F][cam_stride >= 3] (the regressor
 * program's output buffers) -> rotmat [F][24][9] (rot6d_to_rotmat: a = pose6d viewed [24][3][2], b1 = a1 / max(|a1|, 1e-12), b2 =
 * normalised a2 - (b1 . a2) b1, b3 = b1 x b2, columns (b1, b2, b3)), betas [F][10], cam [F][3].  Queued, not synchronised. */
typedef struct pp_smpl_model pp_smpl_model;
int pp_warp_affine_normalize_each(pp_ctx* ctx, const uint8_t* frames, int n_frames, int h, int w, const int32_t* frame_idx,
                                  const double* matrices, int n, int out_w, int out_h, const float* lut, const int32_t* chan_map,
                                  float* out, uint8_t* crop_u8, int mem);
long long pp_gru_param_floats(int in, int hidden, int layers);
int pp_gru_forward(pp_ctx* ctx, const float* x, int B, int T, int in, int hidden, int layers, const float* params, float* y, int mem);
int pp_smpl_model_create(pp_ctx* ctx, const float* v_template, const float* shapedirs, const float* posedirs, const float* j_regressor,
                         const float* weights, const float* j_regressor_extra, int n_verts, const int32_t* vertex_ids,
                         const int32_t* joint_map, pp_smpl_model** out);
void pp_smpl_model_destroy(pp_smpl_model* model);
int pp_smpl_forward(pp_ctx* ctx, pp_smpl_model* model, const float* betas, const float* rotmat, const float* cam, int F, float* verts,
                    float* joints3d, float* kp2d, float* pose_aa, int mem);
int pp_vibe_head_unpack(pp_ctx* ctx, const float* pose6d, const float* shape, int shape_stride, const float* cam_in, int cam_stride,
                        int F, float* rotmat, float* betas, float* cam);

/* ---- TraDeS (trades.hip, fairmot.hip; models/trades.py, tracking.TradesTracker) ----------------------------------------------------
 * The device side of TrackingBboxMethodLookup row 4 besides the layers of models/dla.py.  TraDeS and CenterTrack are not vendored:
 * UNPINNED restatements; numpy twins in tests/trades_ref.py.  Added functions and op types over existing pp_op
 * fields only: sizeof(pp_op) is unchanged and PP_ABI_VERSION stays 10.
 *
 * pp_trades_cva: cost-volume association of n frame pairs.  emb_cur, emb_prev [n][hc][wc][128] float32 (P = hc wc cells).  With
 *   c[q][i][j] = <emb_cur[q], emb_prev[i][j]> (128 terms, ONE fmaf chain in channel order from 0: the float32-input MFMA, exact float32),
 *   ch[q][i] = max_j c[q][i][j],  cw[q][j] = max_i c[q][i][j]   (selections: exact),
 *   soft_h[q][.] = softmax_i(5 ch[q][.]),  soft_w[q][.] = softmax_j(5 cw[q][.]):  x = 5.f * v (float32), m = max x, e = exp(x - m) with
 *   x - m rounded to float32 and exp EVALUATED IN DOUBLE AND ROUNDED ONCE, s = sum e, p = e / s;
 *   off_h[q] = sum_i p_i * float(2 (i - i_q)),  off_w[q] = sum_j p_j * float(2 (j - j_q)),  q = (i_q, j_q).
 *   Sums: lane k of one wave adds its terms k, k + 64, ... in that order, then the 64 lane sums by a fixed butterfly; bit-identical
 *   from run to run.  offset [n][2 hc][2 wc][2]: channel 0 = off_w, channel 1 = off_h, each value written to the 2 x 2 block of its cell
 *   (nearest x2).  soft_h [n][P][hc] and soft_w [n][P][wc]: optional (both or neither).  The P x P volume is never written to global
 *   memory.  mem: where every pointer lives (PP_MEM_HOST: staged, one stream synchronisation; device: only queued).  hc + wc <= 510.
 *
 * pp_trades_render_prehm: CenterTrack's pre_hm after AvgPool2d(4, 4).  boxes: HOST int32 [n_boxes][3] = (cx, cy, radius) in
 *   network-input pixels, computed by the caller in the reference's float arithmetic (models/trades.prehm_boxes).  Input-resolution
 *   map (never stored): pixel (x, y) = max over the boxes with |x - cx| <= r and |y - cy| <= r of g = exp(-((x - cx)^2 + (y - cy)^2) /
 *   (2 sigma^2)), sigma = (2 r + 1) / 6, EVALUATED IN DOUBLE AND ROUNDED ONCE to float32, g < 2^-52 -> 0 (draw_umich_gaussian; the
 *   patch is clipped to the map by construction), 0 where no box reaches.  out [hp / 4][wp / 4] = float32 sum of the 4 x 4 pixels in
 *   (ky, kx) order / 16 (PP_OP_AVGPOOL's rule); mem: where out lives.  hp, wp multiples of 4.  One stream synchronisation.
 *
 * pp_trades_decode: head maps, DEVICE pointers, NHWC: hm [n][h][w][1] logits, reg [n][h][w][2], ltrb [n][h][w][4] (ltrb_amodal),
 *   tracking [n][h][w][2].  Peaks, scores, ranking and the equal-score rule (LOWER FLAT INDEX FIRST) are pp_fairmot_decode's.
 *   dets [n][K][9] = (x + reg0, y + reg1,  x + l, y + t, x + r, y + b  (amodal, about the INTEGER peak),  tracking0, tracking1,  score);
 *   inds [n][K].  Slots beyond the number of peaks hold index -1 and zeros.  mem: where dets / inds live.
 *
 * Three op types of program B (the per-frame half of the network; trades.hip):
 * PP_OP_SUB_CAT: out[y][x] = (in2[y][x][0 .. c2), 0 ..., in[y][x][c] - res1[y][x][c]): in, res1 [h][w][cin], in2 [h][w][c2], c2 <= 4,
 *   out [h][w][4 + cin]; channels [c2, 4) are zeros; cin = the map's channels, cout = 4 + cin, cin % 4 == 0.
 * PP_OP_BCAST_MUL: out[y][x][c] = in2[y][x][0] * in[y][x][c]: in, out [h][w][cin], in2 [h][w][1]; cin = cout % 4 == 0.
 * PP_OP_BLEND2: out[y][x][c] = a0 in[y][x][c] + a1 res1[y][x][c], (a0, a1) = softmax(in2[y][x][0], in3[y][x][0]): m = max, e_k =
 *   exp(l_k - m) evaluated in double and rounded once, a_k = e_k / (e_0 + e_1) (float32); the two products rounded, then added.
 *   in, res1, out [h][w][cin]; in2, in3 [h][w][1]; cin = cout % 4 == 0.  Every other field keeps its neutral value. */
#define PP_OP_SUB_CAT 18
#define PP_OP_BCAST_MUL 19
#define PP_OP_BLEND2 20
int pp_trades_cva(pp_ctx* ctx, const float* emb_cur, const float* emb_prev, int n, int hc, int wc, int dim, float* offset,
                  float* soft_h, float* soft_w, int mem);
int pp_trades_render_prehm(pp_ctx* ctx, const int32_t* boxes, int n_boxes, int hp, int wp, float* out, int mem);
int pp_trades_decode(pp_ctx* ctx, const float* hm, const float* reg, const float* ltrb, const float* tracking, int n, int h, int w,
                     int K, float* dets, int32_t* inds, int mem);

/* ---- GAST-Net lifting (gastnet.hip; models/gastnet.py, wrappers/gastnet.py) --------------------------------------------------------
 * The two ops of GAST-Net's graph-attention blocks (LiftingMethodLookup row 0 "GastNet", pose_pipeline/wrappers/gastnet_lifting.py)
 * besides convolutions.  GAST-Net is not vendored: UNPINNED restatements; numpy / torch twins in tests/gastnet_ref.py.
 * Activations are [17 joints][w time steps][channels] per sample: H is the joint axis, and both ops mix over it within one time step.
 * Float32 on the vector ALU, the same kernels in exact and split nets.  Added op types over existing pp_op fields only: sizeof(pp_op)
 * is unchanged and PP_ABI_VERSION stays 10.  Every field not named keeps its neutral value.
 *
 * PP_OP_GRAPH_MIX: channel-wise graph convolution (SemCHGraphConv), kh = g graphs (1 .. 4) in one pass.
 *   in [17][w][cin], cin = 2 cout: per graph q the channels [2 q c, 2 q c + c) = h0 (the self term), [2 q c + c, 2 q c + 2 c) = h1 (the
 *   neighbour term), c = cout / g, c % 4 == 0 (a 1x1 PP_OP_CONV writes it).  out [17][w][>= out_c_off + cout]: graph q fills the
 *   channels [out_c_off + q c, out_c_off + (q + 1) c), the others are untouched.
 *   w_off: A[g][17][17][c], A[q][j][i][ch] = the weight of source joint i in output joint j for channel ch (ch fastest; zeros off the
 *   graph's mask); b_off: bias[g][c], then nb[g][17]: nb[q][j] = the float whose integer value has bit i set when (j, i) is in the
 *   mask of graph q (the neighbour list, built on the host: it says which terms EXIST, whatever the value of A there).
 *     out[j][t][q c + ch] = act((sum over the i of nb[q][j], ascending, of A[q][j][i][ch] * (i == j ? h0 : h1)[i][t][ch]) + bias[q][ch]):
 *   ONE fmaf chain from 0 over the source joints, then one float32 add of the bias; terms outside the mask are skipped, not
 *   multiplied by zero.  relu: PP_RELU_NONE / PP_RELU_LAST.  No atomics.
 * PP_OP_JOINT_ATTN: per time step, multi-head attention over the 17 joints (MultiGlobalGraph), no scale.
 *   in [17][w][3 * cout] = the qkv map in PP_OP_ATTENTION's channel order: channel s * cout + head * hd + d holds (q, k, v)[s] of head
 *   `head`, hd = cin / heads; channels [cin, cout) of each third are padding and are not read.  out [17][w][>= out_c_off + cout]:
 *   channels [out_c_off, out_c_off + cout).  cin = heads * hd (hd % 4 == 0, hd <= 128) <= cout % 4 == 0, stride = heads; no parameters.
 *   Per sample, time step t and head, over the joints i, j:
 *     s[i][j] = q_i . k_j (one fmaf chain over d from 0);  m_i = max_j s[i][j];  e[i][j] = exp(s[i][j] - m_i) (the difference rounded to
 *     float32, exp EVALUATED IN DOUBLE AND ROUNDED ONCE);  sum_i = e[i][0] + e[i][1] + ... in joint order;  p[i][j] = e[i][j] / sum_i;
 *     out_i = sum_j p[i][j] v_j, one fmaf chain over j = 0 .. 16 from 0.
 *   Channels [out_c_off + cin, out_c_off + cout) of `out` are exact zeros.  No atomics.
 * Neither op folds its output's per-sample maxima (pp_amax.h): where a fp16-form convolution reads what they wrote, the net takes the
 * maxima in a pass of its own behind the op, as for PP_OP_ATTENTION. */
#define PP_OP_GRAPH_MIX 21
#define PP_OP_JOINT_ATTN 22

/* ---- PoseC3D skeleton action (posec3d.hip; models/posec3d.py, wrappers/mmaction.py) -------------------------------------------------
 * The device side of the SkeletonAction stage (pose_pipeline/wrappers/mmaction.py) besides the layer programs, which use PP_OP_CONV,
 * PP_OP_MAXPOOL and PP_OP_AVGPOOL only.  mmaction2 is not vendored: UNPINNED restatements; numpy / torch twins in
 * tests/posec3d_ref.py.  Added functions only: no op type, sizeof(pp_op) is unchanged and PP_ABI_VERSION stays 10.
 *
 * pp_pose_target: GeneratePoseTarget(sigma, use_score, with_kp, double) for one person.  kps: DEVICE float64 [n][K][3] = (x, y, score)
 *   in map pixels; perm: DEVICE int32 [K], the joint that channel c of a MIRRORED sample shows (left / right swapped); out: DEVICE
 *   float32 [2 n][h][w][c_pad] NHWC, c_pad % 4 == 0, c_pad >= K.  For sample s < n, (mu_x, mu_y, score) = kps[s][c]; for sample
 *   s >= n (the mirrored copies: Flip(flip_ratio 1, left_kp, right_kp) of the key points, rendered again), (x0, mu_y, score) =
 *   kps[s - n][perm[c]] and mu_x = x0 != 0 ? w - x0 : x0 in float64; a perm[c] outside [0, K) reads nothing and leaves the channel
 *   zeros.  With int() truncating toward zero,
 *     st_x = max(int(mu_x - 3 sigma), 0), ed_x = min(int(mu_x + 3 sigma) + 1, w), st_y / ed_y likewise with h;
 *     out[s][y][x][c] = float32(exp(-((x - mu_x)^2 + (y - mu_y)^2) / 2 / sigma^2) * score)   EVALUATED IN DOUBLE AND ROUNDED ONCE
 *   where st_x <= x < ed_x, st_y <= y < ed_y and not score < 1e-4; 0 elsewhere and in the channels [K, c_pad).  One person: a
 *   channel holds one patch, so the reference's np.maximum is a plain store and every element is written exactly once (no memset, no
 *   scatter, no atomics).  Queued on the ctx stream; no synchronisation.
 *
 * pp_gather_samples: dst[i] = src[idx[i]], i < n, whole samples of sample_floats floats (a multiple of 4; float4 copies; src and dst
 *   16-byte aligned, not overlapping).  idx: DEVICE int32 [n] with values in [0, n_src); a value outside that range reads nothing and
 *   fills its sample with zeros.  n <= 65535.  Queued on the ctx stream; no synchronisation. */
int pp_pose_target(pp_ctx* ctx, const double* kps, int n, int K, int h, int w, double sigma, const int32_t* perm, int c_pad, float* out);
int pp_gather_samples(pp_ctx* ctx, const float* src, int n_src, const int32_t* idx, int n, long long sample_floats, float* dst);

#ifdef __cplusplus
}
#endif
#endif /* POSEPIPE_HIP_H */
