// conv_split_gemm_kernel: the product kernel of the 1x1 / full-cover split layers, and its launcher (design: conv_split.hip).
#include "conv_split_internal.h"

std::atomic<int> g_split_gemm_epi{-1};       // pp_debug_knob("split_gemm_epilogue"): -1 = POSEPIPE_SPLIT_GEMM_EPI
std::atomic<int> g_split_gemm_tile{-1};      // pp_debug_knob("split_gemm_wave_tile"): -1 = POSEPIPE_SPLIT_GEMM_TILE

namespace {

// ---- 1x1 / full-cover layers with >= 128 output channels: 8 waves, 256 x 256 (or 512 x 128) output tile --------------------------
// A product Y[M][N] = X[M][K] W[K][N] moves 4 / (2 BN) bytes of X and 6 / (2 BM) bytes of split W per float32 FLOP through the
// vector memory path.  With the tap kernel's 256 x 64 tile that is 0.043 B/FLOP -- 10.7 TB/s at the 250 TFLOP/s the matrix pipes
// could do, and the measured ~115 TFLOP/s of that form on ResNet's 1x1 layers is exactly ~5 TB/s of it.  A 256 x 256 tile needs
// 0.0195 B/FLOP, which takes 128 accumulator registers per lane: 8 waves (wave tile 128 pixels x 64 channels), one workgroup per
// CU, BOTH operands staged through LDS (six-product form: X split once per workgroup when it is stored to LDS and shared by the
// waves along N; W copied verbatim in fragment order and shared by the waves along M), two LDS stages of 16 input channels, one
// barrier per stage (3072 matrix-pipe cycles).
// WM x WN = 8 waves: one workgroup per CU; 4 waves (256 x 128 tile): two workgroups per CU, for layers with few 16-channel stages,
// where one workgroup's start-up and epilogue hide under the other's K loop.  Only the 4-wave form is instantiated.
//
// fp16 form (H): X travels to LDS as raw float32 by DMA and is split where a wave reads its fragment, so every wave that reads a
// pixel block converts it.  WIDE: the four waves sit 4 x 1 with wave tiles of 64 pixels x 128 channels (2 pixel blocks x 4 channel
// blocks, acc[4][2]) instead of 2 x 2 with 128 x 64 (acc[2][4]): each pixel block has ONE reader, so X is again split once per
// workgroup -- per wave and stage 4 instead of 8 ds_read_b128 of pixels and ~48 instead of ~96 conversion instructions beside the
// same 24 MFMAs, and 8 instead of 4 weight-fragment reads (12 fragment reads either way).  Same workgroup tile, grid, DMA rings
// and counts; every accumulator receives the same products in the same order, so the two arrangements give the same bits
// (tests/test_gpu_split_gemm_tile.py; measurements: DESIGN_LOG.md 5y).  WIDE is the default of the fp16 form; WIDE = false is the
// kernel as it was (every difference is a constant of PBW / CBW or `if constexpr`).
//
// SEG2 (fp16 form only): a projection shortcut folded into the product.  relu(W3 h + b3 + Ws x + bs) is ONE product over the
// concatenated K = Cin + Cin2: stages [0, seg1) stream h (a.x), stages [seg1, nchunks) stream x (a.x2, read at its own stride) into the
// same pixel ring, and the weight fragments of the two segments follow each other in stage order, so the K loop itself does not know
// about segments -- only issue(c) picks the source.  Both segments add into the SAME float32 accumulators, so they share their scales:
// sample n's activation scale follows max(amax_h[n], amax_x[n]) (no rescaling between the segments: the ratio of two scales can
// overflow float32) and channel co's weight scale follows max(|W3[co, :]|, |Ws[co, :]|) (the concatenated weight is split as one).
// Error: under a scale s with max |v| s in [2^14, 2^15), h0 = f16(v s) and h1 = f16(v s - h0) leave a residual of at most
// max(2^-22 |v s|, 2^-25) (the second term's rounding; 2^-24 is the float16 subnormal spacing).  So an element down to 2^-17 of the
// scale's maximum -- an operand ~10^5 smaller than its partner segment -- still carries its 22 bits; below that its absolute error
// is at most 2^-25 / s <= 2^-39 of the JOINT maximum, far under the 2^-22-relative rounding the larger segment commits on its own
// elements, and the joint maximum is also what bounds the output.  The same holds per output channel for the weights.
// SEG2 = false is the one-segment kernel, instruction for instruction what it was (every use of the second segment is `if constexpr`).
template <int WM, int WN, bool H = false, bool SEG2 = false, bool WIDE = false>
__global__ __launch_bounds__(64 * WM * WN, 512 / (64 * WM * WN)) void conv_split_gemm_kernel(SplitArgs a) {
    static_assert(H || !SEG2, "the second K segment exists in the fp16 form only");
    static_assert(H || !WIDE, "the 64 x 128 wave tile exists in the fp16 form only");
    constexpr int PBW = WIDE ? 2 : 4, CBW = WIDE ? 4 : 2;      // 32-pixel x 32-channel blocks of a wave tile: 128 x 64, WIDE: 64 x 128
    constexpr int WPX = 32 * PBW;                    // pixels of a wave
    constexpr int XP = H ? 2 : 3;                    // activation planes (H: the fp16 form, see conv_split_kernel)
    constexpr int WPL = H ? 2 : 3;                   // weight planes
    constexpr int NT = 64 * WM * WN, NWAVE = WM * WN;
    constexpr int BM = WPX * WM, BN = 32 * CBW * WN;
    constexpr int XS = BM * 4 / NT;                  // float4 patch slots per thread and stage
    constexpr int WU = BN * 2 * WPL;                 // 16-byte units of split weights per stage: BN / 32 blocks x WPL planes x 64 lanes
    constexpr int NPp = BM + 4;
    constexpr int XPLANE = 2 * NPp * 16;
    constexpr int XBYTES = XP * XPLANE, STAGE = XBYTES + WU * 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    unsigned bx = blockIdx.x, by = blockIdx.y;
    PP_TL_DECL;
    PP_TL_MARK(0);
    if (a.xcd_remap) {      // 1-D launch, see xcd_tile_column
        if (!xcd_tile_column(blockIdx.x, a, bx, by)) return;
    }
    const unsigned L = bx, col = by;      // (names the timeline record uses)
    (void)L; (void)col;
    const long long m0 = (long long)bx * BM;
    const int cbB = by * (BN / 32);                  // first channel block of the workgroup
    const int cb0 = cbB + wn * CBW;                  // ... of this wave
    const int wp0 = wm * WPX;                        // first pixel of this wave in the tile

    // sample of the wave's first / last pixel (clamped to the tensor): equal = the wave's pixels lie in one sample
    const unsigned mfirst = (unsigned)min(m0 + wp0, a.S - 1), mlast = (unsigned)min(m0 + wp0 + WPX - 1, a.S - 1);
    const int img_first = __builtin_amdgcn_readfirstlane((int)pp_udiv(mfirst, a.dv_per)), img_last = __builtin_amdgcn_readfirstlane((int)pp_udiv(mlast, a.dv_per));
    unsigned oam_first = 0;                          // fp16 form: maximum of that sample (the epilogue's 1 / s)
    if constexpr (H) oam_first = a.x_amax[img_first];
    if constexpr (SEG2) oam_first = max(oam_first, a.x2_amax[img_first]);       // (bit patterns of non-negative floats: integer order)
    const unsigned lds_base0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const size_t wstep0 = (size_t)a.ncb * (WPL * 64);
    f32x16 acc[CBW][PBW];                             // (zeroed right in front of the K loops: 128 live registers less during the set-up)
    if constexpr (H) {
    // ---- fp16 form (round 5): the pixels travel global -> LDS by DMA as well, as raw float32; the two float16 terms are made when
    // a wave reads its B fragment.  Why: with the pixels staged through registers (rounds 2 - 4, still the six-product form below) a
    // stage could not be shorter than the latency of the loads issued ONE stage earlier -- ~1.3 us from HBM under load against
    // 0.38 us of MFMAs in this form (fc6: a lone workgroup advanced one stage per ~2700 cycles; the product layers ran at 0.13 - 0.3
    // of the matrix peak) -- and a second register set for a deeper prefetch does not fit beside 128 accumulator registers (it
    // spilled 256 B per lane and stage).  A DMA needs no registers: a ring of THREE 16 KB pixel stages ([256 pixels][16 channels],
    // rows of 64 B) + three weight stages, everything requested two stages ahead, every wait an exact count (all vector-memory
    // operations of the loop are DMAs: 4 pixel blocks + 2 weight fragments per wave and stage).
    // LDS layout of a pixel stage: pixel-major rows of 64 B, the row's four 16-byte quads XOR-swizzled by (pixel >> 1) & 3 -- applied
    // on the GLOBAL side (DMA lane i of a block writes slot i, i.e. (pixel i / 4, slot i % 4), and fetches quad slot ^ swizzle of that
    // pixel: the four lanes of a pixel still cover its 64 contiguous bytes).  A lane's fragment (pixel lane & 31, k half lane >> 5)
    // is quads 2 half and 2 half + 1 = two ds_read_b128 at the row + ((2 half) ^ swizzle) * 16 and that address ^ 16: every service
    // group of ds_read_b128 covers all 8 bank quads exactly twice (conflict-free).
    // Conversion per fragment (8 floats of one pixel): scale (power of two per sample), h0 = f16(x s), h1 = f16(x s - h0):
    // 24 vector instructions, 96 per wave and stage beside its 24 MFMAs of 32 cycles (WIDE: 48, two fragments instead of four).
    constexpr int XR = 3, XSTG = BM * 64, WR = 3, WBYTES = WU * 16;
    constexpr int NXD = BM / 16 / NWAVE;             // 1 KB pixel blocks (16 pixels) per wave and stage
    constexpr int NWD = WU / 64 / NWAVE;             // 1 KB weight fragments per wave and stage
    static_assert(BM / 16 % NWAVE == 0 && WU / 64 % NWAVE == 0, "every wave issues the same number of DMAs (vmcnt arithmetic)");
    unsigned gx[NXD];                                // byte offset of this lane's 16 bytes of stage 0 (the tensor is < 4 GiB)
#pragma unroll
    for (int i = 0; i < NXD; ++i) {
        const int pl = (wave + NWAVE * i) * 16 + (lane >> 2);
        const unsigned m = (unsigned)min(m0 + pl, a.S - 1);          // rows past the tensor: any valid address (never stored)
        int img, ho, wo;
        decode_pos(a, m, (unsigned)(a.H * a.W), (unsigned)a.W, img, ho, wo);
        gx[i] = (unsigned)(((img * a.xp_h + ho * a.stride) * a.xp_w + wo * a.stride) * a.Cin) * 4u + (unsigned)(((lane & 3) ^ ((pl >> 1) & 3)) * 16);
    }
    unsigned gx2[SEG2 ? NXD : 1];                    // ... and of the second segment's stage seg1
    if constexpr (SEG2) {
#pragma unroll
        for (int i = 0; i < NXD; ++i) {
            const int pl = (wave + NWAVE * i) * 16 + (lane >> 2);
            const unsigned m = (unsigned)min(m0 + pl, a.S - 1);
            int img, ho, wo;
            decode_pos(a, m, (unsigned)(a.H * a.W), (unsigned)a.W, img, ho, wo);
            gx2[i] = (unsigned)(((img * a.xp2_h + ho * a.stride2) * a.xp2_w + wo * a.stride2) * a.Cin2) * 4u + (unsigned)(((lane & 3) ^ ((pl >> 1) & 3)) * 16);
        }
    }
    float xsc[PBW];                                  // activation scale of the sample of pixel pb * 32 + (lane & 31)
#pragma unroll
    for (int pb = 0; pb < PBW; ++pb) xsc[pb] = pp_act_scale(oam_first);
    if (img_first != img_last) {
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb) {
            const unsigned mp = (unsigned)min(m0 + wp0 + pb * 32 + (lane & 31), a.S - 1);
            unsigned am = a.x_amax[pp_udiv(mp, a.dv_per)];
            if constexpr (SEG2) am = max(am, a.x2_amax[pp_udiv(mp, a.dv_per)]);
            xsc[pb] = pp_act_scale(am);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // (the maxima are in: from here on every vector-memory op is a DMA)
    // (scalar base + 32-bit lane offset: one address register per DMA)
    const unsigned wlane16 = (unsigned)lane * 16u;
    auto issue = [&](int c) {                         // weights and pixels of stage c
        const uint4* wsrc = a.w + (size_t)c * wstep0 + (size_t)cbB * (WPL * 64);          // workgroup-uniform
#pragma unroll
        for (int i = 0; i < NWD; ++i) {
            const int slab = i * NWAVE + wave;
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base0 + (unsigned)(XR * XSTG + (c % WR) * WBYTES + slab * 1024));
            dma_fragment(wlane16 + (unsigned)(slab * 1024), wsrc, dst);
        }
        const float* xsrc = a.x + (size_t)c * 16;                                          // 64 bytes per stage
        bool second = false;                                                               // (workgroup-uniform)
        if constexpr (SEG2) {
            second = c >= a.seg1;
            if (second) xsrc = a.x2 + (size_t)(c - a.seg1) * 16;
        }
#pragma unroll
        for (int i = 0; i < NXD; ++i) {
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base0 + (unsigned)((c % XR) * XSTG + (wave + NWAVE * i) * 1024));
            unsigned g = gx[i];
            if constexpr (SEG2) g = second ? gx2[i] : g;
            dma_fragment(g, xsrc, dst);
        }
    };
    const int fofs = (wp0 + (lane & 31)) * 64 + ((((lane >> 5) * 2) ^ ((lane >> 1) & 3)) * 16);     // + pb * 2048; second quad: ^ 16
    const int wofs = XR * XSTG + ((wn * CBW) * (WPL * 64) + lane) * 16;                                      // + slot * WBYTES + (cb * WPL + plane) * 1024
    auto frag = [&](const unsigned char* sx_, int pb, uint4 (&h)[2]) {
        const float4 q0 = *reinterpret_cast<const float4*>(sx_ + (fofs + pb * 2048));
        const float4 q1 = *reinterpret_cast<const float4*>(sx_ + ((fofs + pb * 2048) ^ 16));
        const float sc = xsc[pb];
        unsigned a_[4], b_[4];       // (split2h: 16 vector instructions per fragment instead of 24)
        split2h(q0.x, q0.y, sc, a_[0], b_[0]);
        split2h(q0.z, q0.w, sc, a_[1], b_[1]);
        split2h(q1.x, q1.y, sc, a_[2], b_[2]);
        split2h(q1.z, q1.w, sc, a_[3], b_[3]);
        h[0] = make_uint4(a_[0], a_[1], a_[2], a_[3]);
        h[1] = make_uint4(b_[0], b_[1], b_[2], b_[3]);
    };
    PP_TL_MARK(4);
    issue(0);
    if (a.nchunks > 1) issue(1);
    PP_TL_MARK(5);
    if (a.nchunks > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NXD + NWD) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    PP_TL_MARK(1);
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[cb][pb][i] = 0.f;
    for (int c = 0; c < a.nchunks; ++c) {
        const unsigned char* sxp = smem + (c % XR) * XSTG;
        const unsigned char* sw = smem + (c % WR) * WBYTES;
        uint4 wf[2][WPL], xh[2][2];
        if constexpr (WIDE) {
        // 64 x 128 wave tile: both pixel blocks are converted ONCE per workgroup (no other wave reads them) and stay live while the
        // four channel blocks pass in two pairs -- every converted fragment feeds 12 MFMAs.  Per accumulator the products of a stage
        // still arrive as g1 h0, g0 h1, g0 h0: the bits of the 128 x 64 arrangement.
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int pl = 0; pl < WPL; ++pl) wf[cb][pl] = *reinterpret_cast<const uint4*>(sw + wofs + (cb * WPL + pl) * 1024);
        frag(sxp, 0, xh[0]);
        if (c + 2 < a.nchunks) issue(c + 2);
#pragma unroll
        for (int pr = 0; pr < 2; ++pr)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                __builtin_amdgcn_sched_barrier(0);
                constexpr int WI[3] = {1, 0, 0}, XI[3] = {0, 1, 0};      // g1 h0 + g0 h1 + g0 h0
#pragma unroll
                for (int p = 0; p < 3; ++p) {
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb)
                        acc[pr * 2 + cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wf[cb][WI[p]]),
                                                                                      __builtin_bit_cast(f16x8, xh[pb][XI[p]]), acc[pr * 2 + cb][pb], 0, 0, 0);
                    // the second pair's weight fragments: plane 1 (what its first MFMAs read) as soon as this pair's last reader of
                    // that plane is issued, plane 0 behind the last MFMA -- it lands under the next block's first two
                    if (pr == 0 && pb == 1 && p != 1) {
                        if (p == 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int cb = 0; cb < 2; ++cb)
                            wf[cb][p == 0 ? 1 : 0] = *reinterpret_cast<const uint4*>(sw + wofs + ((2 + cb) * WPL + (p == 0 ? 1 : 0)) * 1024);
                        if (p == 0) __builtin_amdgcn_sched_barrier(0);      // (else the scheduler sinks these reads to the end of the block)
                    }
                }
                // the second pixel block is read and converted in the shadow of the first block's MFMAs
                if (pr == 0 && pb == 0) frag(sxp, 1, xh[1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int pl = 0; pl < WPL; ++pl) wf[cb][pl] = *reinterpret_cast<const uint4*>(sw + wofs + (cb * WPL + pl) * 1024);
        frag(sxp, 0, xh[0]);
        // stage c + 2 into the slots stage c - 1 used (every wave is past the barrier that closed it)
        if (c + 2 < a.nchunks) issue(c + 2);
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) {
            __builtin_amdgcn_sched_barrier(0);
            constexpr int WI[3] = {1, 0, 0}, XI[3] = {0, 1, 0};      // g1 h0 + g0 h1 + g0 h0
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
                    acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wf[cb][WI[p]]),
                                                                         __builtin_bit_cast(f16x8, xh[pb & 1][XI[p]]), acc[cb][pb], 0, 0, 0);
            // the next pixel block's fragment is read and converted in the shadow of these MFMAs
            if (pb < 3) frag(sxp, pb + 1, xh[(pb + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        }   // !WIDE
        // stage c + 1 has landed (younger in the queue: only what this stage requested for c + 2); every LDS read of this stage is done
        if (c + 2 < a.nchunks) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NXD + NWD) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    } else {
    // ---- loaders -------------------------------------------------------------------------------------------------------------
    unsigned goff[XS];
    int simg[H ? XS : 1];                            // fp16 form: the sample slot j belongs to (its activation scale)
#pragma unroll
    for (int j = 0; j < XS; ++j) {
        const int u = tid + NT * j;
        const long long m = m0 + (u >> 2);
        unsigned off = 0xffffffffu;
        if constexpr (H) simg[j] = 0;
        if (m < a.S) {
            const int img = (int)pp_udiv((unsigned)m, a.dv_per), rem = (int)((unsigned)m - (unsigned)img * (unsigned)(a.H * a.W));
            if constexpr (H) simg[j] = img;
            const int ho = (int)pp_udiv((unsigned)rem, a.dv_row), wo = rem - ho * a.W;
            off = (unsigned)(((img * a.xp_h + ho * a.stride) * a.xp_w + wo * a.stride) * a.Cin) * 4u + (unsigned)(u & 3) * 16u;
        }
        goff[j] = off;
    }
    const int woff0 = ((((tid & 3) >> 1) * NPp + (tid >> 2)) * 16 + (tid & 1) * 8);      // + (NT / 4) * 16 j: NT / 4 pixels further
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)a.x_bytes, 0x00020000);
    const size_t wstep = (size_t)a.ncb * (WPL * 64);
    float4 xr[XS];
    auto load_x = [&](int c) { patch_request<XS>(xrsrc, goff, (unsigned)c * 64u, xr); };
    float sx[H ? XS : 1];                            // fp16 form: activation scale of slot j's sample
    auto store_x = [&](int buf) {
        unsigned char* base = smem + buf * STAGE;
#pragma unroll
        for (int j = 0; j < XS; ++j) {
            uint2 p0, p1, p2;
            if constexpr (H) split4h(xr[j], sx[j], p0, p1);
            else split4(xr[j], p0, p1, p2);
            unsigned char* d = base + woff0 + (NT / 4) * 16 * j;
            *reinterpret_cast<uint2*>(d) = p0;
            *reinterpret_cast<uint2*>(d + XPLANE) = p1;
            if constexpr (!H) *reinterpret_cast<uint2*>(d + 2 * XPLANE) = p2;
        }
    };
    // split weights of a stage: copied verbatim global -> LDS by the DMA path (global_load_lds_dwordx4: no staging registers, no
    // ds_write); wave w moves the 1 KB fragments w, w + 8, ... of the stage's BN / 32 x 3 fragments
    constexpr int NSLAB = WU / 64;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    auto issue_w = [&](int c, int buf) {
        const uint4* src = a.w + (size_t)c * wstep + (size_t)cbB * (WPL * 64) + lane;
#pragma unroll
        for (int i = 0; i < (NSLAB + NWAVE - 1) / NWAVE; ++i) {
            const int slab = i * NWAVE + wave;
            if (NSLAB % NWAVE == 0 || slab < NSLAB)
            {
                // (raw DMA, see dma_fragment: it writes the OTHER stage; completion is awaited explicitly before the barrier below)
                const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(buf * STAGE + XBYTES + slab * 1024));
                dma_fragment(src + slab * 64, dst);
            }
        }
    };

    const int xofs = ((lane >> 5) * NPp + wm * 128 + (lane & 31)) * 16;                 // + plane * XPLANE + pb * 512
    const int wofs = XBYTES + ((wn * 2) * (WPL * 64) + lane) * 16;                      // + (cb * WPL + plane) * 1024


    // vmcnt counts in issue order: a stage issues its weight DMA first and its pixel loads (for the stage after next) after it, so
    // "all but the XS youngest" = the DMA has landed while the pixel loads keep flying across the barrier
    PP_TL_MARK(4);
    issue_w(0, 0);
    load_x(0);
    store_x(0);
    PP_TL_MARK(5);
    if (a.nchunks > 1) load_x(1);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(XS) : "memory");
    if (a.nchunks <= 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    PP_TL_MARK(1);

#pragma unroll
    for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[cb][pb][i] = 0.f;
    for (int c = 0; c < a.nchunks; ++c) {
        const unsigned char* sb = smem + (c & 1) * STAGE;
        uint4 wf[2][WPL], xf[2][XP];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int pl = 0; pl < WPL; ++pl) wf[cb][pl] = *reinterpret_cast<const uint4*>(sb + wofs + (cb * WPL + pl) * 1024);
#pragma unroll
        for (int pl = 0; pl < XP; ++pl) xf[0][pl] = *reinterpret_cast<const uint4*>(sb + xofs + pl * XPLANE);
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) {
            if (pb < 3) {
#pragma unroll
                for (int pl = 0; pl < XP; ++pl) xf[(pb + 1) & 1][pl] = *reinterpret_cast<const uint4*>(sb + xofs + pl * XPLANE + (pb + 1) * 512);
            }
            __builtin_amdgcn_sched_barrier(0);
            // the next stage's pixels (loaded during the previous stage) are split and written to the other buffer in the shadow
            // of the MFMAs; then its weights are requested (DMA) and the pixels of the stage after it -- in this order: the
            // compiler's vmcnt bookkeeping does not see the raw DMA, so nothing it waits for may be older than an in-flight DMA
            if (pb == 1 && c + 1 < a.nchunks) {
                store_x((c + 1) & 1);
                issue_w(c + 1, (c + 1) & 1);
                if (c + 2 < a.nchunks) load_x(c + 2);
            }
            if constexpr (H) {       // g1 h0 + g0 h1 + g0 h0
                constexpr int WI[3] = {1, 0, 0}, XI[3] = {0, 1, 0};
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb)
                        acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wf[cb][WI[p]]),
                                                                             __builtin_bit_cast(f16x8, xf[pb & 1][XI[p]]), acc[cb][pb], 0, 0, 0);
            } else {
            constexpr int WI[6] = {2, 1, 0, 1, 0, 0}, XI[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
                    acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf[cb][WI[p]]),
                                                                          __builtin_bit_cast(bf16x8, xf[pb & 1][XI[p]]), acc[cb][pb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (c + 2 < a.nchunks)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(XS) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    }   // !H

    PP_TL_MARK(2);
    PP_TL_MARK(6);
    // ---- epilogue, transposed through LDS (a.epi_lds) ----------------------------------------------------------------------------
    // A lane holds 4 consecutive channels of ONE pixel (lane & 31): stored from the registers, an instruction touches 32 pixels with
    // 32 bytes each.  The stages are free here (every wave passed the loop's last barrier after its last fragment read), so each
    // wave transposes its WPX pixels x 32 channels (one channel block at a time) through a region of its own ([WPX][128 B]: 16 KiB
    // of 128 pixels, WIDE: 8 KiB of 64; 16-byte chunk ^ (pixel & 7)) and stores whole 128-byte lines, 8 pixels per instruction;
    // residuals are read in the same lines.  The pixel -> (output, residual) offsets are computed once per pixel (one or two lanes'
    // worth of divisions per wave, not per store) into a table behind it (16 B per pixel).  Same arithmetic per element, in the same
    // order, as the register epilogue below: identical bits.
    if (a.epi_lds) {
        unsigned char* stg = smem + wave * (16384 + 2048);
        uint4* tab = reinterpret_cast<uint4*>(stg + 16384);
#pragma unroll
        for (int i = 0; i < WPX / 64; ++i) {
            const int p = lane + 64 * i;
            const long long m = m0 + wp0 + p;
            uint4 t = make_uint4(0u, 0u, 0u, 0u);
            if (m < a.S) {
                const int img = (int)pp_udiv((unsigned)m, a.dv_per), rem = (int)((unsigned)m - (unsigned)img * (unsigned)(a.H * a.W));
                const int oy = (int)pp_udiv((unsigned)rem, a.dv_row), ox = rem - oy * a.W;
                // (copies of decode_pos and out_pixels, here and in the register epilogue: through them the three instances change)
                t.x = (unsigned)(((size_t)img * (a.H + a.y_pad) + oy) * (a.W + a.y_pad) + ox);
                t.y = (unsigned)(((size_t)img * (a.r1_H + a.r1_pad) + (oy >> a.r1_shift)) * (a.r1_W + a.r1_pad) + (ox >> a.r1_shift));
                t.z = (unsigned)(((size_t)img * (a.H + a.r2_pad) + oy) * (a.W + a.r2_pad) + ox);
                t.w = (unsigned)img + 1u;            // 0: no such pixel
            }
            tab[p] = t;
        }
        const int rdrow = lane >> 3, rdpos = lane & 7, rdchunk = rdpos ^ rdrow;
        float xinv[H ? PBW : 1];                     // H: 1 / s of the sample of pixel pb * 32 + (lane & 31)
        if constexpr (H) {
#pragma unroll
            for (int pb = 0; pb < PBW; ++pb) xinv[pb] = pp_act_unscale(oam_first);
            if (img_first != img_last) {
#pragma unroll
                for (int pb = 0; pb < PBW; ++pb) {
                    const unsigned mp = (unsigned)min(m0 + wp0 + pb * 32 + (lane & 31), a.S - 1);
                    unsigned am = a.x_amax[pp_udiv(mp, a.dv_per)];
                    if constexpr (SEG2) am = max(am, a.x2_amax[pp_udiv(mp, a.dv_per)]);
                    xinv[pb] = pp_act_unscale(am);
                }
            }
        }
        float ymax = 0.f, ymax1 = 0.f;               // max |y| of the lane's pixels in img_first / (two samples in the wave) in img_last
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) {
#pragma unroll
            for (int pb = 0; pb < PBW; ++pb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = (cb0 + cb) * 32 + 8 * g + 4 * (lane >> 5);
                    const float4 b4 = *reinterpret_cast<const float4*>(a.bias + co);
                    const f32x16 cc = acc[cb][pb];
                    float4 v, sc = NO_R2;       // (!H: not read)
                    if constexpr (H) sc = *reinterpret_cast<const float4*>(a.wscale + co);
                    // (res1 is added behind the transposition, in whole lines)
                    epi_value<H>(v, cc[4 * g + 0], cc[4 * g + 1], cc[4 * g + 2], cc[4 * g + 3], b4, sc, xinv[H ? pb : 0], a.relu, false, NO_R2);
                    *reinterpret_cast<float4*>(stg + (pb * 32 + (lane & 31)) * 128 + (((2 * g + (lane >> 5)) ^ (lane & 7)) << 4)) = v;
                }
            // the residual lines of this channel block (16, WIDE: 8) are requested back to back (from clamped, always valid addresses) before
            // any of them is consumed: ONE memory round trip per residual and channel block instead of sixteen in a row -- round
            // 4's timeline put the epilogue of the residual layers (256 -> 1024 at 40x68) at the length of their K loop
            const int co = (cb0 + cb) * 32 + rdchunk * 4;
            const unsigned* tabw = reinterpret_cast<const unsigned*>(tab);
            // two batches of eight lines (round 5): with all sixteen in flight (64 + 64 registers beside the 64 accumulator registers of
            // the other channel block) the allocator spilled accumulator tuples -- and kept them spilled INSIDE the K loop
#pragma unroll
            for (int h8 = 0; h8 < WPX / 64; ++h8) {
            float4 vv[8];
#pragma unroll
            for (int i8 = 0; i8 < 8; ++i8) vv[i8] = *reinterpret_cast<const float4*>(stg + ((h8 * 8 + i8) * 8 + rdrow) * 128 + rdpos * 16);
            if (a.res1) {
                float4 rv[8];
#pragma unroll
                for (int i8 = 0; i8 < 8; ++i8) rv[i8] = *reinterpret_cast<const float4*>(a.res1 + (size_t)tabw[((h8 * 8 + i8) * 8 + rdrow) * 4 + 1] * a.Cout + co);
#pragma unroll
                for (int i8 = 0; i8 < 8; ++i8) add4(vv[i8], rv[i8]);
            }
            if (a.res2) {
                float4 rv[8];
#pragma unroll
                for (int i8 = 0; i8 < 8; ++i8) rv[i8] = *reinterpret_cast<const float4*>(a.res2 + (size_t)tabw[((h8 * 8 + i8) * 8 + rdrow) * 4 + 2] * a.Cout + co);
#pragma unroll
                for (int i8 = 0; i8 < 8; ++i8) add4(vv[i8], rv[i8]);
            }
#pragma unroll
            for (int i8 = 0; i8 < 8; ++i8) {
                const int it = h8 * 8 + i8;
                float4 v = vv[i8];
                epi_finish(v, a.relu, false, NO_R2);      // (both residuals were added above)
                const uint2 t = *reinterpret_cast<const uint2*>(tabw + (it * 8 + rdrow) * 4);     // .x: output pixel; then (.w via the next read)
                const unsigned tw = tabw[(it * 8 + rdrow) * 4 + 3];
                if (tw) *reinterpret_cast<float4*>(a.y + (size_t)t.x * a.Cout + co) = v;
                if (a.y_amax) {
                    const float m = tw ? pp_abs4max(v) : 0.f;
                    if (img_last - img_first <= 1) {
                        if ((int)tw - 1 == img_first) ymax = fmaxf(ymax, m);
                        else ymax1 = fmaxf(ymax1, m);
                    } else {             // several samples in the wave's pixels (the RoI head: one per pixel): per pixel, its 8 lanes reduced
                        float m8 = fmaxf(m, __shfl_xor(m, 1));
                        m8 = fmaxf(m8, __shfl_xor(m8, 2));
                        m8 = fmaxf(m8, __shfl_xor(m8, 4));
                        if (rdpos == 0 && m8 > 0.f) atomicMax(a.y_amax + (tw - 1u), __float_as_uint(m8));
                    }
                }
            }
            }
        }
        if (a.y_amax) {      // (a wave with more than two samples has issued its atomics above and passes zeros)
            const unsigned wlast = (unsigned)min(m0 + BM - 1, a.S - 1);       // (a copy of wg_samples, as below: 58 - 64 instructions fewer through it)
            const int im[2] = {img_first, img_last};
            const float ym[2] = {ymax, ymax1};
            pp_amax_commit_wg<NWAVE, 2>(a.y_amax, im, ym, (int)pp_udiv((unsigned)min(m0, (long long)wlast), a.dv_per), (int)pp_udiv(wlast, a.dv_per),
                                        reinterpret_cast<float*>(smem));
        }
        PP_TL_MARK(3);
#ifdef PP_SPLIT_TIMELINE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PP_TL_MARK(7);
#endif
        PP_TL_FLUSH();
        return;
    }

    // ---- epilogue (as conv_split_kernel) -----------------------------------------------------------------------------------------
    int rimg[PBW];
    float rmax[PBW];
#pragma unroll
    for (int pb = 0; pb < PBW; ++pb) {
        const long long mt = m0 + wp0 + pb * 32 + (lane & 31);
        const bool pok = mt < a.S;
        const long long m = pok ? mt : a.S - 1;
        const int img = (int)pp_udiv((unsigned)m, a.dv_per), rem = (int)((unsigned)m - (unsigned)img * (unsigned)(a.H * a.W));
        float xi = 1.f, ymax = 0.f;
        if constexpr (H) xi = pp_act_unscale(a.x_amax[img]);
        if constexpr (SEG2) xi = pp_act_unscale(max(a.x_amax[img], a.x2_amax[img]));
        rimg[pb] = img;
        const int oy = (int)pp_udiv((unsigned)rem, a.dv_row), ox = rem - oy * a.W;
        const size_t ypix = ((size_t)img * (a.H + a.y_pad) + oy) * (a.W + a.y_pad) + ox;
        const size_t r1pix = ((size_t)img * (a.r1_H + a.r1_pad) + (oy >> a.r1_shift)) * (a.r1_W + a.r1_pad) + (ox >> a.r1_shift);
        const size_t r2pix = ((size_t)img * (a.H + a.r2_pad) + oy) * (a.W + a.r2_pad) + ox;
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = (cb0 + cb) * 32 + 8 * g + 4 * (lane >> 5);
                if (co >= a.Cout || !pok) continue;
                const float4 b4 = *reinterpret_cast<const float4*>(a.bias + co);
                const f32x16 cc = acc[cb][pb];
                float4 v;      // (a copy of epi_value / epi_finish: through them this epilogue takes two more SGPRs and ~380 instructions)
                if constexpr (H) {
                    const float4 sc = *reinterpret_cast<const float4*>(a.wscale + co);
                    v = make_float4(__builtin_fmaf(cc[4 * g + 0], sc.x * xi, b4.x), __builtin_fmaf(cc[4 * g + 1], sc.y * xi, b4.y),
                                    __builtin_fmaf(cc[4 * g + 2], sc.z * xi, b4.z), __builtin_fmaf(cc[4 * g + 3], sc.w * xi, b4.w));
                } else {
                    v = make_float4(cc[4 * g + 0] + b4.x, cc[4 * g + 1] + b4.y, cc[4 * g + 2] + b4.z, cc[4 * g + 3] + b4.w);
                }
                if (a.relu == PP_RELU_FIRST) relu4(v);
                else if (a.relu >= PP_ACT_LEAKY) act4(v, a.relu);
                if (a.res1) {
                    const float4 r = *reinterpret_cast<const float4*>(a.res1 + r1pix * a.Cout + co);
                    add4(v, r);
                }
                if (a.res2) {
                    const float4 r = *reinterpret_cast<const float4*>(a.res2 + r2pix * a.Cout + co);
                    add4(v, r);
                }
                if (a.relu == PP_RELU_LAST) relu4(v);
                *reinterpret_cast<float4*>(a.y + ypix * a.Cout + co) = v;
                ymax = fmaxf(ymax, pp_abs4max(v));
            }
        }
        rmax[pb] = ymax;
    }
    if (a.y_amax) {
        const unsigned wlast = (unsigned)min(m0 + BM - 1, a.S - 1);
        pp_amax_commit_wg<NWAVE, PBW>(a.y_amax, rimg, rmax, (int)pp_udiv((unsigned)min(m0, (long long)wlast), a.dv_per), (int)pp_udiv(wlast, a.dv_per),
                                    reinterpret_cast<float*>(smem));
    }
}

}  // namespace

// 256 x 128 tiles, 4 waves; seg2: with a folded shortcut as the second K segment (fp16 form); fp16 form: the waves 4 x 1 with 64 x 128
// wave tiles (wide), or 2 x 2 with 128 x 64: the same bits (pp_debug_knob("split_gemm_wave_tile", ..), read by the caller)
void split_launch_gemm(bool f16, bool seg2, bool wide, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s) {
    wide = wide && f16;
    if (seg2 && wide) launch_split<conv_split_gemm_kernel<4, 1, true, true, true>, 80 * 1024>(grid, 256, lds, stream, s);
    else if (wide) launch_split<conv_split_gemm_kernel<4, 1, true, false, true>, 80 * 1024>(grid, 256, lds, stream, s);
    else if (seg2) launch_split<conv_split_gemm_kernel<2, 2, true, true>, 80 * 1024>(grid, 256, lds, stream, s);
    else if (f16) launch_split<conv_split_gemm_kernel<2, 2, true>, 80 * 1024>(grid, 256, lds, stream, s);
    else launch_split<conv_split_gemm_kernel<2, 2, false>, 80 * 1024>(grid, 256, lds, stream, s);
}
