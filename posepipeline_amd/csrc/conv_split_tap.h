// The tap kernel conv_split_kernel (3x3 stride 1 as tile or stream, strided patch, one-tap and tap-gather products); its instances
// are compiled in conv_split_tap_*.hip, each with a launch function for its forms.
#pragma once
#include "conv_split_internal.h"

namespace {

// COB: output-channel blocks (32 channels) per wave and per workgroup; PXB: pixel blocks (32 pixels) per wave.  PXB = 1
// (128-pixel tiles, ~150 registers, three workgroups per CU) was measured for the layers whose grid does not fill the chip
// twice: 24x18 x 192 channels +9 %, 12x9 x 384 -20 %, 40x68 x 256 -17 % alone; no gain in the 4-stream program -- not instantiated.
//
// NW = 8 (512 threads, one workgroup per CU, 512-pixel tiles) is the form for layers with enough tiles: there the split weights go
// through LDS -- a 4-slot ring of per-tap fragment sets filled by the DMA path (global_load_lds_dwordx4, one 1 KB fragment per
// wave and tap), one barrier per tap.  Why: with per-wave fragment loads straight from global memory (NW = 4) every wave of a
// workgroup pulls the same 6 KB per tap through the texture-address path; an ablation build without those loads runs the
// 256 -> 256 layer at 307 instead of 228 TFLOP/s (profiles/r02_conv_split_ablation.txt), i.e. they are the largest single loss.
//
// RING4 (round 3; NW = 4, 3x3 tile / stream forms): the layers with too few chunks or tiles for the 8-wave form (all of HRNet) get
// the weights through the LDS ring, too, while keeping TWO workgroups per CU -- what made the 8-wave form lose there was one
// workgroup per CU sitting at its per-tap barrier with nothing else to run.  LDS per workgroup: the patch becomes SINGLE-buffered
// (33 - 40 KB: chunk c + 1 waits in registers, as before, and is written during the last tap of chunk c, after the barrier that
// closed tap 7 has seen every fragment read of the old patch complete) + the 4-slot ring (12 / 24 KB) = <= 73 KB, two per CU.
// Every wave copies ceil(COB * 3 / 4) fragments per tap (duplicates where 4 does not divide: the counts must be wave-uniform).
// H (round 5): the fp16 form -- TWO activation planes (h0, h1) in the patch, three weight planes (g0, g1, g2) in the same fragment
// order and ring, three products per term instead of six; the epilogue multiplies by 1 / (s c) per output channel.
// S2 (round 6; fp16 form, RING4, PXB = 1): 3x3 / STRIDE 2 / pad 1 with a strided patch.  Tap (dy, dx) of output pixel (y, x) is input
// pixel (2y + dy - 1, 2x + dx - 1): in stored coordinates r = 2y + dy, c = 2x + dx, i.e. PHASE (dy & 1, dx & 1) of the input at position
// (y + (dy >> 1), x + (dx >> 1)).  The patch of a TH x TW output tile -- (2 TH + 1) x (2 TW + 1) input pixels -- is therefore written to LDS
// DE-INTERLEAVED into its four phases, each a (TH + 1) x (TW + 1) map of pitch PWp: within one phase neighbouring output pixels are
// neighbouring slots, and the nine taps are nine offsets (phase base + shift) exactly as in the stride-1 kernel -- same fragment reads,
// same weight fragments and ring, every input element staged ONCE per channel column and no padding products (the tap-gather product
// staged every element 2.25 times; 95 - 210 TFLOP/s).  The de-interleave costs nothing at the LDS side: slot q of the patch is phase-major
// and the GLOBAL address of a slot is computed from it (neighbouring slots load pixels two apart).  128-pixel tiles (the strided patch
// of 256 would need 18 float4 of staging registers per thread): two workgroups per CU with the single-buffered patch (<= 40 KB) + ring.
template <int T, int NSLOT, int COB, int PXB = 2, int NW = 4, bool RING4 = false, bool H = false, bool S2 = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void conv_split_kernel(SplitArgs a) {
    static_assert(!S2 || (T == 9 && RING4 && H && PXB == 1), "S2 is the 4-wave fp16 ring form with one pixel block per wave");
    constexpr int NT = 64 * NW;
    constexpr int XP = H ? 2 : 3;                     // activation planes
    constexpr int WPL = H ? 2 : 3;                    // weight planes (H: g0, g1 -- the third product reuses g0)
    constexpr bool WLDS = NW == 8 || RING4;
    static_assert(!RING4 || (NW == 4 && T == 9), "RING4 is the 4-wave 3x3 form");
    static_assert(COB >= 1 && COB <= 4 && (COB <= 2 || (RING4 && H)), "three / four channel blocks per wave: the fp16 form's ring kernels only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    unsigned L = blockIdx.x, col = blockIdx.y;
    PP_TL_DECL;
    PP_TL_MARK(0);
    if (a.xcd_remap) {      // 1-D launch, see xcd_tile_column
        if (!xcd_tile_column(blockIdx.x, a, L, col)) return;
    }
    const int cb0 = (int)col * COB;
    const int plane_bytes = 2 * a.NPp * 16;           // [half][pixel] x 16 B
    const int buf_bytes = XP * plane_bytes;

    int n, x0, y0;
    unsigned s0;                                       // STREAM: first stream position, GEMM: first output pixel
    tile_origin(a, L, 32 * PXB * NW, n, x0, y0, s0);

    // ---- patch loader: slot j of this thread = (patch pixel p, channel quad) -----------------------------------------
    // Set-up order (round 4): what the FIRST LOADS need comes first and is lean -- the loads are requested before the rest of the
    // index arithmetic (fragment addresses, output coordinates), whose cost then hides behind their latency
    unsigned goff[NSLOT];
    unsigned vmask[T == 1 ? NSLOT : 1];               // GEMM with taps: bit t = tap t of this slot's pixel lies inside the image
    int simg[H ? NSLOT : 1];                          // fp16 form: the sample slot j belongs to (its activation scale)
    // LDS byte offset (plane 0) of slot j: woff0 + (NT / 4) * 16 j (NT / 4 pixels further, same quad)
    const int woff0 = ((((tid & 3) >> 1) * a.NPp + (tid >> 2)) * 16 + (tid & 1) * 8);
    if (a.mode == MODE_STREAM) {
        // position of slot j = pos0 + (NT / 4) j.  Positions before the stream (first tile only) are masked; positions past it
        // need no test: their byte offset is past the descriptor's range and reads as zero (x_bytes = the stream's size), and
        // a slot past the patch (only the last one can be) is loaded but never stored
        const int pos0 = (int)s0 - a.PWp - 1 + (tid >> 2);
        const unsigned cin4 = (unsigned)a.Cin * 4u;
        const unsigned base = (unsigned)pos0 * cin4 + (unsigned)(tid & 3) * 16u;
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) goff[j] = pos0 + (NT / 4) * j < 0 ? 0xffffffffu : base + (unsigned)((NT / 4) * j) * cin4;
        if constexpr (T == 1) {
#pragma unroll
            for (int j = 0; j < NSLOT; ++j) vmask[j] = 0;
        }
        if constexpr (H) {       // halo positions carry zeros: whichever neighbouring sample they are counted to
#pragma unroll
            for (int j = 0; j < NSLOT; ++j) {
                const int pj = pos0 + (NT / 4) * j;
                simg[j] = (int)pp_udiv((unsigned)min(max(pj, 0), (int)a.S - 1), a.dv_per);
            }
        }
    } else {
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
        const int u = tid + NT * j;
        const int p = u >> 2, quad = u & 3;
        const bool in_patch = p < a.NP;
        unsigned off = 0xffffffffu;
        if constexpr (H) simg[j] = n;
        if constexpr (S2) {
            // slot p = (phase, row, column) of the de-interleaved patch (dv_row holds the reciprocal of SP in this form)
            const int ph = (int)pp_udiv((unsigned)p, a.dv_row), r = p - ph * a.SP;
            const int qr = (int)pp_udiv((unsigned)r, a.dv_pw), qc = r - qr * a.PWp;
            const int pr = 2 * qr + (ph >> 1), pc = 2 * qc + (ph & 1);
            const int iy = 2 * y0 - 1 + pr, ix = 2 * x0 - 1 + pc;
            if (in_patch && pc <= 2 * a.TW && (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win)
                off = (unsigned)(((n * a.xp_h + iy) * a.xp_w + ix) * a.Cin) * 4u;
        } else if (a.mode == MODE_TILE) {
            const int pr = (int)pp_udiv((unsigned)p, a.dv_pw), pc = p - pr * a.PWp;
            const int iy = y0 - 1 + pr, ix = x0 - 1 + pc;
            if (in_patch && pc < a.TW + 2 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                off = (unsigned)(((n * a.xp_h + iy) * a.xp_w + ix) * a.Cin) * 4u;
        } else {
            const unsigned m = s0 + (unsigned)p;
            if constexpr (T == 1) vmask[j] = 0;
            if (in_patch && m < (unsigned)a.S) {
                // (a copy of decode_pos in int arithmetic: through the shared function most instances get another instruction order)
                const int img = (int)pp_udiv(m, a.dv_per), rem = (int)(m - (unsigned)img * (unsigned)(a.H * a.W));
                const int ho = (int)pp_udiv((unsigned)rem, a.dv_row), wo = rem - ho * a.W;
                if constexpr (H) simg[j] = img;
                if (T == 1 && a.ktaps > 1) {
                    // origin of the pixel's window (may lie before the image: the offset wraps, a valid tap's sum is exact again)
                    const int iy0 = ho * a.stride - a.pad, ix0 = wo * a.stride - a.pad;
                    off = (unsigned)(((img * a.xp_h + iy0) * a.xp_w + ix0) * a.Cin) * 4u;
                    unsigned vm = 0;
                    for (int t = 0, dy = 0, dx = 0; t < a.ktaps; ++t) {
                        if ((unsigned)(iy0 + dy) < (unsigned)a.Hin && (unsigned)(ix0 + dx) < (unsigned)a.Win) vm |= 1u << t;
                        if (++dx == a.KW) { dx = 0; ++dy; }
                    }
                    if constexpr (T == 1) vmask[j] = vm;
                    if (off == 0xffffffffu) off = 0xfffffffeu;      // (never a multiple of 16; keeps the sentinel unambiguous)
                } else {
                    off = (unsigned)(((img * a.xp_h + ho * a.stride) * a.xp_w + wo * a.stride) * a.Cin) * 4u;
                }
            }
        }
        goff[j] = off == 0xffffffffu ? off : off + (unsigned)quad * 16u;
    }
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)a.x_bytes, 0x00020000);
    float4 xr[NSLOT];
    auto load_patch = [&](int c) {
        unsigned add = (unsigned)c * 64u;
        int tbit = -1;
        if (T == 1 && a.ktaps > 1) {                  // step c = (channel chunk c / ktaps, tap c % ktaps)
            const int cc = (int)pp_udiv((unsigned)c, a.dv_ktaps), t = c - cc * a.ktaps;
            const int dy = (int)pp_udiv((unsigned)t, a.dv_kw), dx = t - dy * a.KW;
            add = (unsigned)(((dy * a.xp_w + dx) * a.Cin + 16 * cc) * 4);
            tbit = t;
        }
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) {
            bool ok = goff[j] != 0xffffffffu;
            if constexpr (T == 1) {
                if (tbit >= 0) ok = ((vmask[j] >> tbit) & 1u) != 0;
            }
            const unsigned off = ok ? goff[j] + add : 0xffffffffu;
            xr[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (int)off, 0, 0));
        }
    };
    // split + write slots [j0, j1) of the staged chunk; branch-free (it sits between MFMAs) except for the last slot, the only
    // one that can be partly outside the patch (NSLOT = ceil(NP / (NT / 4)))
    const bool last_ok = (tid >> 2) + (NT / 4) * (NSLOT - 1) < a.NP;
    // fp16 form: the activation scale of slot j's sample is a power of two: its EXPONENT byte (pp_amax_exp of the sample's maximum), four
    // slots to a register (round 6: NSLOT floats were live through the K loop), set behind the first requests
    unsigned sxe[H ? (NSLOT + 3) / 4 : 1];
    auto store_patch = [&](int buf, int j0, int j1) {
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) {
            if (j < j0 || j >= j1) continue;
            uint2 p0, p1, p2;
            if constexpr (H) split4h(xr[j], __uint_as_float((268u - ((sxe[j >> 2] >> (8 * (j & 3))) & 0xffu)) << 23), p0, p1);
            else split4(xr[j], p0, p1, p2);
            if (j == NSLOT - 1 && !last_ok) continue;
            unsigned char* d = smem + buf * buf_bytes + woff0 + (NT / 4) * 16 * j;
            *reinterpret_cast<uint2*>(d) = p0;
            *reinterpret_cast<uint2*>(d + plane_bytes) = p1;
            if constexpr (!H) *reinterpret_cast<uint2*>(d + 2 * plane_bytes) = p2;
        }
    };
    // ---- the first requests: weights of the first steps (DMA ring) / first step (registers), patch of chunk 0 -----------------
    PP_TL_MARK(4);
    constexpr int WSLOT = COB * WPL * 1024;
    constexpr int NDMA = (COB * WPL + NW - 1) / NW;  // 1 KB fragments each wave copies per step (8 waves: 1; 4 waves: 2 / 1 for COB 2 / 1)
    const unsigned wring = (unsigned)((RING4 ? 1 : 2) * buf_bytes);
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const int nsteps = a.nchunks * T;
    const size_t wstep = (size_t)a.ncb * WPL * 64;       // uint4 per step
    // step s = chunk * T + tap.  Ring slot s & 3 holds the COB x 3 fragments of step s.
    auto issue_w = [&](int step) {
        if (step >= nsteps) return;
        // (the issue loop is written out here and in conv_split48_kernel: as a function, in three forms, it changed registers and spills)
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const int myslab = (wave + NW * i) % (COB * WPL);      // (waves past COB * 3 copy a duplicate: same bytes, same place)
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + wring + (unsigned)((step & 3) * WSLOT + myslab * 1024));
            const uint4* g = a.w + (size_t)cb0 * (WPL * 64) + myslab * 64 + lane + (size_t)step * wstep;
            dma_fragment(g, dst);
        }
    };
    // weights: fragment (step, channel block cb, plane) at ((step * ncb + cb) * 3 + plane) * 64 + lane, step = chunk * T + tap
    const uint4* wlane = a.w + (size_t)cb0 * WPL * 64 + lane;
    // two register sets of weight fragments (step s + 1 is read while step s multiplies); FOUR channel blocks per wave have room for one
    // only: its fragments of step s + 1 are read behind the last MFMA of step s, in front of the closing barrier
    constexpr int WSETS = COB >= 4 ? 1 : 2;
    uint4 wf[WSETS][COB][WPL];
    uint4 xf[PXB][XP];
    const uint4* wp = wlane;                           // weights of the next step to fetch (one spare step at the end of the buffer)
    auto load_w = [&](uint4 (&dst)[COB][WPL]) {
#pragma unroll
        for (int cb = 0; cb < COB; ++cb)
#pragma unroll
            for (int pl = 0; pl < WPL; ++pl) dst[cb][pl] = wp[(cb * WPL + pl) * 64];
        wp += wstep;
    };
    if constexpr (WLDS) {
        issue_w(0);
        issue_w(1);
        issue_w(2);
        load_patch(0);
    } else {
        load_patch(0);
        load_w(wf[0]);
    }
    // fp16 form: the maxima of the slots' samples are REQUESTED here, with the first loads, and turned into scales behind the index
    // arithmetic below (consuming them here would put a full wait in front of it)
    unsigned xam[H ? NSLOT : 1];
    if constexpr (H) {
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) xam[j] = a.x_amax[simg[j]];
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- operand addresses (behind the first loads) and output pixels ------------------------------------------------------------------
    // (round 6) a lane's output pixels are needed by the EPILOGUE only: computing them here kept 8 - 10 registers alive through the K loop of
    // kernels that sit at the 256-register limit (the fp16-form 3 / 4-block kernels spilled 12 - 124 bytes per lane).  The same arithmetic
    // runs once before the loop for the LDS offsets and once after it -- from a laundered thread id, so that the compiler does not keep
    // the first evaluation -- for the coordinates.
    auto pixel_coords = [&](int lane_, int wave_, int pb, int& aofs_, int& on_, int& oy_, int& ox_, bool& ok_) {
        if (a.mode == MODE_TILE) {
            const int BW = 32 >> a.bw_log2, BH = 1 << a.bw_log2;
            int by, bx;
            block_pixel(lane_ & 31, a.bw_log2, by, bx);
            const int b = wave_ * PXB + pb;
            const int gy = b >> a.gx_log2, gx = b & ((1 << a.gx_log2) - 1);
            const int ry = gy * BH + by, rx = gx * BW + bx;
            aofs_ = (((lane_ >> 5) * a.NPp) + ry * a.PWp + rx) * 16;
            on_ = n;
            oy_ = y0 + ry;
            ox_ = x0 + rx;
            ok_ = oy_ < a.H && ox_ < a.W;
        } else {
            // STREAM: (image, row, column) of a position of the padded input stream; GEMM: of an output pixel (dv_per / dv_row hold
            // the reciprocals of the positions per image / per row of that mode)
            const unsigned per = a.mode == MODE_STREAM ? (unsigned)(a.xp_h * a.PWp) : (unsigned)(a.H * a.W);
            const unsigned row = a.mode == MODE_STREAM ? (unsigned)a.PWp : (unsigned)a.W;
            const int pl = (wave_ * PXB + pb) * 32 + (lane_ & 31);
            aofs_ = (((lane_ >> 5) * a.NPp) + pl) * 16;
            const unsigned sp = s0 + (unsigned)pl;
            const bool in = sp < (unsigned)a.S;
            decode_pos(a, in ? sp : 0u, per, row, on_, oy_, ox_);
            ok_ = in && oy_ < a.H && ox_ < a.W;
        }
    };
    int aofs[PXB];           // LDS byte offset of this lane's pixel (tap (0,0), plane 0) per pixel block
#pragma unroll
    for (int pb = 0; pb < PXB; ++pb) {
        int on_, oy_, ox_;
        bool ok_;
        pixel_coords(lane, wave, pb, aofs[pb], on_, oy_, ox_, ok_);
    }

    f32x16 acc[COB][PXB];
#pragma unroll
    for (int cb = 0; cb < COB; ++cb)
#pragma unroll
        for (int pb = 0; pb < PXB; ++pb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[cb][pb][i] = 0.f;
    if constexpr (H) {
#pragma unroll
        for (int q = 0; q < (NSLOT + 3) / 4; ++q) sxe[q] = 0;
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) sxe[j >> 2] |= pp_amax_exp(xam[j]) << (8 * (j & 3));
    }

    auto load_x = [&](const unsigned char* pbuf, int t, int pb) {
        const int dy = t / 3, dx = t % 3;
        const int toff = S2 ? ((((dy & 1) * 2 + (dx & 1)) * a.SP) + (dy >> 1) * a.PWp + (dx >> 1)) * 16 : T == 9 ? (dy * a.PWp + dx) * 16 : 0;
#pragma unroll
        for (int pl = 0; pl < XP; ++pl) xf[pb][pl] = *reinterpret_cast<const uint4*>(pbuf + pl * plane_bytes + aofs[pb] + toff);
    };

    // ---- prologue (4 waves; the 8-wave form has its own below) -------------------------------------------------------------
    if constexpr (!WLDS) {
        store_patch(0, 0, NSLOT);                      // (patch 0 and the first weights were requested above)
        PP_TL_MARK(5);
        if (a.nchunks > 1) load_patch(1);
        __syncthreads();
#pragma unroll
        for (int pb = 0; pb < PXB; ++pb) load_x(smem, 0, pb);
    }

    // the six products with i + j <= 2 (smallest terms first) of one pixel block against every channel block; consecutive MFMAs
    // go to different accumulators (no back-to-back dependency on the matrix pipe)
    auto mma = [&](const uint4 (&wc)[COB][WPL], int pb) {
        if constexpr (H) {       // g1 h0 + g0 h1 + g0 h0
            constexpr int WI[3] = {1, 0, 0}, XI[3] = {0, 1, 0};
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int cb = 0; cb < COB; ++cb)
                    acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wc[cb][WI[p]]),
                                                                         __builtin_bit_cast(f16x8, xf[pb][XI[p]]), acc[cb][pb], 0, 0, 0);
        } else {
        constexpr int WI[6] = {2, 1, 0, 1, 0, 0}, XI[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int cb = 0; cb < COB; ++cb)
                acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wc[cb][WI[p]]),
                                                                      __builtin_bit_cast(bf16x8, xf[pb][XI[p]]), acc[cb][pb], 0, 0, 0);
        }
    };

    if constexpr (WLDS) {
        // ---- 8 waves: split weights through a 4-slot LDS ring, one barrier per tap ---------------------------------------------
        // step s = chunk * T + tap.  Ring slot s & 3 holds the COB x 3 fragments of step s.  During step s: the fragments of step
        // s + 1 are read into the other register set (they landed before the barrier that ended step s - 1), the DMA of step
        // s + 3 is issued into the slot step s - 1 used, and before the closing barrier the DMA of step s + 2 is awaited -- by
        // counting: vmcnt is in issue order, so "all but the DMA of s + 3 and the patch loads issued after it" have landed.
        auto read_w = [&](int step, uint4 (&dst)[COB][WPL]) { ring_read<COB, WPL>(smem, wring, lane, step, dst); };
        // allow `n` (0, NDMA, NSLOT, NSLOT + NDMA) of the youngest vector-memory operations to stay in flight
        auto wait_all_but = [&](int n) {
            // (8-wave form, no lgkmcnt: a wave's patch writes and fragment reads are complete long before the barriers that matter
            // for them -- the patch of chunk c + 1 is written four taps before its first read, a ring slot is reused two barriers
            // after its last read was consumed.  RING4 reuses its single patch buffer at once and waits for lgkmcnt where it must.)
            ring_wait<NSLOT, NDMA, false>(n);
        };
        // (the DMAs of steps 0 - 2 and patch 0 were requested above, in this order)
        store_patch(0, 0, NSLOT);                      // waits for patch 0, hence (in order) for the three DMAs before it
        PP_TL_MARK(5);
        if (a.nchunks > 1) load_patch(1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        read_w(0, wf[0]);
#pragma unroll
        for (int pb = 0; pb < PXB; ++pb) load_x(smem, 0, pb);

        auto chunk8 = [&](auto par, int c) {
            constexpr int PAR = decltype(par)::value;
            const unsigned char* pbuf = smem + (c & 1) * buf_bytes;
            const int st0 = c * T;
            const bool more_patch = c + 1 < a.nchunks;            // patch c + 1 is staged in this chunk
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int cur = (PAR + t) & 1;
                const int st = st0 + t;
#pragma unroll
                for (int pb = 0; pb < PXB; ++pb) {
                    if (pb == PXB - 1 && t == T / 2) {
                        // patch c + 1: split and written half-way through the chunk; the DMA of this step is issued AFTER it, so
                        // that the compiler's wait for the patch loads (it does not see the DMAs) covers no DMA younger than a tap
                        if (more_patch) store_patch((c + 1) & 1, 0, NSLOT);
                        issue_w(st + 3);
                    }
                    mma(wf[cur % WSETS], pb);
                    __builtin_amdgcn_sched_barrier(0);
                    if (pb == 0) {
                        // (round 4) the next step's fragment reads and the DMA request sit BEHIND the first MFMAs of the step: straight
                        // after the barrier both waves of a SIMD are here at once, and everything issued before the first MFMA is
                        // matrix-pipe idle time.  Same-box A/B (profile_net det 64 / w48 128): 256 -> 256 at 160x272 259.9 -> 264.5
                        // TFLOP/s, 80x136 227 -> 233, 40x68 221 -> 228, HRNet 192 -> 192 179 -> 189.  Moving the BARRIER itself behind the
                        // first MFMA group as well (the group needs nothing the barrier guarantees) measured no further gain (260 vs 260):
                        // the loop runs at the chip's power limit there, a saved cycle comes back as a lower clock.
                        if (st + 1 < nsteps) read_w(st + 1, wf[(cur ^ 1) % WSETS]);
                        if (t != T / 2) issue_w(st + 3);
                    }
                    if (t + 1 < T) load_x(pbuf, t + 1, pb);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // closing barrier of the step: the DMA of step st + 2 has landed (younger: the DMA of st + 3 if there is one, and at
                // the first tap of a chunk the patch loads issued at its start); LDS writes of store_patch are complete
                {
                    const int younger = (st + 3 < nsteps ? NDMA : 0) + ((t == 0 && c + 1 < a.nchunks) ? NSLOT : 0);
                    wait_all_but(younger);
                    __builtin_amdgcn_s_barrier();
                }
            }
            if (c + 1 < a.nchunks) {
#pragma unroll
                for (int pb = 0; pb < PXB; ++pb) load_x(smem + ((c + 1) & 1) * buf_bytes, 0, pb);
            }
            if (c + 2 < a.nchunks) load_patch(c + 2);
        };
        // RING4: ONE patch buffer.  Chunk c + 1 sits in registers from the end of chunk c - 1 and is written during tap T - 1 of chunk c.
        auto chunk4 = [&](auto par, int c) {
            constexpr int PAR = decltype(par)::value;
            const int st0 = c * T;
            const bool more_patch = c + 1 < a.nchunks;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int cur = (PAR + t) & 1;
                const int st = st0 + t;
#pragma unroll
                for (int pb = 0; pb < PXB; ++pb) {
                    if (pb == 0 && t == T - 1) {
                        // every wave's fragment reads of this chunk's patch completed before the barrier that closed tap T - 2:
                        // overwrite it with chunk c + 1 (the compiler's wait for those loads must not cover a younger DMA, hence
                        // the DMA of this step after it), then request chunk c + 2
                        if (more_patch) store_patch(0, 0, NSLOT);
                        issue_w(st + 3);
                        if (c + 2 < a.nchunks) load_patch(c + 2);
                    }
                    mma(wf[cur % WSETS], pb);
                    __builtin_amdgcn_sched_barrier(0);
                    if (pb == 0) {       // behind the first MFMAs of the step, see chunk8
                        if (WSETS == 2 && st + 1 < nsteps) read_w(st + 1, wf[(cur ^ 1) % WSETS]);
                        if (t != T - 1) issue_w(st + 3);
                    }
                    if (t + 1 < T) load_x(smem, t + 1, pb);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (WSETS == 1 && st + 1 < nsteps) read_w(st + 1, wf[0]);
                {
                    // closing barrier: the DMA of step st + 2 has landed.  Younger: the DMA(s) of st + 3, and the patch loads of the
                    // next-but-one chunk where they were issued after it -- in tap T - 1 (this step) and, seen from tap 0, in the
                    // step before
                    const int younger = (st + 3 < nsteps ? NDMA : 0) +
                                        (((t == T - 1 && c + 2 < a.nchunks) || (t == 0 && c + 1 < a.nchunks)) ? NSLOT : 0);
                    wait_all_but(younger);
                    // t == T - 2: the reads of the last tap's fragments (issued above) must be complete before anyone overwrites the
                    // patch; t == T - 1: the patch writes must be complete before anyone reads the new patch
                    if (t >= T - 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                }
            }
            if (more_patch) {
#pragma unroll
                for (int pb = 0; pb < PXB; ++pb) load_x(smem, 0, pb);
            }
        };
        PP_TL_MARK(1);
        if constexpr (RING4) {
            int c4 = 0;
            for (; c4 + 1 < a.nchunks; c4 += 2) {
                chunk4(std::integral_constant<int, 0>{}, c4);
                chunk4(std::integral_constant<int, 1>{}, c4 + 1);
            }
            if (c4 < a.nchunks) chunk4(std::integral_constant<int, 0>{}, c4);
        } else {
        int c8 = 0;
        for (; c8 + 1 < a.nchunks; c8 += 2) {
            chunk8(std::integral_constant<int, 0>{}, c8);
            chunk8(std::integral_constant<int, 1>{}, c8 + 1);
        }
        if (c8 < a.nchunks) chunk8(std::integral_constant<int, 0>{}, c8);
        }   // !RING4
    } else {
    // One 16-channel chunk: T steps.  Weights of step s + 1 are requested (global -> the other register set) before the MFMAs of
    // step s; a pixel block's fragments of step s + 1 are read from LDS into the SAME registers as soon as its MFMAs of step s
    // are issued, i.e. while the other pixel block's MFMAs run.  The fences keep the compiler from sinking the loads.
    auto chunk = [&](auto par, int c) {
        constexpr int PAR = decltype(par)::value;
        const unsigned char* pbuf = smem + (c & 1) * buf_bytes;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int cur = (PAR + t) & 1;
#if !(PP_SPLIT_ABLATE & 1)
            load_w(wf[(cur ^ 1) % WSETS]);
#endif
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pb = 0; pb < PXB; ++pb) {
                // the next chunk's patch (loaded one chunk ago) is split and written half-way through the chunk.  As its own
                // (branched) region: interleaving it with the MFMAs costs ~30 registers (spills with 7-8 patch slots) and
                // measured slower -- the CU's other workgroup keeps the matrix pipe busy meanwhile
#if !(PP_SPLIT_ABLATE & 2)
                if (pb == PXB - 1 && t == T / 2 && c + 1 < a.nchunks) store_patch((c + 1) & 1, 0, NSLOT);
#endif
#if !(PP_SPLIT_ABLATE & 16)
                mma(wf[(PP_SPLIT_ABLATE & 1) ? 0 : cur % WSETS], pb);
#endif
                __builtin_amdgcn_sched_barrier(0);
#if !(PP_SPLIT_ABLATE & 8)
                if (t + 1 < T) load_x(pbuf, t + 1, pb);
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#if !(PP_SPLIT_ABLATE & 4)
        __syncthreads();
#endif
#if !(PP_SPLIT_ABLATE & 8)
        if (c + 1 < a.nchunks) {
#pragma unroll
            for (int pb = 0; pb < PXB; ++pb) load_x(smem + ((c + 1) & 1) * buf_bytes, 0, pb);
        }
#endif
#if !(PP_SPLIT_ABLATE & 2)
        if (c + 2 < a.nchunks) load_patch(c + 2);
#endif
    };
    PP_TL_MARK(1);
    int c = 0;
    for (; c + 1 < a.nchunks; c += 2) {
        chunk(std::integral_constant<int, 0>{}, c);
        chunk(std::integral_constant<int, 1>{}, c + 1);
    }
    if (c < a.nchunks) chunk(std::integral_constant<int, 0>{}, c);
    }   // !WLDS
    PP_TL_MARK(2);

    // ---- epilogue: bias, residuals, ReLU; accumulator register i of a lane = channel 8 (i / 4) + 4 (lane / 32) + i % 4 ---
    int on[PXB], oy[PXB], ox[PXB];
    bool ook[PXB];
    unsigned oam[H ? PXB : 1];                         // fp16 form: maximum of the output pixel's sample (the epilogue's 1 / s)
    {
        int tid_e = tid;
        asm volatile("" : "+v"(tid_e));                // (see pixel_coords: evaluate again instead of carrying the results through the loop)
#pragma unroll
        for (int pb = 0; pb < PXB; ++pb) {
            int aofs_;
            pixel_coords(tid_e & 63, tid_e >> 6, pb, aofs_, on[pb], oy[pb], ox[pb], ook[pb]);
        }
        if constexpr (H) {
#pragma unroll
            for (int pb = 0; pb < PXB; ++pb) oam[pb] = a.x_amax[on[pb]];
        }
    }
#if (PP_SPLIT_ABLATE & 32)
    if (a.relu != 77) {       // keep the accumulators alive with one store per lane
        if (ook[0]) a.y[(((size_t)on[0] * (a.H + a.y_pad) + oy[0]) * (a.W + a.y_pad) + ox[0]) * a.Cout + (lane >> 5)] = acc[0][0][0] + acc[COB - 1][PXB - 1][15];
        return;
    }
#endif
    // all bias / residual loads are issued back to back from clamped (always valid) addresses before anything consumes them: one
    // memory round trip per operand instead of one per (pixel block, channel group) -- the epilogue was 17 % of W48's 48-channel
    // layers (profiles/r02_conv_split_ablation.txt).  Wave tiles of three / four channel blocks (round 5) go block by block: all of
    // them at once would hold 4 x 16 x COB registers beside the accumulators (and the allocator then spills accumulator tuples).
    constexpr int CBB = COB >= 3 ? 1 : COB;            // channel blocks per epilogue batch
    size_t ypix[PXB], r1pix[PXB], r2pix[PXB];
    float xinv[H ? PXB : 1];                           // H: 1 / s of the pixel's sample
#pragma unroll
    for (int pb = 0; pb < PXB; ++pb) {
        if constexpr (H) xinv[pb] = pp_act_unscale(oam[pb]);
        if constexpr (S2) {      // (a copy of out_pixels: through it 8 of the 12 strided-patch instances get another instruction order)
            const int n_ = ook[pb] ? on[pb] : 0, y_ = ook[pb] ? oy[pb] : 0, x_ = ook[pb] ? ox[pb] : 0;
            ypix[pb] = ((size_t)n_ * (a.H + a.y_pad) + y_) * (a.W + a.y_pad) + x_;
            r1pix[pb] = ((size_t)n_ * (a.r1_H + a.r1_pad) + (y_ >> a.r1_shift)) * (a.r1_W + a.r1_pad) + (x_ >> a.r1_shift);
            r2pix[pb] = ((size_t)n_ * (a.H + a.r2_pad) + y_) * (a.W + a.r2_pad) + x_;
        } else {
            out_pixels(a, ook[pb] ? on[pb] : 0, ook[pb] ? oy[pb] : 0, ook[pb] ? ox[pb] : 0, ypix[pb], r1pix[pb], r2pix[pb]);
        }
    }
    float ymax[PXB];
#pragma unroll
    for (int pb = 0; pb < PXB; ++pb) ymax[pb] = 0.f;
#pragma unroll
    for (int cq = 0; cq < COB; cq += CBB) {
    bool cok[CBB][4];
    int cos[CBB][4];
    float4 b4[CBB][4];
    float4 sc4[H ? CBB : 1][H ? 4 : 1];                // H: 1 / (s c) of the lane's channels
#pragma unroll
    for (int cb = 0; cb < CBB; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = (cb0 + cq + cb) * 32 + 8 * g + 4 * (lane >> 5);
            cok[cb][g] = co < a.Cout;
            cos[cb][g] = cok[cb][g] ? co : 0;
            b4[cb][g] = *reinterpret_cast<const float4*>(a.bias + cos[cb][g]);
            if constexpr (H) sc4[cb][g] = *reinterpret_cast<const float4*>(a.wscale + cos[cb][g]);
        }
    float4 rv[PXB][CBB][4];
    if (a.res1) {
#pragma unroll
        for (int pb = 0; pb < PXB; ++pb)
#pragma unroll
            for (int cb = 0; cb < CBB; ++cb)
#pragma unroll
                for (int g = 0; g < 4; ++g) rv[pb][cb][g] = *reinterpret_cast<const float4*>(a.res1 + r1pix[pb] * a.Cout + cos[cb][g]);
    }
#pragma unroll
    for (int pb = 0; pb < PXB; ++pb)
#pragma unroll
        for (int cb = 0; cb < CBB; ++cb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x16 cc = acc[cq + cb][pb];
                // (a copy of epi_value: through the shared function, in three forms of it, every instance gets another instruction order)
                const float4 b = b4[cb][g];
                float4 v;
                if constexpr (H) {       // (the products with powers of two are exact: the fma rounds once, like the add)
                    const float xi = xinv[pb];
                    const float4 sc = make_float4(sc4[cb][g].x * xi, sc4[cb][g].y * xi, sc4[cb][g].z * xi, sc4[cb][g].w * xi);
                    v = make_float4(__builtin_fmaf(cc[4 * g + 0], sc.x, b.x), __builtin_fmaf(cc[4 * g + 1], sc.y, b.y),
                                    __builtin_fmaf(cc[4 * g + 2], sc.z, b.z), __builtin_fmaf(cc[4 * g + 3], sc.w, b.w));
                } else {
                    v = make_float4(cc[4 * g + 0] + b.x, cc[4 * g + 1] + b.y, cc[4 * g + 2] + b.z, cc[4 * g + 3] + b.w);
                }
                if (a.relu == PP_RELU_FIRST) relu4(v);
                else if (a.relu >= PP_ACT_LEAKY) act4(v, a.relu);
                if (a.res1) add4(v, rv[pb][cb][g]);
                rv[pb][cb][g] = v;
            }
    PP_TL_MARK(6);
    if (a.res2) {
#pragma unroll
        for (int pb = 0; pb < PXB; ++pb)
#pragma unroll
            for (int cb = 0; cb < CBB; ++cb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 r = *reinterpret_cast<const float4*>(a.res2 + r2pix[pb] * a.Cout + cos[cb][g]);
                    add4(rv[pb][cb][g], r);
                }
    }
#pragma unroll
    for (int pb = 0; pb < PXB; ++pb) {
#pragma unroll
        for (int cb = 0; cb < CBB; ++cb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 v = rv[pb][cb][g];
                epi_finish(v, a.relu, false, NO_R2);      // (res2 was added above, all loads in one batch)
                if (ook[pb] && cok[cb][g]) {
                    *reinterpret_cast<float4*>(a.y + ypix[pb] * a.Cout + cos[cb][g]) = v;
                    ymax[pb] = fmaxf(ymax[pb], pp_abs4max(v));
                }
            }
    }
    }   // channel-block batches
    if (a.y_amax) {          // the consumer is a fp16-form convolution: max |y| per sample of what was stored (pp_amax.h)
        int wg_first = n, wg_last = n;                 // samples of the workgroup's pixels
        if (a.mode != MODE_TILE) wg_samples(a, s0, 32 * PXB * NW, wg_first, wg_last);
        pp_amax_commit_wg<NW, PXB>(a.y_amax, on, ymax, wg_first, wg_last, reinterpret_cast<float*>(smem));
    }
    PP_TL_MARK(3);
#ifdef PP_SPLIT_TIMELINE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PP_TL_MARK(7);
#endif
    PP_TL_FLUSH();
}

}  // namespace

// the tap kernel conv_split_kernel<T, NS, COB, PXB, NW, RING4, H, S2> for this launch's channel blocks per wave and split form.
// The instances that exist: COB 1 / 2 with H either way, for every (T, NW, RING4) a caller names; COB 3 / 4 only with RING4 and H (the
// fp16 form's 4-wave ring kernels); S2 (the strided patch: PXB = 1, RING4) only with H, COB 1 .. 4.  Anything else falls to COB 1 / 2.
template <int T, int NW, bool R4, int NS, bool S2 = false>
static void launch_tap(int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s) {
    constexpr int L = (NW == 8 ? 160 : 100) * 1024;
    with_value<2, 3, 4, 1>(R4 || cob == 2 ? cob : 1, [&](auto cobc) {
        constexpr int COB = decltype(cobc)::value;
        with_value<1, 0>(f16 || COB >= 3 || S2, [&](auto h) {
            constexpr bool H = decltype(h)::value != 0;
            if constexpr (H ? (COB <= 2 || R4) : (COB <= 2 && !S2))
                launch_split<conv_split_kernel<T, NS, COB, S2 ? 1 : 2, NW, R4, H, S2>, L>(grid, 64 * NW, lds, stream, s);
        });
    });
}
