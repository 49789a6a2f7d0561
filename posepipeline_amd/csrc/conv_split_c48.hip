// conv_split48_kernel: the 3x3 / stride-1 split kernel for 33 .. 48 output channels, and its launcher (design: conv_split.hip).
#include "conv_split_internal.h"

namespace {

// ---- 3x3 layers with 33 .. 48 output channels (HRNet-W48's first branch: 27 % of the program) -----------------------------------
// With 32-row MFMA tiles 48 output channels occupy 3/4 of two channel blocks: a quarter of the matrix work is padding.  This form
// uses v_mfma_f32_16x16x32_bf16 (same rate, 16 x 16 outputs, K = 32): THREE channel blocks of 16 -- no padding -- and K = 32 made
// of TWO TAPS x the chunk's 16 input channels, so the patch layout in LDS and its loader are unchanged: a lane's B fragment is
// pixel (lane & 15) at k half ((lane >> 4) & 1) of tap A (lanes 0 - 31) or tap B (lanes 32 - 63) -- one ds_read_b128 per plane
// at slot pixel + tap offset.  Nine taps make five pairs (the tenth half-step multiplies zero weights): per chunk and 64 pixels
// 3 x 5 x 6 x 4 = 360 MFMAs of 8 passes instead of 2 x 9 x 6 x 2 = 216 of 16: -17 % matrix-pipe time.  A wave covers 64 pixels =
// four 16-pixel sub-blocks (the halves of its two 32-pixel blocks, same lane -> pixel map), 12 accumulators of 4 registers; the
// accumulator rows of a lane are 4 CONSECUTIVE channels of its pixel: the epilogue keeps its float4 stores.
// Weights: [chunk][pair][16-channel block][plane][lane] x 16 B (split_weights48_kernel), read per wave one step ahead.
typedef __attribute__((ext_vector_type(4))) float f32x4;

// WRING (round 5, fp16 form): the split weights through a 4-slot LDS ring filled by the DMA path three pair-steps ahead (as the
// 4-wave ring form of conv_split_kernel), one barrier per pair-step.  Why: with per-wave fragment loads one step ahead a pair-step
// (36 MFMAs of 16 cycles) could not be shorter than an L2 round trip -- the 15 steps of a 48 -> 48 tile took ~15 us for ~4 us of MFMAs.
template <int NSLOT, bool H = false, bool WRING = false>
__global__ __launch_bounds__(256, 2) void conv_split48_kernel(SplitArgs a) {
    constexpr int NT = 256, NPAIR = 5, CB = 3, SB = 4;
    constexpr int XP = H ? 2 : 3;                     // activation planes (H: the fp16 form, see conv_split_kernel)
    constexpr int WPL = H ? 2 : 3;                    // weight planes
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    unsigned L = blockIdx.x, col = blockIdx.y;
    PP_TL_DECL;
    PP_TL_MARK(0);
    if (a.xcd_remap) {
        if (!xcd_tile_column(blockIdx.x, a, L, col)) return;
    }
    const int cbase = (int)col * CB;                  // first 16-channel block of this workgroup (a.ncb blocks in all)
    const int plane_bytes = 2 * a.NPp * 16;
    const int buf_bytes = XP * plane_bytes;
    int n, x0, y0;
    unsigned s0;
    tile_origin(a, L, 256u, n, x0, y0, s0);
    // ---- patch loader (as conv_split_kernel: the first loads are requested before the rest of the index arithmetic) -------------
    // (copies of the tap kernel's slot offsets and split-and-write: see conv_split_dev.h, the patch loader)
    unsigned goff[NSLOT];
    int simg[H ? NSLOT : 1];                          // fp16 form: the sample slot j belongs to (its activation scale)
    const int woff0 = ((((tid & 3) >> 1) * a.NPp + (tid >> 2)) * 16 + (tid & 1) * 8);
    if (a.mode == MODE_STREAM) {
        const int pos0 = (int)s0 - a.PWp - 1 + (tid >> 2);
        const unsigned cin4 = (unsigned)a.Cin * 4u;
        const unsigned base = (unsigned)pos0 * cin4 + (unsigned)(tid & 3) * 16u;
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) goff[j] = pos0 + (NT / 4) * j < 0 ? 0xffffffffu : base + (unsigned)((NT / 4) * j) * cin4;
        if constexpr (H) {
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
            const int pr = (int)pp_udiv((unsigned)p, a.dv_pw), pc = p - pr * a.PWp;
            const int iy = y0 - 1 + pr, ix = x0 - 1 + pc;
            if (in_patch && pc < a.TW + 2 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                off = (unsigned)(((n * a.xp_h + iy) * a.xp_w + ix) * a.Cin) * 4u;
            goff[j] = off == 0xffffffffu ? off : off + (unsigned)quad * 16u;
        }
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)a.x_bytes, 0x00020000);
    float4 xr[NSLOT];
    auto load_patch = [&](int c) { patch_request<NSLOT>(xrsrc, goff, (unsigned)c * 64u, xr); };
    const bool last_ok = (tid >> 2) + (NT / 4) * (NSLOT - 1) < a.NP;
    float sx[H ? NSLOT : 1];                          // fp16 form: activation scale of slot j's sample
    auto store_patch = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) {
            uint2 p0, p1, p2;
            if constexpr (H) split4h(xr[j], sx[j], p0, p1);
            else split4(xr[j], p0, p1, p2);
            if (j == NSLOT - 1 && !last_ok) continue;
            unsigned char* d = smem + buf * buf_bytes + woff0 + (NT / 4) * 16 * j;
            *reinterpret_cast<uint2*>(d) = p0;
            *reinterpret_cast<uint2*>(d + plane_bytes) = p1;
            if constexpr (!H) *reinterpret_cast<uint2*>(d + 2 * plane_bytes) = p2;
        }
    };
    // weights: fragment (step, block cb, plane) at ((step * ncb + cb) * 3 + plane) * 64 + lane, step = chunk * 5 + pair
    const uint4* wp = a.w + (size_t)cbase * WPL * 64 + lane;
    const size_t wstep = (size_t)a.ncb * WPL * 64;
    uint4 wf[2][CB][WPL];
    auto load_w = [&](uint4 (&dst)[CB][WPL]) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int pl = 0; pl < WPL; ++pl) dst[cb][pl] = wp[(cb * WPL + pl) * 64];
        wp += wstep;
    };
    // ring form: slot (step & 3) of the ring behind the two patch buffers holds the CB x WPL fragments of step = chunk * 5 + pair
    constexpr int WSLOT = CB * WPL * 1024, NDMA = (CB * WPL + 3) / 4;
    const int nsteps = a.nchunks * NPAIR;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wring = (unsigned)(2 * buf_bytes);
    auto issue_w = [&](int step) {
        if (step >= nsteps) return;
        // (a copy of the tap kernel's issue loop, see there)
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const int myslab = (wave + 4 * i) % (CB * WPL);      // (waves past CB * WPL copy a duplicate: same bytes, same place)
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + wring + (unsigned)((step & 3) * WSLOT + myslab * 1024));
            const uint4* g = a.w + (size_t)cbase * WPL * 64 + myslab * 64 + lane + (size_t)step * wstep;
            dma_fragment(g, dst);
        }
    };
    auto read_w = [&](int step, uint4 (&dst)[CB][WPL]) { ring_read<CB, WPL>(smem, wring, lane, step, dst); };
    auto wait_all_but = [&](int n) { ring_wait<NSLOT, NDMA, true>(n); };
    // ---- the first requests ---------------------------------------------------------------------------------------------------------
    PP_TL_MARK(4);
    if constexpr (WRING) {
        issue_w(0);
        issue_w(1);
        issue_w(2);
        load_patch(0);
    } else {
        load_patch(0);
        load_w(wf[0]);
    }
    unsigned xam[H ? NSLOT : 1];                      // (requested with the first loads, consumed behind the index arithmetic)
    if constexpr (H) {
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) xam[j] = a.x_amax[simg[j]];
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- operand addresses and output pixels: sub-block sb = 2 * (32-pixel block of the wave) + half ------------------------------
    // (the output coordinates are recomputed in the epilogue: 16 registers less across the K loop)
    const int khalf = (lane >> 4) & 1;
    auto sub_block = [&](int sb, int& aof, int& on_, int& oy_, int& ox_, bool& ok) {
        const int b = wave * 2 + (sb >> 1), r = (sb & 1) * 16 + (lane & 15);
        if (a.mode == MODE_TILE) {
            const int BW = 32 >> a.bw_log2, BH = 1 << a.bw_log2;
            int by, bx;
            block_pixel(r, a.bw_log2, by, bx);
            const int gy = b >> a.gx_log2, gx = b & ((1 << a.gx_log2) - 1);
            const int ry = gy * BH + by, rx = gx * BW + bx;
            aof = ((khalf * a.NPp) + ry * a.PWp + rx) * 16;
            on_ = n;
            oy_ = y0 + ry;
            ox_ = x0 + rx;
            ok = oy_ < a.H && ox_ < a.W;
        } else {
            const int pl = b * 32 + r;
            aof = ((khalf * a.NPp) + pl) * 16;
            const unsigned sp = s0 + (unsigned)pl;
            const bool in = sp < (unsigned)a.S;
            const unsigned sc = in ? sp : 0u;      // (a copy of decode_pos: through it one instance comes out an instruction shorter)
            const unsigned img = pp_udiv(sc, a.dv_per);
            const unsigned rem = sc - img * (unsigned)(a.xp_h * a.PWp);
            const unsigned yy = pp_udiv(rem, a.dv_row);
            on_ = (int)img;
            oy_ = (int)yy;
            ox_ = (int)(rem - yy * (unsigned)a.PWp);
            ok = in && oy_ < a.H && ox_ < a.W;
        }
    };
    int aofs[SB];            // LDS byte offset of this lane's pixel (tap (0,0), plane 0, its k half)
    unsigned oam[H ? SB : 1];                          // fp16 form: maximum of the output pixel's sample (the epilogue's 1 / s)
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
        int t0, t1, t2;
        bool t3;
        sub_block(sb, aofs[sb], t0, t1, t2, t3);
        if constexpr (H) oam[sb] = a.x_amax[t0];
    }
    // tap offset of this lane per pair: lanes 0 - 31 read tap 2 * pair, lanes 32 - 63 tap 2 * pair + 1 (pair 4: tap 8 twice, the
    // second against zero weights)
    int tofs[NPAIR];
#pragma unroll
    for (int q = 0; q < NPAIR; ++q) {
        const int t = min(2 * q + (lane >> 5), 8);
        tofs[q] = ((t / 3) * a.PWp + (t % 3)) * 16;
    }
    f32x4 acc[CB][SB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int sb = 0; sb < SB; ++sb) acc[cb][sb] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint4 xf[2][XP];         // the B fragments of sub-block sb live in set sb & 1; the next sub-block's are read during this one's MFMAs
    auto load_x = [&](const unsigned char* pbuf, int q, int sb) {
#pragma unroll
        for (int pl = 0; pl < XP; ++pl) xf[sb & 1][pl] = *reinterpret_cast<const uint4*>(pbuf + pl * plane_bytes + aofs[sb] + tofs[q]);
    };
    auto mma = [&](const uint4 (&wc)[CB][WPL], int sb) {
        if constexpr (H) {       // g1 h0 + g0 h1 + g0 h0
            constexpr int WI[3] = {1, 0, 0}, XI[3] = {0, 1, 0};
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
                    acc[cb][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wc[cb][WI[p]]),
                                                                         __builtin_bit_cast(f16x8, xf[sb & 1][XI[p]]), acc[cb][sb], 0, 0, 0);
        } else {
        constexpr int WI[6] = {2, 1, 0, 1, 0, 0}, XI[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
                acc[cb][sb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wc[cb][WI[p]]),
                                                                      __builtin_bit_cast(bf16x8, xf[sb & 1][XI[p]]), acc[cb][sb], 0, 0, 0);
        }
    };
    // ---- prologue ---------------------------------------------------------------------------------------------------------------
    if constexpr (H) {
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) sx[j] = pp_act_scale(xam[j]);
    }
    store_patch(0);              // (patch 0 and the first weights were requested above; ring form: waits, in order, for the DMAs as well)
    PP_TL_MARK(5);
    if (a.nchunks > 1) load_patch(1);
    if constexpr (WRING) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        read_w(0, wf[0]);
    } else {
        __syncthreads();
    }
    load_x(smem, 0, 0);
    // ---- K loop: 5 pair-steps per 16-channel chunk (odd: the weight register sets swap roles from chunk to chunk) -------------------
    auto chunk = [&](auto par, int c) {
        constexpr int PAR = decltype(par)::value;
        const unsigned char* pbuf = smem + (c & 1) * buf_bytes;
#pragma unroll
        for (int q = 0; q < NPAIR; ++q) {
            const int cur = (PAR + q) & 1;
            load_w(wf[cur ^ 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) {
                if (sb == SB - 1 && q == NPAIR / 2 && c + 1 < a.nchunks) store_patch((c + 1) & 1);
                // the next sub-block's fragments (of this pair, or sub-block 0 of the next pair) are requested before this one's MFMAs
                if (sb + 1 < SB) load_x(pbuf, q, sb + 1);
                else if (q + 1 < NPAIR) load_x(pbuf, q + 1, 0);
                __builtin_amdgcn_sched_barrier(0);
                mma(wf[cur], sb);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        if (c + 1 < a.nchunks) load_x(smem + ((c + 1) & 1) * buf_bytes, 0, 0);
        if (c + 2 < a.nchunks) load_patch(c + 2);
    };
    // ring form.  Order of the vector-memory operations (vmcnt is in issue order): step st issues the DMA of step st + 3 behind its first
    // sub-block -- in the middle step of a chunk (q = 2) behind the patch store instead (the compiler's wait for the staged patch must
    // not cover a younger DMA), followed by the loads of the patch after next.  The closing barrier of step st needs the DMA of st + 2
    // (issued in step st - 1) landed: younger are the DMA of st + 3 and, in steps q = 2 / 3, those patch loads.
    auto chunk_ring = [&](auto par, int c) {
        constexpr int PAR = decltype(par)::value;
        const unsigned char* pbuf = smem + (c & 1) * buf_bytes;
#pragma unroll
        for (int q = 0; q < NPAIR; ++q) {
            const int cur = (PAR + q) & 1;
            const int st = c * NPAIR + q;
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) {
                if (sb == SB - 1 && q == NPAIR / 2) {
                    if (c + 1 < a.nchunks) store_patch((c + 1) & 1);
                    issue_w(st + 3);
                    if (c + 2 < a.nchunks) load_patch(c + 2);
                }
                if (sb + 1 < SB) load_x(pbuf, q, sb + 1);
                else if (q + 1 < NPAIR) load_x(pbuf, q + 1, 0);
                __builtin_amdgcn_sched_barrier(0);
                mma(wf[cur], sb);
                __builtin_amdgcn_sched_barrier(0);
                if (sb == 0) {
                    if (st + 1 < nsteps) read_w(st + 1, wf[cur ^ 1]);
                    if (q != NPAIR / 2) issue_w(st + 3);
                }
            }
            const int younger = (st + 3 < nsteps ? NDMA : 0) + (((q == NPAIR / 2 || q == NPAIR / 2 + 1) && c + 2 < a.nchunks) ? NSLOT : 0);
            wait_all_but(younger);
            __builtin_amdgcn_s_barrier();
        }
        if (c + 1 < a.nchunks) load_x(smem + ((c + 1) & 1) * buf_bytes, 0, 0);
    };
    PP_TL_MARK(1);
    int c = 0;
    for (; c + 1 < a.nchunks; c += 2) {           // 5 steps per chunk: the register-set parity alternates per chunk
        if constexpr (WRING) {
            chunk_ring(std::integral_constant<int, 0>{}, c);
            chunk_ring(std::integral_constant<int, 1>{}, c + 1);
        } else {
            chunk(std::integral_constant<int, 0>{}, c);
            chunk(std::integral_constant<int, 1>{}, c + 1);
        }
    }
    if (c < a.nchunks) {
        if constexpr (WRING) chunk_ring(std::integral_constant<int, 0>{}, c);
        else chunk(std::integral_constant<int, 0>{}, c);
    }
    PP_TL_MARK(2);
    // ---- epilogue: accumulator register i of a lane = channel 16 cb + 4 (lane >> 4) + i of pixel (lane & 15) -------------------------
    bool cok[CB];
    int cos[CB];
    float4 b4[CB];
    float4 sc4[H ? CB : 1];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int co = (cbase + cb) * 16 + 4 * (lane >> 4);
        cok[cb] = co < a.Cout;
        cos[cb] = cok[cb] ? co : 0;
        b4[cb] = *reinterpret_cast<const float4*>(a.bias + cos[cb]);
        if constexpr (H) sc4[cb] = *reinterpret_cast<const float4*>(a.wscale + cos[cb]);
    }
    size_t ypix[SB], r1pix[SB], r2pix[SB];
    bool ook[SB];
    int onn[SB];
    float xinv[H ? SB : 1];                            // H: 1 / s of the pixel's sample
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
        int aof_, on_, oy_, ox_;
        sub_block(sb, aof_, on_, oy_, ox_, ook[sb]);
        onn[sb] = on_;
        if constexpr (H) xinv[sb] = pp_act_unscale(oam[sb]);
        out_pixels(a, ook[sb] ? on_ : 0, ook[sb] ? oy_ : 0, ook[sb] ? ox_ : 0, ypix[sb], r1pix[sb], r2pix[sb]);
    }
    float4 rv[SB][CB];
    if (a.res1) {
#pragma unroll
        for (int sb = 0; sb < SB; ++sb)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) rv[sb][cb] = *reinterpret_cast<const float4*>(a.res1 + r1pix[sb] * a.Cout + cos[cb]);
    }
#pragma unroll
    for (int sb = 0; sb < SB; ++sb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            const f32x4 cc = acc[cb][sb];
            float4 v;
            epi_value<H>(v, cc[0], cc[1], cc[2], cc[3], b4[cb], sc4[H ? cb : 0], xinv[H ? sb : 0], a.relu, a.res1 != nullptr, rv[sb][cb]);
            rv[sb][cb] = v;
        }
    PP_TL_MARK(6);
    if (a.res2) {
#pragma unroll
        for (int sb = 0; sb < SB; ++sb)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const float4 r = *reinterpret_cast<const float4*>(a.res2 + r2pix[sb] * a.Cout + cos[cb]);
                add4(rv[sb][cb], r);
            }
    }
    float ymax[SB];
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
        ymax[sb] = 0.f;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            float4 v = rv[sb][cb];
            epi_finish(v, a.relu, false, NO_R2);      // (res2 was added above, all loads in one batch)
            if (ook[sb] && cok[cb]) {
                *reinterpret_cast<float4*>(a.y + ypix[sb] * a.Cout + cos[cb]) = v;
                ymax[sb] = fmaxf(ymax[sb], pp_abs4max(v));
            }
        }
    }
    if (a.y_amax) {          // max |y| per sample of what was stored (pp_amax.h)
        int wg_first = n, wg_last = n;
        if (a.mode != MODE_TILE) wg_samples(a, s0, 256, wg_first, wg_last);
        pp_amax_commit_wg<4, SB>(a.y_amax, onn, ymax, wg_first, wg_last, reinterpret_cast<float*>(smem));
    }
    PP_TL_MARK(3);
#ifdef PP_SPLIT_TIMELINE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PP_TL_MARK(7);
#endif
    PP_TL_FLUSH();
}

}  // namespace

void split_launch_c48(int nslot, bool f16, bool ring, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s) {
    with_nslot<5, 6, 7, 8>(nslot, [&](auto ns) {
        constexpr int NS = decltype(ns)::value, L = 100 * 1024;
        if (ring) launch_split<conv_split48_kernel<NS, true, true>, L>(grid, 256, lds, stream, s);
        else if (f16) launch_split<conv_split48_kernel<NS, true, false>, L>(grid, 256, lds, stream, s);
        else launch_split<conv_split48_kernel<NS, false, false>, L>(grid, 256, lds, stream, s);
    });
}
