// Internal declarations of the split-conv translation units (conv_split*.hip): what the dispatch in conv_split.hip and the kernel
// families' launchers share.  Nothing outside those files includes this header (their public surface is in pp_internal.h).
#pragma once
#include <atomic>
#include <type_traits>

#include "conv_split_dev.h"

// conv_split_stem.hip: geometry of the stem kernel (the plan and the weight split size its fragments by it)
constexpr int STEM_TH = 16, STEM_TW = 32, STEM_PH = 2 * STEM_TH + 5, STEM_PW = 72, STEM_STEPS = 14;
constexpr int STEM_PLANE = STEM_PH * STEM_PW * 8, STEM_BUF = 2 * STEM_PLANE, STEM_WBYTES = STEM_STEPS * 2 * 2 * 1024;
constexpr int STEM_SLOTS = (STEM_PH * STEM_PW + 511) / 512;
constexpr int STEM_LDS = STEM_WBYTES + 2 * STEM_BUF + 256;

void pp_split_make_magic(unsigned d, unsigned (&dv)[2]);      // conv_split.hip
extern std::atomic<int> g_split_gemm_epi, g_split_gemm_tile;      // conv_split_gemm.hip

// launches kernel K with `lds` bytes of dynamic LDS; more than 64 KB has to be allowed per kernel, once per device (up to MAX_LDS)
template <auto K, int MAX_LDS, class Args>
static void launch_split(dim3 grid, unsigned threads, size_t lds, hipStream_t stream, const Args& s) {
    static PpPerDeviceOnce once;
    once.run([] { (void)hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS); });
    hipLaunchKernelGGL(K, grid, dim3(threads), lds, stream, s);
}

// calls f(std::integral_constant<int, NS>) for the first NS of the list with room for nslot patch slots per thread (else the last)
template <int NS, int... MORE, class F>
static void with_nslot(int nslot, F&& f) {
    if constexpr (sizeof...(MORE) == 0) f(std::integral_constant<int, NS>());
    else if (nslot <= NS) f(std::integral_constant<int, NS>());
    else with_nslot<MORE...>(nslot, f);
}

// calls f(std::integral_constant<int, V>) for the V of the list that equals v (else the last)
template <int V, int... MORE, class F>
static void with_value(int v, F&& f) {
    if constexpr (sizeof...(MORE) == 0) f(std::integral_constant<int, V>());
    else if (v == V) f(std::integral_constant<int, V>());
    else with_value<MORE...>(v, f);
}

// The kernel families' launch functions: each picks the template instance for the given form and launches it on `grid` with `lds` bytes
// of dynamic LDS.  Which form a layer takes is decided by the caller (pp_launch_conv_split); errors are read there (hipGetLastError).
// nslot: patch slots per thread; cob: 32-channel blocks per wave; f16: the fp16 form
void split_launch_tap_ring4(int nslot, int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s);   // conv_split_tap_ring4.hip
void split_launch_tap_nw4(int nslot, int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s);     // conv_split_tap_nw4.hip
void split_launch_tap_gemm(int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s);               // conv_split_tap_nw4.hip
void split_launch_tap_nw8(int nslot, int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s);     // conv_split_tap_nw8.hip
void split_launch_tap_s2p(int nslot, int cob, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s);               // conv_split_weights.hip
void split_launch_c48(int nslot, bool f16, bool ring, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s);       // conv_split_c48.hip
void split_launch_gemm(bool f16, bool seg2, bool wide, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s);                 // conv_split_gemm.hip
int split_launch_stem7(const ConvArgs& a, hipStream_t stream);                                                                    // conv_split_stem.hip
