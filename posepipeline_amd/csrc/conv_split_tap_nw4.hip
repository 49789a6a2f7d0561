// Instances of conv_split_kernel (conv_split_tap.h): the 4-wave 3x3 / stride-1 forms with per-wave weight loads, and the product
// forms (one-tap, tap-gather).
#include "conv_split_tap.h"

void split_launch_tap_nw4(int nslot, int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s) {
    with_nslot<5, 6, 7, 8>(nslot, [&](auto ns) { launch_tap<9, 4, false, decltype(ns)::value>(cob, f16, grid, lds, stream, s); });
}

void split_launch_tap_gemm(int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s) {
    launch_tap<1, 4, false, 4>(cob, f16, grid, lds, stream, s);
}
