// Instances of conv_split_kernel (conv_split_tap.h): the 4-wave 3x3 / stride-1 forms with the weights through the LDS ring (RING4),
// one to four channel blocks per wave.
#include "conv_split_tap.h"

void split_launch_tap_ring4(int nslot, int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s) {
    with_nslot<5, 6, 7, 8>(nslot, [&](auto ns) { launch_tap<9, 4, true, decltype(ns)::value>(cob, f16, grid, lds, stream, s); });
}
