// Instances of conv_split_kernel (conv_split_tap.h): the 8-wave 3x3 / stride-1 forms.
#include "conv_split_tap.h"

void split_launch_tap_nw8(int nslot, int cob, bool f16, dim3 grid, size_t lds, hipStream_t stream, const SplitArgs& s) {
    with_nslot<5, 6>(nslot, [&](auto ns) { launch_tap<9, 8, false, decltype(ns)::value>(cob, f16, grid, lds, stream, s); });
}
