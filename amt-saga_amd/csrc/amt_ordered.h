// The two small launches around an ordered atomicMax (amt_common.h: float_to_ordered): every slot starts at -inf in the
// ordered encoding, and is turned back into the float's own bits once the maxima are in.  Templates, so that only a
// translation unit that launches them emits them: ordered_init_kernel<><<<...>>>(p, n).
#pragma once
#include "amt_common.h"

template <int = 0>
__global__ void ordered_init_kernel(unsigned int *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = AMT_ORDERED_NEG_INF;
}
template <int = 0>
__global__ void ordered_decode_kernel(unsigned int *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = __float_as_uint(ordered_to_float(p[i]));
}
