// Workgroup primitives of the ragged codec and scoring modules (amt_flac, amt_flacdec, amt_png, amt_pcm, amt_score):
// the one exclusive scan, the one typed wave reduction, the one length clamp.  DESIGN.md 28.
//
// INTEGER types only: a sum, a minimum or a maximum of integers is the same in any association order, so a kernel may
// move between these and a hand-written loop without changing a bit.  Floating-point reductions stay with wave_sum /
// wave_max / block_max of amt_common.h, whose order is part of their results.
#pragma once
#include "amt_common.h"

// a signal's length as every ragged kernel takes it from its table: held inside [0, max_len]
__device__ __forceinline__ long long amt_clamp_len(long long l, long long max_len) {
    return l < 0 ? 0 : (l > max_len ? max_len : l);
}

struct amt_sum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct amt_min { template <class T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };
struct amt_max { template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };

// op over the 64 lanes, the result in every lane: xor butterflies, 32 down to 1
template <class T, class Op>
__device__ __forceinline__ T amt_wave_reduce(T v, Op op) {
    static_assert(std::is_integral<T>::value, "integer reductions only: the order must not matter");
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, (T)__shfl_xor(v, off, 64));
    return v;
}

// Exclusive prefix sum of one value per thread over a workgroup of THREADS; every thread gets the workgroup's sum in
// *total.  lds: THREADS / 64 elements.  A barrier stands before lds is written (its previous use is over) and after.
template <class T, int THREADS>
__device__ __forceinline__ T amt_block_scan(T v, T *lds, T *total) {
    static_assert(std::is_integral<T>::value && THREADS % AMT_WAVE == 0, "integers, whole waves");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = (T)__shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    __syncthreads();
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < THREADS / AMT_WAVE; ++i) {
        const T t = lds[i];
        if (i < w) before += t;
        all += t;
    }
    *total = all;
    return before + incl - v;
}
