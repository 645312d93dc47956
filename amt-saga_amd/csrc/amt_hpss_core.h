// Harmonic/percussive separation of a magnitude spectrogram by median filtering (Fitzgerald 2010; the form people know
// as librosa.decompose.hpss): the rule, plain C++ behind one macro, so the same functions compile into the kernel of
// amt_hpss.hip and into a stand-alone CPU program (tests/hpss_host_main.cpp, built with the address and undefined-
// behaviour sanitizers).  Restated independently in tests/hpss_reference.py.  It stands in front of the transcription
// because the reference renders drum tracks into every training song (util_audio.py:843) and hands the heads pitched
// notes only (util_train_test.py:83, :159).  DESIGN.md 30.
//
// INPUT     S [T][ldf] float32, frame-major, F <= ldf live bins, finite values in [0, 2^100].  Other values give
//           unspecified results, never an access outside the arrays.  Columns F..ldf-1 are never read and are zero in
//           every output.
// KERNEL    kt, kf odd in 1..63 (1: the identity on that axis); power in {1, 2, inf}; margin_h, margin_p in [1, 100].
// REFLECT   idx(j, n) = j mod 2n (non-negative), mapped to 2n - 1 - j where that is >= n.  Periodic: an axis shorter than
//           the kernel is defined, down to n = 1.
// MEDIANS   Ht[t][f] = the (kt-1)/2-th smallest of S[idx(t + d, T)][f], d = -(kt-1)/2 .. (kt-1)/2; Pf[t][f] the same
//           along f over the F live bins with kf.  Exact: the result is an input value.
// SOFT      soft(X, R): Z = max(X, R); Z < FLT_MIN -> 0.5 when both margins are 1, else 0; otherwise a = X / Z,
//           b = R / Z, both squared when power == 2, m = a / (a + b).  Every operation single-rounded float32, in this
//           order.  mask_h = soft(Ht, Pf margin_h), mask_p = soft(Pf, Ht margin_p).
// HARD      power = inf: mask_h = (Ht >= Pf margin_h), mask_p = (Pf > Ht margin_p): a tie is harmonic, so that at margins
//           (1, 1) the masks are complementary (librosa gives a tie to neither side).
// OUTPUT    Sh = S mask_h, Sp = S mask_p; on request the rest, Sr = max((S - Sh) - Sp, 0), which is more than rounding
//           only where a margin exceeds 1.
//
// How the medians are computed.  The order of non-negative floats is the order of their uint32 images, so a window is
// sorted as integers: min / max only, no ties to break, no rounding.  The k values of a window are put into an array of
// N = 8, 32 or 64 (the size classes) between (N - 1 - k) / 2 zeros and one more of 0xFFFFFFFF, which leaves the median at
// the fixed place N / 2 - 1; Batcher's odd-even merge sort of N, generated at compile time, runs on that array with every
// index a constant (registers in the kernel), and the compiler drops the exchanges the one output read does not need.
#ifndef AMT_HPSS_CORE_H
#define AMT_HPSS_CORE_H
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <utility>

#ifdef __HIP__
#define AMT_HPSS_HD __host__ __device__ inline
#else
#define AMT_HPSS_HD inline
#endif

#define HPSS_MAX_KERNEL 63
#define HPSS_MAX_MARGIN 100.0f
#define HPSS_PAD_HI 0xFFFFFFFFu

AMT_HPSS_HD int hpss_kernel_ok(int k) { return k >= 1 && k <= HPSS_MAX_KERNEL && (k & 1); }
AMT_HPSS_HD int hpss_power_ok(float p) { return p == 1.0f || p == 2.0f || p > FLT_MAX; }   // (> FLT_MAX: +inf alone)
AMT_HPSS_HD int hpss_margin_ok(float m) { return m >= 1.0f && m <= HPSS_MAX_MARGIN; }      // (false for a NaN)
AMT_HPSS_HD int hpss_params_ok(int kt, int kf, float power, float margin_h, float margin_p) {
    return hpss_kernel_ok(kt) && hpss_kernel_ok(kf) && hpss_power_ok(power) && hpss_margin_ok(margin_h) &&
           hpss_margin_ok(margin_p);
}
// the size class of a kernel length: the array its window is sorted in
AMT_HPSS_HD int hpss_class(int k) { return k <= 7 ? 8 : (k <= 31 ? 32 : 64); }

// idx(j, n), n >= 1, any j
AMT_HPSS_HD long long hpss_reflect(long long j, long long n) {
    if (j >= 0 && j < n) return j;               // (inside the axis: no division; all of an interior tile)
    long long m = j % (2 * n);
    if (m < 0) m += 2 * n;
    return m >= n ? 2 * n - 1 - m : m;
}

AMT_HPSS_HD uint32_t hpss_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
AMT_HPSS_HD float hpss_float(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

// ---- Batcher's odd-even merge sort of N = 2^m values as a list of compare-exchanges, made at compile time ----
template <int N> struct hpss_net {
    int n;
    unsigned char a[N * 12], b[N * 12];          // (N log2 N (log2 N + 1) / 4 exchanges at the most: 672 for N = 64)
};
template <int N> constexpr hpss_net<N> hpss_make_net() {
    hpss_net<N> net{};
    for (int p = 1; p < N; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i)
                    if ((i + j) / (p * 2) == (i + j + k) / (p * 2)) {
                        net.a[net.n] = (unsigned char)(i + j);
                        net.b[net.n] = (unsigned char)(i + j + k);
                        ++net.n;
                    }
    return net;
}
template <int N> inline constexpr hpss_net<N> hpss_net_v = hpss_make_net<N>();

template <int N, int I> AMT_HPSS_HD void hpss_exchange(uint32_t (&w)[N]) {
    constexpr int a = hpss_net_v<N>.a[I], b = hpss_net_v<N>.b[I];
    static_assert(a < b && b < N, "an exchange inside the array");
    const uint32_t lo = w[a] < w[b] ? w[a] : w[b], hi = w[a] < w[b] ? w[b] : w[a];
    w[a] = lo;
    w[b] = hi;
}
template <int N, size_t... I> AMT_HPSS_HD void hpss_sort(uint32_t (&w)[N], std::index_sequence<I...>) {
    const int each[] = {(hpss_exchange<N, (int)I>(w), 0)...};
    (void)each;
}

// The median of the k values fetch(0) .. fetch(k - 1), k odd and < N, as uint32 images.
template <int N, class Fetch> AMT_HPSS_HD uint32_t hpss_median(int k, Fetch fetch) {
    uint32_t w[N];
    const int lo = (N - 1 - k) / 2;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int q = j - lo;
        w[j] = q < 0 ? 0u : (q < k ? fetch(q) : HPSS_PAD_HI);
    }
    hpss_sort<N>(w, std::make_index_sequence<(size_t)hpss_net_v<N>.n>{});
    return w[N / 2 - 1];
}

// The same median by bisection on the bit pattern, the window read again in each of 32 counting passes: the largest x
// with fewer than (k + 1) / 2 values below it.  No array, any k.  The kernel does not use it (measured 16.8 times slower
// at k = 31); the CPU program runs it as a second implementation that must give the same bytes.
template <class Fetch> AMT_HPSS_HD uint32_t hpss_median_bisect(int k, Fetch fetch) {
    const int r = (k - 1) / 2;
    uint32_t x = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t c = x | (1u << bit);
        int below = 0;
        for (int j = 0; j < k; ++j) below += fetch(j) < c;
        if (below <= r) x = c;
    }
    return x;
}

AMT_HPSS_HD float hpss_soft(float X, float R, int squared, int halves) {
    const float Z = X > R ? X : R;
    if (Z < FLT_MIN) return halves ? 0.5f : 0.0f;
    float a = X / Z, b = R / Z;
    if (squared) {
        a = a * a;
        b = b * b;
    }
    return a / (a + b);
}

AMT_HPSS_HD void hpss_masks(float Ht, float Pf, float power, float margin_h, float margin_p, float *mask_h,
                            float *mask_p) {
    const float Rh = Pf * margin_h, Rp = Ht * margin_p;
    if (power > FLT_MAX) {
        *mask_h = Ht >= Rh ? 1.0f : 0.0f;
        *mask_p = Pf > Rp ? 1.0f : 0.0f;
        return;
    }
    const int squared = power == 2.0f, halves = margin_h == 1.0f && margin_p == 1.0f;
    *mask_h = hpss_soft(Ht, Rh, squared, halves);
    *mask_p = hpss_soft(Pf, Rp, squared, halves);
}

AMT_HPSS_HD float hpss_rest(float s, float sh, float sp) {
    const float r = (s - sh) - sp;
    return r > 0.0f ? r : 0.0f;
}

#endif /* AMT_HPSS_CORE_H */
