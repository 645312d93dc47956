// Rational polyphase resampler (Kaiser-windowed sinc, zero phase) for gfx950: a file of any sample rate -> a signal at
// the rate the networks were built for.
//
// Replaces the `sr=` argument of librosa.load as reached from audio_from_file
// (/root/reference/util_audio.py:962-964), its mono=True downmix included.
//
// Definition (tests/resample_reference.py restates it in float64):
//   g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, R = max(L, M), Z = 32, beta = 10, rolloff = 0.88
//   h[k] = L (rolloff / R) sinc(rolloff k / R) I0(beta sqrt(1 - (k / (Z R))^2)) / I0(beta),  |k| <= Z R
//   y[n] = sum over m with |n M - m L| <= Z R of x[m] h[n M - m L],  x = 0 outside [0, n_in),  n < ceil(n_in L / M)
//
// Design:
//  * output n has phase p = n M mod L and centre m0 = floor(n M / L); its taps are m = m0 - A + j, j = 0 .. W - 1 with
//    A = floor(Z R / L) and W = 2 A + 2: every phase's support lies inside that range, and the table holds a zero where
//    a phase's |k| passes Z R (at most two of the W entries), so every output runs the same W steps.
//  * the table is TAP-major, coef[j][p] (row pitch L): the 64 lanes of a wave hold 64 consecutive outputs, whose phases
//    are scattered over [0, L), and at step j they all read inside ONE row of L floats (588 B at L = 147) -- a handful
//    of cache lines per load, where phase-major rows would have every lane on a line of its own.
//  * a 256-thread workgroup owns AMT_RS_TILE consecutive outputs of one signal (thread t: outputs n0 + t + 256 o).  The
//    input span they need (TILE M / L + W samples) is staged in LDS in pieces of AMT_RS_CHUNK samples: consecutive
//    threads load consecutive samples (frames of `channels` floats: one 8-byte load per lane for stereo), the mean over
//    the channels is formed there, and samples outside [0, n_in) become zeros -- the zero extension is an LDS value,
//    never a branch in the tap loop.  Every usual rate pair fits ONE piece (TILE M / L + W <= CHUNK up to M / L ~ 7.7);
//    steeper decimations walk several pieces, each output taking from a piece the taps that lie in it.
//  * each output adds its products one by one in ascending m, across pieces too, so the sum does not depend on where the
//    tile or a piece begins: a signal gives the same bits alone and inside a batch, at any base.
//  * n M and the bases are 64-bit; everything inside a piece is a 32-bit offset.  No atomics.
#include <math.h>

#include "amt_common.h"

#define AMT_RS_THREADS 256
#define AMT_RS_OPT 4                                   /* outputs per thread */
#define AMT_RS_TILE (AMT_RS_THREADS * AMT_RS_OPT)      /* outputs per workgroup */
#define AMT_RS_CHUNK 8192                              /* staged input samples: 32 KB of LDS, five workgroups per CU */
#define AMT_RS_Z 32
#define AMT_RS_RMAX 2048

struct amt_resampler {
    int sr_in, sr_out, L, M, A, W;
    float *coef_dev;          // [W][L] tap-major
};

template <int C>
__device__ __forceinline__ float rs_frame_mean(const float *__restrict__ x, long long m, int channels) {
    if constexpr (C == 1) {
        return x[m];
    } else if constexpr (C == 2) {
        // (an interleaved stereo frame is 8 bytes; the signal's base need not be 8-byte aligned, so two dword loads that
        // the lanes of a wave issue on consecutive addresses)
        const float a = x[2 * m], b = x[2 * m + 1];
        return (a + b) / 2.f;
    } else {
        const float *f = x + m * channels;
        float s = f[0];
        for (int c = 1; c < channels; ++c) s += f[c];
        return s / (float)channels;
    }
}

template <int C>
__global__ __launch_bounds__(AMT_RS_THREADS) void resample_ragged_kernel(
    const float *__restrict__ in, const int64_t *__restrict__ in_base, const int64_t *__restrict__ in_len,
    int channels, long long in_floats, float *__restrict__ out, const int64_t *__restrict__ out_base,
    long long out_floats, const float *__restrict__ coef, int L, int M, int A) {
    __shared__ float xs[AMT_RS_CHUNK];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const long long n_in = in_len[b], ib = in_base[b], ob = out_base[b];
    if (n_in <= 0) return;
    const long long n_out = (n_in * L + M - 1) / M;
    const long long n0 = (long long)blockIdx.x * AMT_RS_TILE;
    if (n0 >= n_out) return;                                        // whole workgroup: past this signal's last output
    if (ib < 0 || ib + n_in * channels > in_floats || ob < 0 || ob + n_out > out_floats) return;
    const float *x = in + ib;
    const int W = 2 * A + 2;
    const long long n_last = (n0 + AMT_RS_TILE < n_out ? n0 + AMT_RS_TILE : n_out) - 1;
    const long long m_first = n0 * M / L - A;                       // first and last input sample the tile touches
    const long long m_last = n_last * M / L + A + 1;

    long long mlo[AMT_RS_OPT];                                      // first tap m0 - A of each of the thread's outputs
    int ph[AMT_RS_OPT];
    float acc[AMT_RS_OPT];
#pragma unroll
    for (int o = 0; o < AMT_RS_OPT; ++o) {
        long long n = n0 + tid + AMT_RS_THREADS * o;
        if (n > n_last) n = n_last;                                 // (computed, not stored)
        const long long nm = n * M, m0 = nm / L;
        mlo[o] = m0 - A;
        ph[o] = (int)(nm - m0 * L);
        acc[o] = 0.f;
    }

    for (long long c0 = m_first; c0 <= m_last; c0 += AMT_RS_CHUNK) {
        const int cn = (int)(m_last + 1 - c0 < AMT_RS_CHUNK ? m_last + 1 - c0 : AMT_RS_CHUNK);
        if (c0 != m_first) __syncthreads();                         // every wave is done with the previous piece
        for (int i = tid; i < cn; i += AMT_RS_THREADS) {
            const long long m = c0 + i;
            xs[i] = (m >= 0 && m < n_in) ? rs_frame_mean<C>(x, m, channels) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int o = 0; o < AMT_RS_OPT; ++o) {
            // tap j sits at xs[d + j]; |d| is below the tile's span, TILE M / L + W < 2^22.  The taps of this piece are
            // those with 0 <= d + j < cn (an empty range where the output's taps lie wholly in other pieces)
            const int d = (int)(mlo[o] - c0);
            const int j_lo = d < 0 ? -d : 0;
            const int j_hi = cn - d < W ? cn - d : W;
            const float *co = coef + ph[o];
            float a = acc[o];
            for (int j = j_lo; j < j_hi; ++j) a += xs[d + j] * co[(size_t)j * L];
            acc[o] = a;
        }
    }
    float *y = out + ob;
#pragma unroll
    for (int o = 0; o < AMT_RS_OPT; ++o) {
        const long long n = n0 + tid + AMT_RS_THREADS * o;
        if (n <= n_last) y[n] = acc[o];
    }
}

// modified Bessel function of the first kind, order 0: sum ((x / 2)^i / i!)^2
static double rs_bessel_i0(double x) {
    double sum = 1.0, t = 1.0;
    for (int i = 1; i < 500; ++i) {
        t *= (x / 2.0) / (double)i;
        sum += t * t;
        if (t * t < 1e-20 * sum) break;
    }
    return sum;
}

static long long rs_gcd(long long a, long long b) {
    while (b) { const long long t = a % b; a = b; b = t; }
    return a;
}

extern "C" {

int amt_resampler_create(amt_resampler **rs, int sr_in, int sr_out) {
    if (!rs || sr_in <= 0 || sr_out <= 0 || sr_in == sr_out) return AMT_E_INVALID;
    const int g = (int)rs_gcd(sr_in, sr_out);
    const int L = sr_out / g, M = sr_in / g, R = L > M ? L : M;
    if (R > AMT_RS_RMAX) return AMT_E_INVALID;
    const int ZR = AMT_RS_Z * R, A = ZR / L, W = 2 * A + 2;
    const double pi = 3.14159265358979323846, beta = 10.0, rolloff = 0.88, i0b = rs_bessel_i0(beta);
    const size_t count = (size_t)W * L;
    float *h = new float[count];
    for (int j = 0; j < W; ++j)
        for (int p = 0; p < L; ++p) {
            const long long k = p + (long long)(A - j) * L;         // n M - m L at m = m0 - A + j
            double v = 0.0;
            if (k >= -ZR && k <= ZR) {
                const double t = rolloff * (double)k / (double)R, u = (double)k / (double)ZR;
                const double s = k == 0 ? 1.0 : sin(pi * t) / (pi * t);
                v = (double)L * (rolloff / (double)R) * s * rs_bessel_i0(beta * sqrt(1.0 - u * u)) / i0b;
            }
            h[(size_t)j * L + p] = (float)v;
        }
    amt_resampler *r = new amt_resampler();
    r->sr_in = sr_in; r->sr_out = sr_out; r->L = L; r->M = M; r->A = A; r->W = W; r->coef_dev = nullptr;
    hipError_t e = hipMalloc(&r->coef_dev, sizeof(float) * count);
    if (e == hipSuccess) e = hipMemcpy(r->coef_dev, h, sizeof(float) * count, hipMemcpyHostToDevice);
    delete[] h;
    if (e != hipSuccess) {
        snprintf(amt_hip_err_buf, sizeof(amt_hip_err_buf), "resampler table upload: %s", hipGetErrorString(e));
        if (r->coef_dev) (void)hipFree(r->coef_dev);
        delete r;
        return AMT_E_HIP;
    }
    *rs = r;
    return AMT_OK;
}

int amt_resampler_destroy(amt_resampler *rs) {
    if (!rs) return AMT_OK;
    if (rs->coef_dev) (void)hipFree(rs->coef_dev);
    delete rs;
    return AMT_OK;
}

long long amt_resample_length(const amt_resampler *rs, long long n_in) {
    if (!rs || n_in <= 0) return AMT_E_INVALID;
    return (n_in * rs->L + rs->M - 1) / rs->M;
}

int amt_resample_ragged(const amt_resampler *rs, const float *in, const int64_t *in_base, const int64_t *in_len,
                        int n, int channels, long long in_floats, long long max_out_len,
                        float *out, const int64_t *out_base, long long out_floats, void *stream) {
    if (!rs || !in || !in_base || !in_len || !out || !out_base || n <= 0 || n > 65535 || channels < 1 || channels > 8)
        return AMT_E_INVALID;
    if (in_floats <= 0 || out_floats <= 0 || max_out_len <= 0 || max_out_len > out_floats) return AMT_E_SHAPE;
    const long long tiles = (max_out_len + AMT_RS_TILE - 1) / AMT_RS_TILE;
    if (tiles > 0x7fffffffLL) return AMT_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)n);
#define AMT_RS_LAUNCH(C)                                                                                            \
    resample_ragged_kernel<C><<<grid, AMT_RS_THREADS, 0, st>>>(in, in_base, in_len, channels, in_floats, out, out_base, \
                                                               out_floats, rs->coef_dev, rs->L, rs->M, rs->A)
    if (channels == 1) AMT_RS_LAUNCH(1);
    else if (channels == 2) AMT_RS_LAUNCH(2);
    else AMT_RS_LAUNCH(0);
#undef AMT_RS_LAUNCH
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // extern "C"
