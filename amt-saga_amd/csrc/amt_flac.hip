// FLAC encoder for gfx950: float waves on the device -> finished, compressed FLAC frame streams.
//
// Replaces the soundfile.write of audio_to_flac (util_audio.py:966-968 of the reference) for the residual and stem audio
// of a song walk, which is already on the device when it is to be written.
//
// Format (all integer, every byte defined; tests/flac_encode_reference.py restates it in numpy):
//   mono, bps in {16, 24}, fixed block size in [16, 4096], the last block of a signal shorter (>= 1 sample).
//   q = clip(rint(y 2^(bps-1)), -2^(bps-1), 2^(bps-1) - 1), NaN -> 0.
//   header: FF F8 | 70 | sample-size code << 1 | frame number, UTF-8 style | bs - 1 in 16 bits | CRC-8 (0x07).
//   one subframe, no wasted bits:
//     CONSTANT if all samples are equal; else over FIXED orders o = 0..4 (bs > o) and partition orders p = 0..8
//     (2^p | bs, (bs >> p) > o), Rice2 parameters k_j = argmin_k 5 + n_j (k + 1) + sum(u >> k) (smallest k on ties):
//     bits(o, p) = 8 + o bps + 6 + sum_j cost_j; smallest bits, smallest p, then smallest o on ties; VERBATIM unless
//     that is strictly below 8 + bs bps.
//   zero bits to the byte boundary, CRC-16 (0x8005) of the whole frame.
//   With linear prediction (amt_flac_encode_lpc_ragged; DESIGN 20, tests/flac_lpc_reference.py): after the FIXED orders
//   the LPC orders m = 1..L (bs > m) of amt_flac_lpc_core.h join the same choice -- type byte (32 + m - 1) << 1, m
//   warm-up samples, 4 bits P - 1, 5 bits shift, m coefficients of P bits, the same residual coding;
//     bits(m, p) = 8 + m bps + 4 + 5 + m P + 6 + sum_j cost_j.  A candidate replaces the best so far only if strictly
//   smaller, so FIXED wins a tie against LPC and the smaller order wins; |r| >= 2^27 disqualifies an LPC order.
//
// Design:
//  * frame kernel: one 256-thread workgroup per frame, grid (frames of the longest signal, signals).  Thread t owns at
//    most 16 consecutive samples, laid out so that the partitions of level p are the groups of 256 >> p consecutive
//    threads, for every block size: with P = 2^min(8, ctz(bs)) finest partitions, 256 / P threads share one.
//  * u < 2^28 (a fourth difference of 24-bit samples), so k > 28 costs strictly more than k = 28 and only k = 0..28
//    are evaluated; 16 values of u fit 32 bits, every longer sum is 64-bit.
//  * per order, a thread sums u >> k over its samples, and the sums are merged upward by addition: xor-butterflies
//    inside a wave (group sizes 2 .. 64), LDS across the four waves (128, 256).  After step lg every thread holds the
//    sums of its level-(8 - lg) partition; the first thread of each partition records the best k and adds the
//    partition's cost to the level's total.
//  * the bit stream is assembled in a zeroed LDS buffer with atomicOr on 32-bit words, MSB first: the unary zeros are
//    free, a code is its stop bit and k low bits, at most 29 bits in one or two words.  Positions come from a
//    block-wide prefix sum of the code lengths.
//  * CRC-16: the frame is taken as 256 equal chunks (zero bytes in front change nothing with a zero initial value),
//    every thread walks one chunk with a byte table, and the chunk values are combined pairwise: crc(A | B) =
//    crc(A) x^(8 |B|) + crc(B) modulo the polynomial, eight levels with the multiplier squared at each.
//  * offsets: one workgroup per signal scans its frame sizes; one workgroup scans the signals' totals.
//  * compaction: one workgroup per frame copies slot -> byte offset, byte-granular.
//  * MD5: one wave per signal; the lanes build the message words from the same quantiser, the rounds run on LDS words.
//  * LPC (the kernel's second instantiation): the windowed block goes to LDS, every thread sums its samples' products
//    for the 13 lags in int64, the sums are added over the wave and the four waves (exact: any order), thread 0 runs the
//    float64 recurrence and the quantiser of amt_flac_lpc_core.h for all orders into LDS, and every order then goes
//    through the cost search of the fixed orders with its residuals computed from q and its coefficients in LDS.
//  * no workgroup waits for another; the kernels are ordered by the stream alone.  No global atomics.
#include <math.h>

#include "amt_common.h"
#include "amt_flac_common.h"
#include "amt_flac_lpc_core.h"
#include "amt_scratch.h"
#include "amt_wg.h"

#define AMT_FL_THREADS 256
#define AMT_FL_MAXBS 4096
#define AMT_FL_KN 29                                            /* k = 0 .. 28 */
#define AMT_FL_CAND (5 + FLL_MAX_ORDER)                           /* FIXED 0 .. 4, then LPC 1 .. 12 */
#define AMT_FL_WORDS ((13 + (8 + AMT_FL_MAXBS * 24 + 7) / 8 + 2 + 3) / 4 + 2)

typedef unsigned long long fl_u64;

static __host__ __device__ inline long long fl_bound(int blocksize, int bps) {
    return 13 + (8 + (long long)blocksize * bps + 7) / 8 + 2;
}

// the one quantiser of the frame and the MD5 kernel
__device__ __forceinline__ int fl_quant(float y, int bps) {
    const int lim = 1 << (bps - 1);
    const float r = rintf(y * (float)lim);
    if (!(r == r)) return 0;
    if (r >= (float)lim) return lim - 1;
    if (r < -(float)lim) return -lim;
    return (int)r;
}

__device__ __forceinline__ int fl_resid(const int *q, int i, int o) {
    switch (o) {
        case 0: return q[i];
        case 1: return q[i] - q[i - 1];
        case 2: return q[i] - 2 * q[i - 1] + q[i - 2];
        case 3: return q[i] - 3 * q[i - 1] + 3 * q[i - 2] - q[i - 3];
        default: return q[i] - 4 * q[i - 1] + 6 * q[i - 2] - 4 * q[i - 3] + q[i - 4];
    }
}

__device__ __forceinline__ unsigned fl_zig(int r) { return ((unsigned)r << 1) ^ (unsigned)(r >> 31); }

// The residual of sample i under one predictor, as the cost search and the emit phase take it.  `bad` is raised where
// the candidate is disqualified (LPC: |r| >= 2^27); the fixed predictors never raise it.
struct fl_fixed_resid {
    const int *q;
    int o;
    __device__ __forceinline__ int operator()(int i, int &bad) const { return fl_resid(q, i, o); }
};

struct fl_lpc_resid {
    const int *q, *c;
    int m, shift;
    __device__ __forceinline__ int operator()(int i, int &bad) const {
        const fll_i64 r = fll_resid(q, i, c, m, shift);
        bad |= !fll_resid_ok(r);
        return (int)r;
    }
};

// n bits (1 .. 32) of v (< 2^n) at bit `pos` of the zeroed big-endian word buffer of AMT_FL_WORDS words
__device__ __forceinline__ void fl_put(unsigned *buf, unsigned pos, int n, unsigned v) {
    const unsigned w = pos >> 5;
    const int room = 32 - (int)(pos & 31);
    if (w + 1 >= AMT_FL_WORDS) return;                            // (never: a chosen form is shorter than VERBATIM)
    if (n <= room) {
        atomicOr(&buf[w], v << (room - n));
    } else {
        const int lo = n - room;
        atomicOr(&buf[w], v >> lo);
        atomicOr(&buf[w + 1], v << (32 - lo));
    }
}

__device__ __forceinline__ unsigned fl_byte(const unsigned *buf, int i) { return (buf[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu; }

// The cost search of one predictor of order o over the block: the thread's sums of u >> k over its samples [i0, i1),
// the butterflies, the best k of every partition of every level into kbest_o, the level totals.  Returns the smallest
// head_bits + sum of the partition costs over the partition orders, *best_p its p (the smallest of a tie); *bad is
// raised in the threads whose residuals disqualify the predictor.  Ends with a barrier: wsum and red are free again.
template <class Resid>
__device__ __forceinline__ fl_u64 fl_cost_search(const Resid &resid, int o, fl_u64 head_bits, int bs, int pmax, int i0,
                                                 int i1, fl_u64 (*wsum)[AMT_FL_KN], fl_u64 (*red)[9],
                                                 unsigned char *kbest_o, int *best_p, int *bad) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned s32[AMT_FL_KN];
#pragma unroll
    for (int k = 0; k < AMT_FL_KN; ++k) s32[k] = 0u;
    for (int i = max(i0, o); i < i1; ++i) {
        const unsigned u = fl_zig(resid(i, *bad));
#pragma unroll
        for (int k = 0; k < AMT_FL_KN; ++k) s32[k] += u >> k;
    }
    fl_u64 s[AMT_FL_KN];
#pragma unroll
    for (int k = 0; k < AMT_FL_KN; ++k) s[k] = s32[k];
    fl_u64 c[9];
#pragma unroll
    for (int lg = 0; lg <= 8; ++lg) {
        const int p = 8 - lg;
        if (lg >= 1 && lg <= 6) {
#pragma unroll
            for (int k = 0; k < AMT_FL_KN; ++k) s[k] += __shfl_xor(s[k], 1 << (lg - 1), 64);
        } else if (lg == 7) {
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < AMT_FL_KN; ++k) wsum[w][k] = s[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < AMT_FL_KN; ++k) s[k] += wsum[w ^ 1][k];
        } else if (lg == 8) {
#pragma unroll
            for (int k = 0; k < AMT_FL_KN; ++k) s[k] += wsum[w ^ 2][k] + wsum[w ^ 3][k];
        }
        c[lg] = 0;
        if (p <= pmax && (bs >> p) > o) {                         // block-uniform
            const fl_u64 n = (fl_u64)((bs >> p) - (tid < (1 << lg) ? o : 0));
            fl_u64 bc = 5 + n + s[0];
            int bk = 0;
#pragma unroll
            for (int k = 1; k < AMT_FL_KN; ++k) {
                const fl_u64 v = 5 + n * (fl_u64)(k + 1) + s[k];
                if (v < bc) { bc = v; bk = k; }
            }
            if ((tid & ((1 << lg) - 1)) == 0) {
                kbest_o[(1 << p) - 1 + (tid >> lg)] = (unsigned char)bk;
                c[lg] = bc;
            }
        }
    }
    // totals of the nine levels over the block
#pragma unroll
    for (int lg = 0; lg <= 8; ++lg) {
        c[lg] = amt_wave_reduce(c[lg], amt_sum{});
        if (lane == 0) red[w][lg] = c[lg];
    }
    __syncthreads();
    fl_u64 ob = ~0ull;
    int op = 0;
#pragma unroll
    for (int lg = 0; lg <= 8; ++lg) {                             // p descending: <= keeps the smallest p of a tie
        const int p = 8 - lg;
        if (p <= pmax && (bs >> p) > o) {
            const fl_u64 t = head_bits + red[0][lg] + red[1][lg] + red[2][lg] + red[3][lg];
            if (t <= ob) { ob = t; op = p; }
        }
    }
    *best_p = op;
    __syncthreads();                                              // wsum / red are free for the next predictor
    return ob;
}

// The residual codes of the chosen predictor of order o, partition order 8 - lg, from bit `at` of the frame: per
// partition the 5-bit parameter (its leader thread), per sample the unary zeros, the stop bit and the k low bits.
template <class Resid>
__device__ __forceinline__ void fl_emit_codes(const Resid &resid, int o, int i0, int i1, int lg, int k, unsigned at,
                                              unsigned *bits, fl_u64 *scan_lds) {
    const int tid = threadIdx.x;
    const bool leader = (tid & ((1 << lg) - 1)) == 0;
    int bad = 0;
    unsigned mine = leader ? 5u : 0u;
    for (int i = max(i0, o); i < i1; ++i) mine += (fl_zig(resid(i, bad)) >> k) + 1u + k;
    fl_u64 total;
    unsigned pos = at + (unsigned)amt_block_scan<fl_u64, AMT_FL_THREADS>(mine, scan_lds, &total);
    if (leader) { fl_put(bits, pos, 5, (unsigned)k); pos += 5; }
    for (int i = max(i0, o); i < i1; ++i) {
        const unsigned u = fl_zig(resid(i, bad));
        pos += u >> k;
        fl_put(bits, pos, 1 + k, (1u << k) | (u & ((1u << k) - 1u)));
        pos += 1 + k;
    }
}

// LPC = false: the fixed predictors alone (amt_flac_encode_ragged; lpc_order is not read).  LPC = true: the LPC orders
// 1 .. lpc_order as well.
template <bool LPC>
__global__ __launch_bounds__(AMT_FL_THREADS) void flac_frame_kernel(
    const float *__restrict__ wave, const long long *__restrict__ base, const long long *__restrict__ len,
    long long max_len, int blocksize, int bps, long long first_frame, long long frames_max,
    unsigned char *__restrict__ scratch, long long bound, long long *__restrict__ frame_bytes, int lpc_order) {
    __shared__ int q[AMT_FL_MAXBS];
    __shared__ unsigned bits[AMT_FL_WORDS];
    __shared__ fl_u64 wsum[4][AMT_FL_KN];
    __shared__ fl_u64 red[4][9];
    __shared__ fl_u64 scan_lds[4];
    __shared__ unsigned char kbest[LPC ? AMT_FL_CAND : 5][512];
    __shared__ unsigned crc_s[AMT_FL_THREADS];
    __shared__ unsigned short crctab[256];
    // LPC only (never referenced, so not allocated, in the fixed instantiation)
    __shared__ int xw[LPC ? AMT_FL_MAXBS : 1];                    // the windowed block
    __shared__ fll_i64 acorr[4][FLL_LAGS];                        // per wave, then [0]: the block's autocorrelation
    __shared__ double lpc_work[FLL_WORK];
    __shared__ int lpc_coef[FLL_MAX_ORDER * FLL_MAX_ORDER];
    __shared__ int lpc_shift[FLL_MAX_ORDER];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y;
    const long long f = blockIdx.x;
    const long long n_s = amt_clamp_len(len[b], max_len);
    const long long nframes = (n_s + blocksize - 1) / blocksize;
    const long long slot = (long long)b * frames_max + f;
    if (f >= nframes) {                                           // past this signal's last frame
        if (tid == 0) frame_bytes[slot] = 0;
        return;
    }
    const long long s0 = f * blocksize;
    const int bs = (int)(n_s - s0 < blocksize ? n_s - s0 : blocksize);
    const float *x = wave + base[b] + s0;
    const unsigned mask = (1u << bps) - 1u;

    for (int i = tid; i < bs; i += AMT_FL_THREADS) q[i] = fl_quant(x[i], bps);
    for (int i = tid; i < AMT_FL_WORDS; i += AMT_FL_THREADS) bits[i] = 0u;
    crctab[tid] = fl_crc16_entry((unsigned)tid);
    __syncthreads();

    int same = 1;
    for (int i = tid; i < bs; i += AMT_FL_THREADS) same &= (q[i] == q[0]);
    const int constant = __syncthreads_and(same);

    // the thread's samples [i0, i1): at most 16, inside one finest partition
    const int pmax = min(8, __ffs(bs) - 1);
    const int plen = bs >> pmax, tpp = AMT_FL_THREADS >> pmax;
    const int chunk = (plen + tpp - 1) / tpp;
    int i0 = (tid >> (8 - pmax)) * plen + (tid & (tpp - 1)) * chunk;
    int i1 = min(i0 + chunk, ((tid >> (8 - pmax)) + 1) * plen);
    if (i1 < i0) i1 = i0;

    fl_u64 best_bits = ~0ull;
    int best_o = 0, best_p = 0;
    if (!constant) {
        for (int o = 0; o < 5 && bs > o; ++o) {
            int op, bad = 0;
            const fl_u64 ob = fl_cost_search(fl_fixed_resid{q, o}, o, 8 + (fl_u64)(o * bps) + 6, bs, pmax, i0, i1, wsum,
                                             red, kbest[o], &op, &bad);
            if (ob < best_bits) { best_bits = ob; best_o = o; best_p = op; }
        }
        if constexpr (LPC) {
            // autocorrelation of the windowed block: exact int64 sums, so the order of the additions is free
            for (int i = i0; i < i1; ++i) xw[i] = fll_windowed(q[i], i, bs);
            __syncthreads();
            fll_i64 acc[FLL_LAGS];
#pragma unroll
            for (int l = 0; l < FLL_LAGS; ++l) acc[l] = 0;
            for (int i = i0; i < i1; ++i) {
                const fll_i64 xi = xw[i];
#pragma unroll
                for (int l = 0; l < FLL_LAGS; ++l)
                    if (i >= l) acc[l] += xi * xw[i - l];
            }
#pragma unroll
            for (int l = 0; l < FLL_LAGS; ++l) {
                acc[l] = amt_wave_reduce(acc[l], amt_sum{});
                if (lane == 0) acorr[w][l] = acc[l];
            }
            __syncthreads();
            const int orders = min(lpc_order, bs - 1);
            if (tid == 0) {                                       // one lane: the recurrence is sequential
                for (int l = 0; l < FLL_LAGS; ++l) acorr[0][l] += acorr[1][l] + acorr[2][l] + acorr[3][l];
                fll_analyse(acorr[0], orders, fll_precision(bps), lpc_work, lpc_coef, lpc_shift);
            }
            __syncthreads();
            for (int m = 1; m <= orders; ++m) {
                const int sh = lpc_shift[m - 1];                  // block-uniform
                if (sh < 0) continue;
                int op, bad = 0;
                const fl_lpc_resid rs{q, lpc_coef + (m - 1) * FLL_MAX_ORDER, m, sh};
                const fl_u64 head = 8 + (fl_u64)(m * bps) + 4 + 5 + (fl_u64)(m * fll_precision(bps)) + 6;
                const fl_u64 ob = fl_cost_search(rs, m, head, bs, pmax, i0, i1, wsum, red, kbest[4 + m], &op, &bad);
                if (__syncthreads_or(bad)) continue;              // some |r| >= 2^27: no candidate
                if (ob < best_bits) { best_bits = ob; best_o = 4 + m; best_p = op; }
            }
        }
    }

    // ---- header (thread 0), its length (every thread) ----
    const fl_u64 fn = (fl_u64)(first_frame + f);
    const int nb = fn < 0x80 ? 1 : fn < 0x800 ? 2 : fn < 0x10000 ? 3 : fn < 0x200000 ? 4 : fn < 0x4000000 ? 5 : 6;
    const int hb = 4 + nb + 2 + 1;
    if (tid == 0) {
        unsigned crc = 0;
        int at = 0;
        auto emit = [&](unsigned byte) {
            fl_put(bits, (unsigned)(8 * at), 8, byte);
            crc = fl_crc8_step(crc, byte);
            ++at;
        };
        emit(0xFF); emit(0xF8); emit(0x70); emit(bps == 16 ? 0x08 : 0x0C);
        if (nb == 1) {
            emit((unsigned)fn);
        } else {
            emit(((0xFFu << (8 - nb)) & 0xFFu) | (unsigned)(fn >> (6 * (nb - 1))));
            for (int i = nb - 2; i >= 0; --i) emit(0x80u | (unsigned)((fn >> (6 * i)) & 0x3F));
        }
        emit((unsigned)(bs - 1) >> 8);
        emit((unsigned)(bs - 1) & 0xFFu);
        fl_put(bits, (unsigned)(8 * at), 8, crc);
    }

    // ---- subframe ----
    const unsigned sp = 8u * hb;
    const fl_u64 verbatim_bits = 8 + (fl_u64)bs * bps;
    fl_u64 body_bits;
    if (constant) {
        body_bits = 8 + bps;
        if (tid == 0) fl_put(bits, sp + 8, bps, (unsigned)q[0] & mask);
    } else if (best_bits < verbatim_bits) {
        body_bits = best_bits;
        const int p = best_p, lg = 8 - p;
        const int k = kbest[best_o][(1 << p) - 1 + (tid >> lg)];
        if (!LPC || best_o < 5) {
            const int o = best_o;
            if (tid == 0) {
                fl_put(bits, sp, 8, (unsigned)(8 + o) << 1);
                for (int i = 0; i < o; ++i) fl_put(bits, sp + 8 + i * bps, bps, (unsigned)q[i] & mask);
                fl_put(bits, sp + 8 + o * bps, 6, 0x10u | (unsigned)p);
            }
            fl_emit_codes(fl_fixed_resid{q, o}, o, i0, i1, lg, k, sp + 8 + o * bps + 6, bits, scan_lds);
        } else if constexpr (LPC) {
            const int m = best_o - 4, prec = fll_precision(bps), sh = lpc_shift[m - 1];
            const int *cf = lpc_coef + (m - 1) * FLL_MAX_ORDER;
            const unsigned at = sp + 8 + m * bps + 4 + 5 + m * prec;
            if (tid == 0) {
                fl_put(bits, sp, 8, (unsigned)(32 + m - 1) << 1);
                for (int i = 0; i < m; ++i) fl_put(bits, sp + 8 + i * bps, bps, (unsigned)q[i] & mask);
                fl_put(bits, sp + 8 + m * bps, 4, (unsigned)(prec - 1));
                fl_put(bits, sp + 8 + m * bps + 4, 5, (unsigned)sh);
                for (int j = 0; j < m; ++j) fl_put(bits, sp + 8 + m * bps + 9 + j * prec, prec, (unsigned)cf[j] & ((1u << prec) - 1u));
                fl_put(bits, at, 6, 0x10u | (unsigned)p);
            }
            fl_emit_codes(fl_lpc_resid{q, cf, m, sh}, m, i0, i1, lg, k, at + 6, bits, scan_lds);
        }
    } else {
        body_bits = verbatim_bits;
        if (tid == 0) fl_put(bits, sp, 8, 0x02u);
        for (int i = tid; i < bs; i += AMT_FL_THREADS) fl_put(bits, sp + 8 + i * bps, bps, (unsigned)q[i] & mask);
    }
    const int ncrc = hb + (int)((body_bits + 7) >> 3);            // bytes the CRC-16 covers
    const int fsize = ncrc + 2;
    __syncthreads();

    // ---- CRC-16 ----
    {
        const int lc = (ncrc + AMT_FL_THREADS - 1) / AMT_FL_THREADS;
        const int pad = AMT_FL_THREADS * lc - ncrc;
        unsigned crc = 0, m = 1;
        for (int j = 0; j < lc; ++j) {
            const int idx = tid * lc + j - pad;
            if (idx >= 0) crc = ((crc << 8) & 0xffffu) ^ crctab[((crc >> 8) ^ fl_byte(bits, idx)) & 0xffu];
            m = ((m << 8) & 0xffffu) ^ crctab[(m >> 8) & 0xffu];  // x^(8 lc)
        }
        crc_s[tid] = crc;
        for (int st = 1; st < AMT_FL_THREADS; st <<= 1) {
            __syncthreads();
            if ((tid & (2 * st - 1)) == 2 * st - 1) crc_s[tid] = fl_mulmod16(crc_s[tid - st], m) ^ crc_s[tid];
            m = fl_mulmod16(m, m);
        }
        __syncthreads();
        if (tid == 0) fl_put(bits, 8u * ncrc, 16, crc_s[AMT_FL_THREADS - 1]);
        __syncthreads();
    }

    unsigned char *dst = scratch + slot * bound;
    for (int i = tid; i < fsize; i += AMT_FL_THREADS) dst[i] = (unsigned char)fl_byte(bits, i);
    if (tid == 0) frame_bytes[slot] = fsize;
}

// per signal: exclusive scan of its frame sizes -> frame_off, total -> stream_off[b + 1], min / max frame size
__global__ __launch_bounds__(AMT_FL_THREADS) void flac_frame_offsets_kernel(
    const long long *__restrict__ len, long long max_len, int blocksize, long long frames_max,
    const long long *__restrict__ frame_bytes, long long *__restrict__ frame_off, long long *__restrict__ stream_off,
    int *__restrict__ frame_minmax) {
    __shared__ fl_u64 lds[4];
    __shared__ int mm[2][4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const long long n_s = amt_clamp_len(len[b], max_len);
    const long long nframes = (n_s + blocksize - 1) / blocksize;
    fl_u64 carry = 0;
    int mn = 0x7fffffff, mx = 0;
    for (long long f0 = 0; f0 < nframes; f0 += AMT_FL_THREADS) {
        const long long f = f0 + tid;
        const long long v = f < nframes ? frame_bytes[(long long)b * frames_max + f] : 0;
        fl_u64 total;
        const fl_u64 ex = amt_block_scan<fl_u64, AMT_FL_THREADS>((fl_u64)v, lds, &total);
        if (f < nframes) {
            frame_off[(long long)b * frames_max + f] = (long long)(carry + ex);
            mn = min(mn, (int)v);
            mx = max(mx, (int)v);
        }
        carry += total;
    }
    mn = amt_wave_reduce(mn, amt_min{});
    mx = amt_wave_reduce(mx, amt_max{});
    if ((tid & 63) == 0) { mm[0][tid >> 6] = mn; mm[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 4; ++i) { mn = min(mn, mm[0][i]); mx = max(mx, mm[1][i]); }
        stream_off[b + 1] = (long long)carry;
        frame_minmax[2 * b] = nframes ? mn : 0;
        frame_minmax[2 * b + 1] = nframes ? mx : 0;
    }
}

// stream_off[i + 1] holds signal i's total: in-place inclusive scan, stream_off[0] = 0.  One workgroup.
__global__ __launch_bounds__(AMT_FL_THREADS) void flac_stream_offsets_kernel(long long *__restrict__ stream_off, int n) {
    __shared__ fl_u64 lds[4];
    const int tid = threadIdx.x;
    fl_u64 carry = 0;
    if (tid == 0) stream_off[0] = 0;
    for (int i0 = 0; i0 < n; i0 += AMT_FL_THREADS) {
        const int i = i0 + tid;
        const fl_u64 v = i < n ? (fl_u64)stream_off[i + 1] : 0;
        fl_u64 total;
        const fl_u64 ex = amt_block_scan<fl_u64, AMT_FL_THREADS>(v, lds, &total);
        if (i < n) stream_off[i + 1] = (long long)(carry + ex + v);
        carry += total;
    }
}

__global__ __launch_bounds__(AMT_FL_THREADS) void flac_compact_kernel(
    const unsigned char *__restrict__ scratch, long long bound, long long frames_max,
    const long long *__restrict__ frame_bytes, const long long *__restrict__ frame_off,
    const long long *__restrict__ stream_off, unsigned char *__restrict__ out, long long out_bytes) {
    const long long slot = (long long)blockIdx.y * frames_max + blockIdx.x;
    const long long size = frame_bytes[slot];
    if (size <= 0 || size > bound) return;
    const long long at = stream_off[blockIdx.y] + frame_off[slot];
    if (at < 0 || at + size > out_bytes) return;                  // the caller sees stream_off[n] > out_bytes
    const unsigned char *src = scratch + slot * bound;
    unsigned char *dst = out + at;
    for (int i = threadIdx.x; i < (int)size; i += AMT_FL_THREADS) dst[i] = src[i];
}

#define AMT_FL_MD5_LANES 64

// MD5 of the little-endian PCM of every signal: one wave per signal.  The chain of rounds is sequential, everything
// around it is not: per 64 samples (2 or 3 blocks) lane w < 16 bps / 8 builds message word w -- its four bytes lie in two
// consecutive samples, loaded while the previous blocks are hashed -- and stores it to LDS; then every lane runs the
// same rounds on the same words (LDS broadcasts), so the lane that writes the digest spends its time on the rounds only.
// The last piece (fewer than 64 samples, the 0x80 byte, zeros, the bit length: at most 256 bytes) is one word per lane.
__global__ __launch_bounds__(AMT_FL_MD5_LANES) void flac_md5_kernel(
    const float *__restrict__ wave, const long long *__restrict__ base, const long long *__restrict__ len,
    long long max_len, int bps, unsigned char *__restrict__ md5, fl_md5_consts kc) {
    __shared__ unsigned m[64];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const long long n_s = amt_clamp_len(len[b], max_len);
    const float *x = wave + base[b];
    const int nb = bps >> 3;                                      // bytes per sample, blocks per 64 samples
    const unsigned mask = (1u << bps) - 1u;
    const int sa = nb == 2 ? 2 * lane : (4 * lane) / 3;           // first sample of word `lane` within a piece
    const int shift = 8 * (4 * lane - sa * nb);                   // its first byte inside that sample
    unsigned st[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    // the word from its two samples (a sample past the signal's end is 0 and quantises to 0)
    auto word = [&](float y0, float y1) {
        const fl_u64 v = (fl_u64)((unsigned)fl_quant(y0, bps) & mask) | ((fl_u64)((unsigned)fl_quant(y1, bps) & mask) << bps);
        return (unsigned)(v >> shift);
    };
    const bool builder = lane < 16 * nb;
    long long s0 = 0;
    float y0 = 0.f, y1 = 0.f;
    if (builder && n_s >= 64) { y0 = x[sa]; y1 = sa + 1 < 64 ? x[sa + 1] : 0.f; }
    for (; s0 + 64 <= n_s; s0 += 64) {
        if (builder) m[lane] = word(y0, y1);
        __syncthreads();
        if (builder && s0 + 128 <= n_s) {                         // the next piece's samples, in flight during the rounds
            y0 = x[s0 + 64 + sa];
            y1 = sa + 1 < 64 ? x[s0 + 64 + sa + 1] : 0.f;
        }
        for (int k = 0; k < nb; ++k) fl_md5_block(st, m + 16 * k, kc);
        __syncthreads();
    }
    {
        const int r = (int)(n_s - s0);                            // 0 .. 63 samples left
        const int data = r * nb;
        const int tail = (data + 9 + 63) / 64 * 64;               // with the 0x80 byte and the 8-byte length: <= 256
        const int words = tail >> 2;
        const fl_u64 total_bits = (fl_u64)n_s * nb * 8;
        unsigned wv = word(sa < r ? x[s0 + sa] : 0.f, sa + 1 < r ? x[s0 + sa + 1] : 0.f);
        if (4 * lane <= data && data < 4 * lane + 4) wv |= 0x80u << (8 * (data - 4 * lane));
        if (lane == words - 2) wv = (unsigned)total_bits;
        if (lane == words - 1) wv = (unsigned)(total_bits >> 32);
        if (lane < words) m[lane] = wv;
        __syncthreads();
        for (int k = 0; k < (tail >> 6); ++k) fl_md5_block(st, m + 16 * k, kc);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) md5[16 * (long long)b + j] = (unsigned char)(st[j >> 2] >> (8 * (j & 3)));
    }
}

static long long fl_frames(long long samples, int blocksize) { return (samples + blocksize - 1) / blocksize; }

extern "C" {

long long amt_flac_frame_bound(int blocksize, int bps) {
    if ((bps != 16 && bps != 24) || blocksize < 16 || blocksize > AMT_FL_MAXBS) return AMT_E_INVALID;
    return fl_bound(blocksize, bps);
}

long long amt_flac_scratch_bytes(int n, long long max_len, int blocksize, int bps) {
    const long long bound = amt_flac_frame_bound(blocksize, bps);
    if (bound < 0 || n < 1 || max_len < 0) return AMT_E_INVALID;
    amt_flac_layout L;
    const long long need = amt_flac_make_layout(nullptr, n, fl_frames(max_len, blocksize), bound, &L);
    return need < 0 ? AMT_E_INVALID : need;
}

// both entries: lpc_order 0 = the fixed predictors alone
static int fl_encode(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                     int blocksize, int bps, long long first_frame, unsigned char *scratch, long long scratch_bytes,
                     unsigned char *out, long long out_bytes, long long *frame_bytes, long long *stream_off,
                     int *frame_minmax, unsigned char *md5, void *stream_, int lpc_order) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!wave || !base || !len || !scratch || !out || !frame_bytes || !stream_off || !frame_minmax || !md5)
        return AMT_E_INVALID;
    if (n < 1 || max_len < 0 || first_frame < 0) return AMT_E_INVALID;
    if (n > 65535) return AMT_E_UNSUPPORTED;                      // the grid's second dimension
    const long long bound = amt_flac_frame_bound(blocksize, bps);
    if (bound < 0) return AMT_E_INVALID;
    const long long frames = fl_frames(max_len, blocksize);
    if (first_frame + frames >= (1LL << 31)) return AMT_E_INVALID;
    amt_flac_layout L;
    const long long need = amt_flac_make_layout(scratch, n, frames, bound, &L);
    if (need < 0) return AMT_E_INVALID;
    if (scratch_bytes < need || out_bytes < frames * bound) return AMT_E_SHAPE;
    if (frames > 0) {
        const dim3 grid((unsigned)frames, (unsigned)n);
        if (lpc_order > 0)
            flac_frame_kernel<true><<<grid, AMT_FL_THREADS, 0, stream>>>(wave, base, len, max_len, blocksize, bps,
                                                                         first_frame, frames, L.slots, bound,
                                                                         frame_bytes, lpc_order);
        else
            flac_frame_kernel<false><<<grid, AMT_FL_THREADS, 0, stream>>>(wave, base, len, max_len, blocksize, bps,
                                                                          first_frame, frames, L.slots, bound,
                                                                          frame_bytes, 0);
        AMT_LAUNCH_CHECK();
    }
    flac_frame_offsets_kernel<<<n, AMT_FL_THREADS, 0, stream>>>(len, max_len, blocksize, frames, frame_bytes,
                                                                L.frame_off, stream_off, frame_minmax);
    AMT_LAUNCH_CHECK();
    flac_stream_offsets_kernel<<<1, AMT_FL_THREADS, 0, stream>>>(stream_off, n);
    AMT_LAUNCH_CHECK();
    if (frames > 0) {
        const dim3 grid((unsigned)frames, (unsigned)n);
        flac_compact_kernel<<<grid, AMT_FL_THREADS, 0, stream>>>(L.slots, bound, frames, frame_bytes, L.frame_off,
                                                                 stream_off, out, out_bytes);
        AMT_LAUNCH_CHECK();
    }
    fl_md5_consts kc;
    fl_md5_fill(kc);
    flac_md5_kernel<<<n, AMT_FL_MD5_LANES, 0, stream>>>(wave, base, len, max_len, bps, md5, kc);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_flac_encode_ragged(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                           int blocksize, int bps, long long first_frame, unsigned char *scratch,
                           long long scratch_bytes, unsigned char *out, long long out_bytes, long long *frame_bytes,
                           long long *stream_off, int *frame_minmax, unsigned char *md5, void *stream) {
    return fl_encode(wave, base, len, n, max_len, blocksize, bps, first_frame, scratch, scratch_bytes, out, out_bytes,
                     frame_bytes, stream_off, frame_minmax, md5, stream, 0);
}

int amt_flac_encode_lpc_ragged(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                               int blocksize, int bps, long long first_frame, int lpc_order, unsigned char *scratch,
                               long long scratch_bytes, unsigned char *out, long long out_bytes, long long *frame_bytes,
                               long long *stream_off, int *frame_minmax, unsigned char *md5, void *stream) {
    if (lpc_order < 1 || lpc_order > FLL_MAX_ORDER) return AMT_E_INVALID;
    return fl_encode(wave, base, len, n, max_len, blocksize, bps, first_frame, scratch, scratch_bytes, out, out_bytes,
                     frame_bytes, stream_off, frame_minmax, md5, stream, lpc_order);
}

}  // extern "C"
