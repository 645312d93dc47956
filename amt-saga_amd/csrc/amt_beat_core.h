// Beat tracking by dynamic programming (Ellis 2007; the form people know as librosa.beat.beat_track): the rule, plain
// C++ behind one macro, so the same functions compile into the kernels of amt_beat.hip and into a stand-alone CPU program
// (tests/beat_host_main.cpp, built with the address and undefined-behaviour sanitizers).  Restated independently in
// tests/beat_reference.py.  It stands behind the transcription: the reference stops at fixed-tempo note_sequence files
// (util_audio.py:594-639), so a note's time is right in seconds and meaningless in bars.  DESIGN.md 31.
//
// After one float32 step per cell everything is an integer: a result is equal or wrong.  One song: mag [T][F] float32,
// ref (its maximum magnitude), half-width w, lags lag_lo..lag_hi, tables prior and pen.
//
// COMPRESS  x = mag / ref; c = 0 unless x > 0 (a NaN included); x = min(x, 1); c = (int)(sqrtf(x) * 1024 + 0.5f): 0..1024.
//           Correctly rounded float32 division and square root.
// FLUX      flux[0] = 0, flux[t] = sum_f max(0, c[t][f] - c[t-1][f])                         <= 2049 * 1024 < 2^22
// MEAN      lo = max(0, t - w), hi = min(T - 1, t + w); m[t] = (sum flux[lo..hi]) / (hi - lo + 1) (floor);
//           d[t] = max(0, flux[t] - m[t])                            window sums < 2^20 * 2^22 = 2^42; d < 2^22
// SCALE     q = isqrt((sum d^2) / T)                                 d <= 2049 * 1024: sum d^2 < 2^20 * 2^42.01 < 2^63
//           e[t] = min(65535, d[t] * 256 / q)                        d * 256 < 2^30
//           A song with ref <= 0 (or NaN), with q == 0 or with T == 0 has no beats: flux (ref <= 0) and e are all zero.
// TEMPO     a[L] = (sum_{t < T - L} e[t] e[t + L]) / (T - L), 0 where T - L <= 0, for 1 <= L <= 2 lag_hi + 1
//                                                                    products < 2^32, sums < 2^52, a < 2^32
//           s[L] = prior[L - lag_lo] (2 a[L] + a[2 L]), lag_lo <= L <= lag_hi         |s| < 2^15 * 3 * 2^32 < 2^49
//           P = argmax s, a tie to the smaller lag.  s[P] <= 0: no beats (period 0, count 0, C all zero, back all -1).
//           This settles T = 1, T <= lag_lo and an envelope of zeros or of one spike without a rule of their own.
// LOCAL     ls[t] = e[t-1] + 2 e[t] + e[t+1], zeros outside [0, T)                    < 2^18
// DP        H = ceil(P / 2); C[t] = ls[t] + max(0, max_tau (C[t - tau] - pen[P - lag_lo][tau])), H <= tau <= 2 P,
//           t - tau >= 0; back[t] = the winning t - tau, the smallest tau on a tie; -1 when the maximum is <= 0 (the 0
//           wins a tie) or no tau is allowed.                        C < 2^20 * 2^18 = 2^38
//           The argmax is the maximum of the packed keys (C[p] - pen[tau]) * 2^20 + p, p = t - tau < 2^20: the value
//           decides, then the larger predecessor, which is the smaller tau.  |key| < 2^58 + 2^51.
// START     argmax C over [max(0, T - P), T - 1], a tie to the smallest t, then follow back: n beats, ascending.
// TRIM      with S = sum ls[b]^2 over the n beats (< 2^20 * 2^36), keep the beats from the first to the last with
//           4 ls[b]^2 n >= S (< 2^58).  n >= 1 and the largest ls always passes, so count >= 1 for a song with beats.
// BOUND     n <= T / ceil(lag_lo / 2) + 1: consecutive beats are at least ceil(P / 2) >= ceil(lag_lo / 2) apart.
#ifndef AMT_BEAT_CORE_H
#define AMT_BEAT_CORE_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIP__
#define AMT_BEAT_HD __host__ __device__ inline
#else
#define AMT_BEAT_HD inline
#endif

#define BEAT_MAX_BINS 2049
#define BEAT_MAX_FRAMES ((1 << 20) - 1)
#define BEAT_MAX_LAG 1024
#define BEAT_E_MAX 65535
#define BEAT_IDX_BITS 20
#define BEAT_IDX_MASK ((1LL << BEAT_IDX_BITS) - 1)
#define BEAT_LAG_BITS 11                         /* a lag <= 1024 below a tempo score */
#define BEAT_KEY_NONE INT64_MIN                  /* below every key */
// The DP keeps C in a ring of BEAT_RING values, slot t mod BEAT_RING: a chunk of H = ceil(P / 2) frames writes slots
// t0 .. t0 + H - 1 and reads t0 - 2P .. t0 - 1, a span of 2P + H <= 2560 frames, so no slot written is one read.
#define BEAT_RING 4096
static_assert(BEAT_RING >= 2 * BEAT_MAX_LAG + (BEAT_MAX_LAG + 1) / 2 && (BEAT_RING & (BEAT_RING - 1)) == 0, "the ring");

// the limits of a call, checked before any HIP call
AMT_BEAT_HD int beat_env_limits_ok(long long F, long long max_frames, long long w) {
    return F >= 1 && F <= BEAT_MAX_BINS && max_frames >= 0 && max_frames <= BEAT_MAX_FRAMES && w >= 0;
}
AMT_BEAT_HD int beat_lags_ok(long long lag_lo, long long lag_hi) {
    return lag_lo >= 1 && lag_lo <= lag_hi && lag_hi <= BEAT_MAX_LAG;
}
AMT_BEAT_HD int beat_track_limits_ok(long long max_frames, long long lag_lo, long long lag_hi) {
    return max_frames >= 0 && max_frames <= BEAT_MAX_FRAMES && beat_lags_ok(lag_lo, lag_hi);
}

// lags a song's autocorrelation is kept for, index L: [0, 2 lag_hi + 2), entry 0 unused
AMT_BEAT_HD long long beat_acorr_len(long long lag_hi) { return 2 * lag_hi + 2; }
// a row of pen: index tau in [0, 2 lag_hi + 1); the entries no period of the row allows are never read
AMT_BEAT_HD long long beat_pen_pitch(long long lag_hi) { return 2 * lag_hi + 1; }
AMT_BEAT_HD long long beat_chunk(long long P) { return (P + 1) / 2; }
// beats of a song of T frames at the most
AMT_BEAT_HD long long beat_bound(long long T, long long lag_lo) { return (T < 0 ? 0 : T) / beat_chunk(lag_lo) + 1; }

AMT_BEAT_HD int beat_live(float ref) { return ref > 0.0f; }               // (false for a NaN)

AMT_BEAT_HD int beat_compress(float mag, float ref) {
    float x = mag / ref;
    if (!(x > 0.0f)) return 0;
    if (x > 1.0f) x = 1.0f;
    return (int)(sqrtf(x) * 1024.0f + 0.5f);
}

AMT_BEAT_HD int beat_rise(int c, int c_before) { return c > c_before ? c - c_before : 0; }

// d[t] from flux[t] and the inclusive prefix sums S of flux: S(i) = sum flux[0..i]
template <class Prefix> AMT_BEAT_HD long long beat_excess(long long flux_t, long long t, long long T, long long w, Prefix S) {
    const long long lo = t - w > 0 ? t - w : 0, hi = (w >= T - 1 - t) ? T - 1 : t + w;    // (no t + w: w may be huge)
    const long long sum = S(hi) - (lo > 0 ? S(lo - 1) : 0);
    const long long d = flux_t - sum / (hi - lo + 1);
    return d > 0 ? d : 0;
}

// floor(sqrt(v))
AMT_BEAT_HD uint64_t beat_isqrt(uint64_t v) {
    uint64_t r = 0;
    for (uint64_t bit = 1ULL << 62; bit; bit >>= 2) {
        if (v >= r + bit) {
            v -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
    }
    return r;
}

AMT_BEAT_HD uint64_t beat_rms(uint64_t sum_d2, long long T) { return T > 0 ? beat_isqrt(sum_d2 / (uint64_t)T) : 0; }

AMT_BEAT_HD uint16_t beat_scale(long long d, uint64_t q) {
    if (q == 0) return 0;
    const uint64_t v = (uint64_t)d * 256 / q;
    return (uint16_t)(v > BEAT_E_MAX ? BEAT_E_MAX : v);
}

// ---- tempo ----
AMT_BEAT_HD long long beat_tempo_score(long long prior, long long a_L, long long a_2L) { return prior * (2 * a_L + a_2L); }
// larger is better: the score, then the smaller lag
AMT_BEAT_HD long long beat_tempo_key(long long s, long long L) { return s * (1LL << BEAT_LAG_BITS) + ((1LL << BEAT_LAG_BITS) - 1 - L); }
AMT_BEAT_HD long long beat_tempo_key_lag(long long key) { return (1LL << BEAT_LAG_BITS) - 1 - (key & ((1LL << BEAT_LAG_BITS) - 1)); }
AMT_BEAT_HD long long beat_tempo_key_score(long long key) { return key >> BEAT_LAG_BITS; }      // (arithmetic: floor)

// ---- the DP ----
template <class Env> AMT_BEAT_HD long long beat_local(long long t, long long T, Env e) {
    return (t > 0 ? (long long)e(t - 1) : 0) + 2 * (long long)e(t) + (t + 1 < T ? (long long)e(t + 1) : 0);
}
AMT_BEAT_HD long long beat_dp_key(long long c_before, long long pen, long long p) { return (c_before - pen) * (1LL << BEAT_IDX_BITS) + p; }
// C[t] and back[t] from ls[t] and the largest key (BEAT_KEY_NONE: no candidate)
AMT_BEAT_HD long long beat_dp_close(long long ls, long long key, int32_t *back) {
    if (key < (1LL << BEAT_IDX_BITS)) {          // value <= 0: the 0 wins
        *back = -1;
        return ls;
    }
    *back = (int32_t)(key & BEAT_IDX_MASK);
    return ls + (key >> BEAT_IDX_BITS);
}
// larger is better: C, then the smaller frame
AMT_BEAT_HD long long beat_start_key(long long C, long long t) { return C * (1LL << BEAT_IDX_BITS) + (BEAT_IDX_MASK - t); }
AMT_BEAT_HD long long beat_start_key_frame(long long key) { return BEAT_IDX_MASK - (key & BEAT_IDX_MASK); }

AMT_BEAT_HD int beat_keep(long long ls, long long n, long long sum_ls2) { return 4 * ls * ls * n >= sum_ls2; }

#endif /* AMT_BEAT_CORE_H */
