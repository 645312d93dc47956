// amt_beat_core.h and the beat layout of amt_scratch.h on the host, alone: built by tests/test_beat_cpu.py with the address
// and undefined-behaviour sanitizers and run directly.  Reads packed cases and does each the way the kernels do -- the
// prefix sums, the packed keys, the DP in chunks over a ring of BEAT_RING values, the backtrace written from the end of
// the found list -- in arrays of exactly the stated sizes, the scratch carved by amt_beat_make_layout from a buffer of
// exactly the bytes it counted.
//
// File: "BEAT", int32 groups; per group int32 kind.
//   kind 0 (envelope): int32 T, F, ldf, w; float32 ref; float32 S[T][ldf].   Out: int32 flux[T], uint16 e[T].
//   kind 1 (tracks):   int32 lag_lo, lag_hi, n; int32 prior[lag_hi - lag_lo + 1]; int32 pen[lag_hi - lag_lo + 1][2 lag_hi + 1];
//                      per song int32 T, uint16 e[T].   Out per song: int32 period, count, beats[count]; int64 C[T]; int32 back[T].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "amt_beat_core.h"
#include "amt_scratch.h"

static bool read_exact(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
template <class T> static bool put(const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, stdout) == n; }

static int fail(int group, const char *what, int code) {
    fprintf(stderr, "group %d: %s\n", group, what);
    return code;
}

static int envelope(FILE *f, int g) {
    int32_t dims[4];
    float ref;
    if (!read_exact(f, dims, sizeof dims) || !read_exact(f, &ref, 4)) return fail(g, "short file", 2);
    const int T = dims[0], F = dims[1], ldf = dims[2], w = dims[3];
    if (!beat_env_limits_ok(F, T, w) || F > ldf) return fail(g, "parameters outside the limits", 3);
    // the live bins alone, in an array of exactly T * F values: a read of a pad column or past an end is a report
    std::vector<float> row((size_t)ldf), S((size_t)T * F);
    for (int t = 0; t < T; ++t) {
        if (!read_exact(f, row.data(), 4u * ldf)) return fail(g, "short file", 2);
        memcpy(S.data() + (size_t)t * F, row.data(), 4u * F);
    }
    amt_beat_layout L;
    const long long bytes = amt_beat_make_layout(nullptr, 1, T, 0, 0, &L);
    if (bytes < 0) return fail(g, "layout refused", 3);
    void *scratch = malloc(bytes ? (size_t)bytes : 1);
    if (amt_beat_make_layout(scratch, 1, T, 0, 0, &L) != bytes) return fail(g, "layout changed", 2);
    std::vector<uint16_t> e((size_t)T, 0);
    std::vector<int> prev((size_t)F, 0);
    const bool live = beat_live(ref);
    for (int t = 0; t < T; ++t) {
        int sum = 0;
        for (int b = 0; live && b < F; ++b) {
            const int c = beat_compress(S[(size_t)t * F + b], ref);
            if (t > 0) sum += beat_rise(c, prev[b]);
            prev[b] = c;
        }
        L.flux[t] = sum;
        L.prefix[t] = (t ? L.prefix[t - 1] : 0) + sum;
    }
    const auto prefix = [&](long long i) { return L.prefix[i]; };
    uint64_t d2 = 0;
    for (int t = 0; t < T; ++t) {
        const uint64_t d = (uint64_t)beat_excess(L.flux[t], t, T, w, prefix);
        d2 += d * d;
    }
    const uint64_t q = live ? beat_rms(d2, T) : 0;
    for (int t = 0; t < T; ++t) e[t] = q ? beat_scale(beat_excess(L.flux[t], t, T, w, prefix), q) : (uint16_t)0;
    const bool ok = put(L.flux, (size_t)T) && put(e.data(), (size_t)T);
    free(scratch);
    return ok ? 0 : fail(g, "short write", 2);
}

static int tracks(FILE *f, int g) {
    int32_t dims[3];
    if (!read_exact(f, dims, sizeof dims)) return fail(g, "short file", 2);
    const int lag_lo = dims[0], lag_hi = dims[1], n = dims[2];
    if (!beat_lags_ok(lag_lo, lag_hi) || n < 0) return fail(g, "parameters outside the limits", 3);
    const long long rows = lag_hi - lag_lo + 1, pitch = beat_pen_pitch(lag_hi), len = beat_acorr_len(lag_hi);
    std::vector<int32_t> prior((size_t)rows), pen((size_t)(rows * pitch));
    if (!read_exact(f, prior.data(), 4u * prior.size()) || !read_exact(f, pen.data(), 4u * pen.size()))
        return fail(g, "short file", 2);
    for (int s = 0; s < n; ++s) {
        int32_t T;
        if (!read_exact(f, &T, 4)) return fail(g, "short file", 2);
        if (!beat_track_limits_ok(T, lag_lo, lag_hi)) return fail(g, "parameters outside the limits", 3);
        std::vector<uint16_t> e((size_t)T);
        if (!read_exact(f, e.data(), 2u * T)) return fail(g, "short file", 2);
        const long long bound = beat_bound(T, lag_lo);
        amt_beat_layout L;
        const long long bytes = amt_beat_make_layout(nullptr, 1, T, len, bound, &L);
        if (bytes < 0) return fail(g, "layout refused", 3);
        void *scratch = malloc((size_t)bytes);
        if (amt_beat_make_layout(scratch, 1, T, len, bound, &L) != bytes) return fail(g, "layout changed", 2);
        const auto env = [&](long long t) { return e[(size_t)t]; };
        std::vector<long long> C((size_t)T, 0), ring(BEAT_RING, 0);
        std::vector<int32_t> beats;
        int32_t period = 0, count = 0;
        for (long long lag = 0; lag < len; ++lag) {
            unsigned long long sum = 0;
            const long long m = lag >= 1 ? T - lag : 0;
            for (long long t = 0; t < m; ++t) sum += (unsigned long long)((uint32_t)e[t] * (uint32_t)e[t + lag]);
            L.acorr[lag] = m > 0 ? (long long)(sum / (unsigned long long)m) : 0;
        }
        long long key = BEAT_KEY_NONE;
        for (int lag = lag_lo; lag <= lag_hi; ++lag) {
            const long long k = beat_tempo_key(beat_tempo_score(prior[lag - lag_lo], L.acorr[lag], L.acorr[2 * lag]), lag);
            key = k > key ? k : key;
        }
        period = beat_tempo_key_score(key) > 0 ? (int32_t)beat_tempo_key_lag(key) : 0;
        for (int t = 0; t < T; ++t) L.back[t] = -1;
        if (period && T) {
            const int H = (int)beat_chunk(period);
            const int32_t *row = pen.data() + (size_t)(period - lag_lo) * pitch;
            for (int t0 = 0; t0 < T; t0 += H)
                for (int t = t0; t < t0 + H && t < T; ++t) {
                    long long best = BEAT_KEY_NONE;
                    for (int tau = H; tau <= 2 * period && tau <= t; ++tau) {
                        const int p = t - tau;
                        const long long k = beat_dp_key(ring[p & (BEAT_RING - 1)], row[tau], p);
                        best = k > best ? k : best;
                    }
                    ring[t & (BEAT_RING - 1)] = C[t] = beat_dp_close(beat_local(t, T, env), best, &L.back[t]);
                }
            key = BEAT_KEY_NONE;
            for (int t = T > period ? T - period : 0; t < T; ++t) {
                const long long k = beat_start_key(ring[t & (BEAT_RING - 1)], t);
                key = k > key ? k : key;
            }
            int found = 0;
            for (long long b = beat_start_key_frame(key); b >= 0 && b < T && found < bound; b = L.back[b])
                L.found[bound - 1 - found++] = (int32_t)b;
            const int32_t *list = L.found + (bound - found);
            long long sum = 0, first = found, last = -1;
            for (int k = 0; k < found; ++k) {
                const long long ls = beat_local(list[k], T, env);
                sum += ls * ls;
            }
            for (int k = 0; k < found; ++k)
                if (beat_keep(beat_local(list[k], T, env), found, sum)) {
                    first = k < first ? k : first;
                    last = k;
                }
            count = last >= first ? (int32_t)(last - first + 1) : 0;
            beats.assign(list + (count ? first : 0), list + (count ? first : 0) + count);
        }
        const bool ok = put(&period, 1) && put(&count, 1) && put(beats.data(), beats.size()) && put(C.data(), C.size()) &&
                        put(L.back, (size_t)T);
        free(scratch);
        if (!ok) return fail(g, "short write", 2);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: beat_host_main cases.bin > results\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char magic[4];
    int32_t n = 0;
    if (!read_exact(f, magic, 4) || memcmp(magic, "BEAT", 4) != 0 || !read_exact(f, &n, 4) || n < 0) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    for (int g = 0; g < n; ++g) {
        int32_t kind;
        if (!read_exact(f, &kind, 4) || (kind != 0 && kind != 1)) return fail(g, "bad kind", 2);
        const int rc = kind == 0 ? envelope(f, g) : tracks(f, g);
        if (rc) return rc;
    }
    fclose(f);
    return 0;
}
