// Beat tracking on the device for gfx950: onset envelopes and dynamic-programming beat tracks (Ellis 2007) of any number
// of songs of unequal lengths, two ABI calls of a few stream-ordered launches each and no host synchronisation between
// their stages.  The reference stops at fixed-tempo note_sequence files (util_audio.py:594-639); this gives the MIDI
// writer a tempo map.  The rule is amt_beat_core.h's: one float32 step per cell, integers from there on.
//
// amt_beat_envelope, two launches:
//  * beat_flux_kernel -- the work item is one run of BEAT_RUN frames of one song, taken by ONE WAVE: a lane owns the bins
//    lane, lane + 64, ... (33 registers for F = 2049) and keeps the previous frame's compressed values there, so a
//    magnitude is read once, plus one frame per run for the run's first difference.  A frame's flux is one integer wave
//    reduction; no LDS, no barrier.  Pad columns f >= F are never read.
//  * beat_scale_kernel -- one workgroup per song: a carried block scan turns flux into int64 prefix sums (scratch), every
//    local mean is then two reads, sum d^2 is an integer block reduction, and e follows from a second evaluation of d.
// amt_beat_track, two launches:
//  * beat_acorr_kernel -- one wave per (song, lag), lanes over the frames, an integer wave reduction.
//  * beat_dp_kernel -- one workgroup of sixteen waves per song: the tempo (a block reduction of packed keys; the period
//    never leaves the device), then the DP in chunks of H = ceil(P / 2) frames: C[t] reads C[t - 2P .. t - H] only, so
//    the frames of a chunk are independent -- waves over the chunk's frames, four at a time with sixteen lanes each over a frame's candidates, the argmax one
//    butterfly of the packed key inside the groups of sixteen (four steps for four frames).  C lives in an LDS ring of 4096 values (>= 2P + H = 2560 at P = 1024): a chunk
//    writes slots no wave of the chunk reads, so ONE barrier per chunk orders everything, ceil(T / H) in all, and one
//    more whenever the local scores of the next 1024 frames are swept into LDS (a chunk that loaded its own e from
//    global memory waited a load's latency per barrier: measured 2.7 us a chunk).  back goes to scratch with plain
//    stores; one thread follows it (at most T / H dependent loads), all trim and copy.
//  * plain stores, no atomics, no packed-FP32 instructions: any stream.  Every table value read on the device is held
//    inside the arrays whatever the tables say.
#include "amt_launch.h"
#include "amt_wg.h"
#include "amt_scratch.h"
#include "amt_beat_core.h"

#define BEAT_THREADS 256                  /* flux, scale, acorr: four waves */
#define BEAT_RUN 16                       /* frames a wave walks */
#define BEAT_COLS ((BEAT_MAX_BINS + 63) / 64)
#define BEAT_DP_THREADS 1024              /* sixteen waves */
#define BEAT_DP_LANES 16                  /* lanes that share a frame's candidates: a power of two */
#define BEAT_DP_FRAMES (64 / BEAT_DP_LANES) /* frames of a chunk a wave takes at a time */
#define BEAT_LS_RING 1024                 /* local scores kept in LDS: >= a chunk (512 at the most), a power of two */
#define BEAT_MAX_GRID 65535
#define BEAT_MAX_SONGS (1LL << 24)

static_assert(BEAT_LS_RING >= (BEAT_MAX_LAG + 1) / 2 && (BEAT_LS_RING & (BEAT_LS_RING - 1)) == 0, "a chunk fits the ring of local scores");

// the song's frames, held inside the pool whatever the tables say: false if it is to be left alone
__device__ __forceinline__ bool beat_song(const int64_t *frame_base, const int32_t *t_frames, long long sig, int max_frames,
                                          long long pool_frames, long long *fb, int *T) {
    const long long b = frame_base[sig];
    const int t = t_frames[sig];
    *fb = b;
    *T = t;
    return t >= 0 && t <= max_frames && b >= 0 && b <= pool_frames - t;
}

// op over a workgroup of THREADS, the result in every thread.  lds: THREADS / 64 elements; a barrier before it is written
// and one after.
template <int THREADS, class T, class Op>
__device__ __forceinline__ T beat_block_reduce(T v, T *lds, Op op) {
    v = amt_wave_reduce(v, op);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = lds[0];
#pragma unroll
    for (int i = 1; i < THREADS / 64; ++i) r = op(r, lds[i]);
    return r;
}

struct beat_env_params {
    const float *mag, *ref;
    const int64_t *frame_base;
    const int32_t *t_frames;
    uint16_t *env;
    int32_t *flux;
    long long *prefix;
    long long n, pool_frames, tiles, w;
    int max_frames, ldf, F;
};

__global__ __launch_bounds__(BEAT_THREADS) void beat_flux_kernel(beat_env_params P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, F = P.F;
    const long long items = P.n * P.tiles;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long sig = item / P.tiles;
        const long long t0 = ((item % P.tiles) * (BEAT_THREADS / 64) + wave) * BEAT_RUN;
        long long fb;
        int T;
        if (!beat_song(P.frame_base, P.t_frames, sig, P.max_frames, P.pool_frames, &fb, &T) || t0 >= T) continue;
        const int rows = (int)(T - t0 < BEAT_RUN ? T - t0 : BEAT_RUN);
        const float ref = P.ref[sig];
        if (!beat_live(ref)) {
            if (lane < rows) P.flux[fb + t0 + lane] = 0;
            continue;
        }
        int prev[BEAT_COLS];
        for (int r = t0 > 0 ? -1 : 0; r < rows; ++r) {
            const float *row = P.mag + (fb + t0 + r) * P.ldf;
            int sum = 0;
#pragma unroll
            for (int j = 0; j < BEAT_COLS; ++j) {
                if (j * 64 >= F) continue;                               // (the same answer in the whole wave)
                const int f = j * 64 + lane;
                const int c = f < F ? beat_compress(row[f], ref) : 0;
                if (r >= 0 && t0 + r > 0) sum += beat_rise(c, prev[j]);
                prev[j] = c;
            }
            if (r < 0) continue;
            sum = amt_wave_reduce(sum, amt_sum{});
            if (lane == 0) P.flux[fb + t0 + r] = sum;
        }
    }
}

__global__ __launch_bounds__(BEAT_THREADS) void beat_scale_kernel(beat_env_params P) {
    __shared__ long long lds[BEAT_THREADS / 64];
    __shared__ unsigned long long lds_u[BEAT_THREADS / 64];
    const int tid = threadIdx.x;
    for (long long sig = blockIdx.x; sig < P.n; sig += gridDim.x) {
        long long fb;
        int T;
        if (!beat_song(P.frame_base, P.t_frames, sig, P.max_frames, P.pool_frames, &fb, &T) || T == 0) continue;
        const int32_t *flux = P.flux + fb;
        long long *S = P.prefix + fb;
        long long carry = 0;
        for (int base = 0; base < T; base += BEAT_THREADS) {
            const int t = base + tid;
            const long long v = t < T ? flux[t] : 0;
            long long total;
            const long long before = amt_block_scan<long long, BEAT_THREADS>(v, lds, &total);
            if (t < T) S[t] = carry + before + v;
            carry += total;
        }
        __syncthreads();                                               // S, written by other threads, is read below
        const auto prefix = [&](long long i) { return S[i]; };
        unsigned long long d2 = 0;
        for (int t = tid; t < T; t += BEAT_THREADS) {
            const unsigned long long d = (unsigned long long)beat_excess(flux[t], t, T, P.w, prefix);
            d2 += d * d;
        }
        d2 = beat_block_reduce<BEAT_THREADS>(d2, lds_u, amt_sum{});
        const uint64_t q = beat_live(P.ref[sig]) ? beat_rms(d2, T) : 0;
        for (int t = tid; t < T; t += BEAT_THREADS)
            P.env[fb + t] = q ? beat_scale(beat_excess(flux[t], t, T, P.w, prefix), q) : (uint16_t)0;
        __syncthreads();                                               // lds of the next song's scan
    }
}

struct beat_track_params {
    const uint16_t *env;
    const int64_t *frame_base, *beat_base;
    const int32_t *t_frames, *prior, *pen;
    int32_t *period, *count, *beats, *back, *found;
    long long *acorr, *C;
    long long n, pool_frames, beats_total, lag_blocks;
    int max_frames, lag_lo, lag_hi;
};

__global__ __launch_bounds__(BEAT_THREADS) void beat_acorr_kernel(beat_track_params P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long len = beat_acorr_len(P.lag_hi), items = P.n * P.lag_blocks;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long sig = item / P.lag_blocks;
        const long long L = (item % P.lag_blocks) * (BEAT_THREADS / 64) + wave;      // 0 .. len - 1 (and a few behind)
        long long fb;
        int T;
        if (L >= len) continue;
        unsigned long long sum = 0;
        const bool song = beat_song(P.frame_base, P.t_frames, sig, P.max_frames, P.pool_frames, &fb, &T);
        const long long m = song && L >= 1 ? T - L : 0;
        if (m > 0) {
            const uint16_t *e = P.env + fb;
            for (long long t = lane; t < m; t += 64) sum += (unsigned long long)((uint32_t)e[t] * (uint32_t)e[t + L]);
            sum = amt_wave_reduce(sum, amt_sum{}) / (unsigned long long)m;
        }
        if (lane == 0) P.acorr[sig * len + L] = (long long)sum;
    }
}

__global__ __launch_bounds__(BEAT_DP_THREADS) void beat_dp_kernel(beat_track_params P) {
    __shared__ long long ring[BEAT_RING];
    __shared__ int32_t pen[2 * BEAT_MAX_LAG + 1];
    __shared__ int32_t ls_ring[BEAT_LS_RING];
    __shared__ long long red[BEAT_DP_THREADS / 64];
    __shared__ int found_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = BEAT_DP_THREADS / 64;
    const long long len = beat_acorr_len(P.lag_hi);
    for (long long sig = blockIdx.x; sig < P.n; sig += gridDim.x) {
        long long fb;
        int T;
        const bool song = beat_song(P.frame_base, P.t_frames, sig, P.max_frames, P.pool_frames, &fb, &T);
        const long long bound = beat_bound(song ? T : 0, P.lag_lo), bb = P.beat_base[sig];
        const bool room = bb >= 0 && bb <= P.beats_total - bound;
        if (!song || !room) {                                          // left alone but for the two counts
            if (tid == 0) P.period[sig] = P.count[sig] = 0;
            continue;
        }
        const uint16_t *e = P.env + fb;
        const auto env = [&](long long t) { return e[t]; };
        // ---- tempo ----
        const long long *a = P.acorr + sig * len;
        long long key = BEAT_KEY_NONE;
        for (int L = P.lag_lo + tid; L <= P.lag_hi; L += BEAT_DP_THREADS) {
            const long long k = beat_tempo_key(beat_tempo_score(P.prior[L - P.lag_lo], a[L], a[2 * L]), L);
            key = k > key ? k : key;
        }
        key = beat_block_reduce<BEAT_DP_THREADS>(key, red, amt_max{});
        const int period = beat_tempo_key_score(key) > 0 ? (int)beat_tempo_key_lag(key) : 0;
        if (period == 0 || T == 0) {
            for (int t = tid; t < T; t += BEAT_DP_THREADS) {
                P.back[fb + t] = -1;
                if (P.C) P.C[fb + t] = 0;
            }
            if (tid == 0) P.period[sig] = P.count[sig] = 0;
            continue;
        }
        // ---- the DP ----
        const int H = (int)beat_chunk(period);
        const int32_t *pen_row = P.pen + (long long)(period - P.lag_lo) * beat_pen_pitch(P.lag_hi);
        __syncthreads();                                               // the last song's reads of pen and ring are over
        for (int tau = H + tid; tau <= 2 * period; tau += BEAT_DP_THREADS) pen[tau] = pen_row[tau];
        __syncthreads();
        int loaded_to = 0;                                             // ls of the frames below it is in ls_ring
        for (int t0 = 0; t0 < T; t0 += H) {
            const int t1 = t0 + H < T ? t0 + H : T;
            if (t1 > loaded_to) {                                      // (the same answer in every thread)
                // the local scores of the next BEAT_LS_RING frames in one sweep: a chunk then waits for no global load.
                // The barrier that ended the last chunk stands between its reads of ls_ring and these writes.
                loaded_to = t0 + BEAT_LS_RING < T ? t0 + BEAT_LS_RING : T;
                for (int t = t0 + tid; t < loaded_to; t += BEAT_DP_THREADS)
                    ls_ring[t & (BEAT_LS_RING - 1)] = (int32_t)beat_local(t, T, env);
                __syncthreads();
            }
            // a wave takes BEAT_DP_FRAMES consecutive frames at a time, BEAT_DP_LANES lanes each: the lanes of a frame stride
            // over its candidates, and one butterfly inside the groups of BEAT_DP_LANES reduces all the frames at once
            for (int tb = t0 + wave * BEAT_DP_FRAMES; tb < t1; tb += waves * BEAT_DP_FRAMES) {
                const int t = tb + lane / BEAT_DP_LANES, slot = lane % BEAT_DP_LANES;
                long long best = BEAT_KEY_NONE;
                if (t < t1)
                    for (int tau = H + slot; tau <= 2 * period && tau <= t; tau += BEAT_DP_LANES) {
                        const int p = t - tau;
                        const long long key_p = beat_dp_key(ring[p & (BEAT_RING - 1)], pen[tau], p);
                        best = key_p > best ? key_p : best;
                    }
#pragma unroll
                for (int off = BEAT_DP_LANES / 2; off > 0; off >>= 1) {
                    const long long other = __shfl_xor(best, off, 64);
                    best = other > best ? other : best;
                }
                if (slot == 0 && t < t1) {
                    int32_t from;
                    const long long c = beat_dp_close(ls_ring[t & (BEAT_LS_RING - 1)], best, &from);
                    ring[t & (BEAT_RING - 1)] = c;
                    P.back[fb + t] = from;
                    if (P.C) P.C[fb + t] = c;
                }
            }
            __syncthreads();                                           // the chunk's C and back, before anyone reads them
        }
        // ---- where the last beat is ----
        key = BEAT_KEY_NONE;
        for (int t = (T > period ? T - period : 0) + tid; t < T; t += BEAT_DP_THREADS) {
            const long long k = beat_start_key(ring[t & (BEAT_RING - 1)], t);
            key = k > key ? k : key;
        }
        key = beat_block_reduce<BEAT_DP_THREADS>(key, red, amt_max{});
        int32_t *found = P.found + bb;
        if (tid == 0) {
            int n = 0;
            for (long long b = beat_start_key_frame(key); b >= 0 && b < T && n < bound; b = P.back[fb + b])
                found[bound - 1 - n++] = (int32_t)b;
            found_n = n;
        }
        __syncthreads();
        const int n = found_n;
        const int32_t *list = found + (bound - n);                     // ascending
        // ---- trim ----
        long long sum = 0;
        for (int k = tid; k < n; k += BEAT_DP_THREADS) {
            const long long ls = beat_local(list[k], T, env);
            sum += ls * ls;
        }
        sum = beat_block_reduce<BEAT_DP_THREADS>(sum, red, amt_sum{});
        long long first = n, last = -1;
        for (int k = tid; k < n; k += BEAT_DP_THREADS)
            if (beat_keep(beat_local(list[k], T, env), n, sum)) {
                first = k < first ? k : first;
                last = k > last ? k : last;
            }
        first = beat_block_reduce<BEAT_DP_THREADS>(first, red, amt_min{});
        last = beat_block_reduce<BEAT_DP_THREADS>(last, red, amt_max{});
        const int count = last >= first ? (int)(last - first + 1) : 0;
        for (int k = tid; k < count; k += BEAT_DP_THREADS) P.beats[bb + k] = list[first + k];
        if (tid == 0) {
            P.period[sig] = period;
            P.count[sig] = count;
        }
    }
}

static long long beat_grid(long long items) { return items < 1 ? 1 : (items > BEAT_MAX_GRID ? BEAT_MAX_GRID : items); }

extern "C" {

long long amt_beat_scratch_bytes(long long n, long long pool_frames, int lag_hi, long long beats_total) {
    amt_beat_layout L;
    if (lag_hi < 0 || lag_hi > BEAT_MAX_LAG || n > BEAT_MAX_SONGS) return AMT_E_INVALID;
    const long long bytes = amt_beat_make_layout(nullptr, n, pool_frames, beat_acorr_len(lag_hi), beats_total, &L);
    return bytes < 0 ? (long long)AMT_E_INVALID : bytes;
}

int amt_beat_envelope(const amt_beat_env_args *x, void *stream) {
    if (!x || !x->mag || !x->ref || !x->frame_base || !x->t_frames || !x->env || !x->scratch ||
        ((uintptr_t)x->scratch & 15))
        return AMT_E_INVALID;
    if (!beat_env_limits_ok(x->F, x->max_frames, x->w) || x->F > x->ldf || x->n < 0 || x->n > BEAT_MAX_SONGS ||
        x->pool_frames < 0 || x->scratch_bytes < 0)
        return AMT_E_INVALID;
    amt_beat_layout L;
    const long long need = amt_beat_make_layout(x->scratch, x->n, x->pool_frames, beat_acorr_len(0), 0, &L);   // (lag_hi = 0)
    if (need < 0) return AMT_E_INVALID;
    if (x->scratch_bytes < need) return AMT_E_SHAPE;
    if (x->n == 0 || x->max_frames == 0) return AMT_OK;               // nothing to do, and nothing is launched
    beat_env_params P;
    P.mag = x->mag; P.ref = x->ref; P.frame_base = x->frame_base; P.t_frames = x->t_frames; P.env = x->env;
    P.flux = x->flux ? x->flux : L.flux; P.prefix = L.prefix;
    P.n = x->n; P.pool_frames = x->pool_frames; P.w = x->w;
    P.tiles = ((long long)x->max_frames + BEAT_RUN * (BEAT_THREADS / 64) - 1) / (BEAT_RUN * (BEAT_THREADS / 64));
    P.max_frames = x->max_frames; P.ldf = x->ldf; P.F = x->F;
    hipStream_t st = (hipStream_t)stream;
    beat_flux_kernel<<<(unsigned)beat_grid(P.n * P.tiles), BEAT_THREADS, 0, st>>>(P);
    AMT_LAUNCH_CHECK();
    beat_scale_kernel<<<(unsigned)beat_grid(P.n), BEAT_THREADS, 0, st>>>(P);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_beat_track(const amt_beat_track_args *x, void *stream) {
    if (!x || !x->env || !x->frame_base || !x->t_frames || !x->prior || !x->pen || !x->beat_base || !x->period ||
        !x->count || !x->beats || !x->scratch || ((uintptr_t)x->scratch & 15))
        return AMT_E_INVALID;
    if (!beat_track_limits_ok(x->max_frames, x->lag_lo, x->lag_hi) || x->n < 0 || x->n > BEAT_MAX_SONGS ||
        x->pool_frames < 0 || x->beats_total < 0 || x->scratch_bytes < 0)
        return AMT_E_INVALID;
    amt_beat_layout L;
    const long long need = amt_beat_make_layout(x->scratch, x->n, x->pool_frames, beat_acorr_len(x->lag_hi), x->beats_total, &L);
    if (need < 0) return AMT_E_INVALID;
    if (x->scratch_bytes < need) return AMT_E_SHAPE;
    if (x->n == 0) return AMT_OK;                                     // nothing to do, and nothing is launched
    beat_track_params P;
    P.env = x->env; P.frame_base = x->frame_base; P.beat_base = x->beat_base; P.t_frames = x->t_frames;
    P.prior = x->prior; P.pen = x->pen; P.period = x->period; P.count = x->count; P.beats = x->beats;
    P.back = x->back ? x->back : L.back; P.found = L.found; P.acorr = L.acorr; P.C = (long long *)x->C;
    P.n = x->n; P.pool_frames = x->pool_frames; P.beats_total = x->beats_total;
    P.lag_blocks = (beat_acorr_len(x->lag_hi) + BEAT_THREADS / 64 - 1) / (BEAT_THREADS / 64);
    P.max_frames = x->max_frames; P.lag_lo = x->lag_lo; P.lag_hi = x->lag_hi;
    hipStream_t st = (hipStream_t)stream;
    beat_acorr_kernel<<<(unsigned)beat_grid(P.n * P.lag_blocks), BEAT_THREADS, 0, st>>>(P);
    AMT_LAUNCH_CHECK();
    beat_dp_kernel<<<(unsigned)beat_grid(P.n), BEAT_DP_THREADS, 0, st>>>(P);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // extern "C"
