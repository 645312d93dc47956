// Harmonic/percussive separation on the device for gfx950: any number of spectrograms of unequal lengths in one launch,
// each split into a harmonic and a percussive magnitude by two median filters and a mask (Fitzgerald 2010).
//
// Stands in front of the transcription: the reference renders drum tracks into every training song (util_audio.py:843)
// and hands the heads pitched notes only (util_train_test.py:83, :159), so a drum hit is energy no head can explain.
// The rule is amt_hpss_core.h's.
//
// Design:
//  * the work item is one tile of TT frames x 64 bins of one signal; a workgroup of four waves takes items in a
//    grid-stride loop under a capped grid.  Tiles that lie behind a signal's last frame are skipped by the whole
//    workgroup.
//  * LDS holds the tile twice, through the reflection map: `a` = the tile's 64 columns with (kt - 1) / 2 frames above and
//    below, `b` = the tile's rows with (kf - 1) / 2 bins left and right.  The corners of the full halo feed neither
//    median and are not loaded.  S is read about (1 + (kt - 1) / TT) + (1 + (kf - 1) / 64) times, mostly from L2.
//  * a lane owns one bin and walks the tile's frames in steps of four (one wave, one frame): the time median reads
//    a[(t + j)][lane], the frequency median b[t][lane + j] -- consecutive LDS addresses across the lanes either way.
//  * the window goes from LDS into an array that is only ever indexed by constants (registers), padded to the size class
//    so that the median lands at a fixed place, and through the compile-time sorting network of the core: integer min /
//    max, no ties, no rounding.  Templated on the two size classes (8, 32, 64), not on every k.  (Bisection on the
//    bit pattern with the window read from LDS in every pass measured 16.8 times slower at k = 31: DESIGN 30.)
//  * masks and products in the core's written-out order; contraction is off for this file.
//  * plain stores, every cell of a signal's frames written exactly once, pad columns as zero; no atomics; no packed-FP32
//    instructions: any stream.
#include "amt_launch.h"
#include "amt_hpss_core.h"

#define HPSS_THREADS 256                  /* four waves */
#define HPSS_TF 64                        /* bins of a tile: one per lane */
#define HPSS_MAX_GRID 2047

template <int NT, int NF> struct hpss_tile {
    static constexpr int TT = (NT == 64 || NF == 64) ? 32 : 64;         // frames of a tile
    static constexpr int A_ROWS = TT + NT - 2, B_COLS = HPSS_TF + NF - 2;
    static constexpr int A_WORDS = A_ROWS * HPSS_TF, B_WORDS = TT * B_COLS;
};

static int hpss_tile_frames(int nt, int nf) { return (nt == 64 || nf == 64) ? 32 : 64; }

struct hpss_params {
    const float *mag;
    float *out_h, *out_p, *out_r, *med_t, *med_f;
    const int64_t *frame_base;
    const int32_t *t_frames;
    long long n, pool_frames, tiles_t, tiles_f;
    int max_frames, ldf, F, kt, kf;
    float power, margin_h, margin_p;
};

template <int NT, int NF>
__global__ __launch_bounds__(HPSS_THREADS) void hpss_kernel(hpss_params P) {
    using tile = hpss_tile<NT, NF>;
    __shared__ uint32_t lds[tile::A_WORDS + tile::B_WORDS];
    uint32_t *a = lds, *b = lds + tile::A_WORDS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ht = (P.kt - 1) / 2, hf = (P.kf - 1) / 2, F = P.F, ldf = P.ldf;
    const int b_cols = HPSS_TF + P.kf - 1;
    const long long per_signal = P.tiles_t * P.tiles_f, items = P.n * per_signal;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long sig = item / per_signal, rest = item % per_signal;
        const long long t0 = (rest / P.tiles_f) * tile::TT;
        const int f0 = (int)(rest % P.tiles_f) * HPSS_TF;
        // the signal's frames, held inside the pools whatever the tables say (the same answer in every thread)
        const long long fb = P.frame_base[sig], T = P.t_frames[sig];
        if (T <= 0 || T > P.max_frames || fb < 0 || fb > P.pool_frames - T || t0 >= T) continue;
        const int rows = (int)(T - t0 < tile::TT ? T - t0 : tile::TT);
        __syncthreads();                                               // the last item's reads of lds are over
        // a wave takes every fourth row of either image, a lane a column (and every 64th of b's): one reflection per row
        // of a, none that divides inside the axis
        const int f = f0 + lane;
        for (int r = wave; r < rows + 2 * ht; r += HPSS_THREADS / 64) {
            uint32_t v = 0;
            if (f < F) v = hpss_bits(P.mag[(fb + hpss_reflect(t0 - ht + r, T)) * ldf + f]);
            a[r * HPSS_TF + lane] = v;
        }
        for (int r = wave; r < rows; r += HPSS_THREADS / 64) {
            const float *src = P.mag + (fb + t0 + r) * ldf;
            for (int c = lane; c < b_cols; c += 64)
                b[r * tile::B_COLS + c] = hpss_bits(src[hpss_reflect((long long)f0 - hf + c, F)]);
        }
        __syncthreads();
        if (f >= ldf) continue;                                        // (no barrier below)
        for (int t = wave; t < rows; t += HPSS_THREADS / 64) {
            const long long at = (fb + t0 + t) * ldf + f;
            float med_t = 0.0f, med_f = 0.0f, sh = 0.0f, sp = 0.0f, sr = 0.0f;
            if (f < F) {
                const uint32_t *col = a + t * HPSS_TF + lane, *row = b + t * tile::B_COLS + lane;
                med_t = hpss_float(hpss_median<NT>(P.kt, [&](int j) { return col[j * HPSS_TF]; }));
                med_f = hpss_float(hpss_median<NF>(P.kf, [&](int j) { return row[j]; }));
                const float s = hpss_float(row[hf]);
                float mask_h, mask_p;
                hpss_masks(med_t, med_f, P.power, P.margin_h, P.margin_p, &mask_h, &mask_p);
                sh = s * mask_h;
                sp = s * mask_p;
                sr = hpss_rest(s, sh, sp);
            }
            P.out_h[at] = sh;
            P.out_p[at] = sp;
            if (P.out_r) P.out_r[at] = sr;
            if (P.med_t) P.med_t[at] = med_t;
            if (P.med_f) P.med_f[at] = med_f;
        }
    }
}

using HpssClasses = amt_values<8, 32, 64>;

extern "C" {

int amt_hpss_ragged(const amt_hpss_args *x, void *stream) {
    if (!x || !x->mag || !x->out_h || !x->out_p || !x->frame_base || !x->t_frames) return AMT_E_INVALID;
    const float *outs[5] = {x->out_h, x->out_p, x->out_r, x->med_t, x->med_f};
    for (int i = 0; i < 5; ++i) {
        if (!outs[i]) continue;
        if (outs[i] == x->mag) return AMT_E_INVALID;
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return AMT_E_INVALID;
    }
    if (!hpss_params_ok(x->kt, x->kf, x->power, x->margin_h, x->margin_p)) return AMT_E_INVALID;
    if (x->F < 1 || x->F > x->ldf || (x->ldf & 3) || x->n < 0 || x->max_frames < 0 || x->pool_frames < 0)
        return AMT_E_INVALID;
    if (x->n == 0 || x->max_frames == 0) return AMT_OK;               // nothing to do, and nothing is launched
    const int nt = hpss_class(x->kt), nf = hpss_class(x->kf), tt = hpss_tile_frames(nt, nf);
    hpss_params P;
    P.mag = x->mag; P.out_h = x->out_h; P.out_p = x->out_p; P.out_r = x->out_r; P.med_t = x->med_t; P.med_f = x->med_f;
    P.frame_base = x->frame_base; P.t_frames = x->t_frames;
    P.n = x->n; P.pool_frames = x->pool_frames;
    P.tiles_t = ((long long)x->max_frames + tt - 1) / tt;
    P.tiles_f = (x->ldf + HPSS_TF - 1) / HPSS_TF;
    P.max_frames = x->max_frames; P.ldf = x->ldf; P.F = x->F; P.kt = x->kt; P.kf = x->kf;
    P.power = x->power; P.margin_h = x->margin_h; P.margin_p = x->margin_p;
    long long grid = P.n * P.tiles_t * P.tiles_f;
    if (grid > HPSS_MAX_GRID) grid = HPSS_MAX_GRID;
    hipStream_t st = (hipStream_t)stream;
    return amt_dispatch(HpssClasses{}, nt, [&](auto NT) {
        return amt_dispatch(HpssClasses{}, nf, [&](auto NF) {
            hpss_kernel<NT(), NF()><<<(unsigned)grid, HPSS_THREADS, 0, st>>>(P);
            AMT_LAUNCH_CHECK();
            return (int)AMT_OK;
        });
    });
}

}  // extern "C"
