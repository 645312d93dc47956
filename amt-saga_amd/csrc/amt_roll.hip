// Piano-roll images on the device for gfx950: any number of images in one launch, each with its own geometry, an
// estimate list and, in pair mode, a gold list -> uint8 [H, W] palette indices (background with key rows and ticks,
// sixteen group hues with onsets, or the estimate-only / gold-only / both classes of a pair).
//
// Stands where the reference's users would plot a piano roll of the MIDI/audio pairs the reference trains on (main.py:7)
// with matplotlib on the host.  The host sorts and packs (amt_saga/score.py, amt_saga/roll.py); every edge, every search
// and every pixel is here.  The rule is amt_roll_core.h's.
//
// Design:
//  * the work item is one (image, pitch) of the image's pitch range; a workgroup of four waves takes items in a
//    grid-stride loop under a capped grid.  Every thread finds the item's ranges by binary search in the pitch-sorted
//    lists (the same answer in every lane), as the scoring kernel does.
//  * scan: the running maximum of end = max(off, on + 1) with its first index, over the item's notes of each side, 256
//    notes a step -- __shfl_up inside a wave, the four wave totals through LDS, a carry in registers -- into the caller's
//    scratch, indexed by the note's place in the call, so two items never meet.  Two barriers per 256 notes, none per
//    note.
//  * pixels: a thread owns columns tid, tid + 256, ...; per column two edges, one binary search per side for the last
//    note that began before the column's end, one read of the prefix: O(log notes) a pixel, no loop over the notes.
//    The row's W bytes go to LDS.
//  * rows: the pitch's row_px equal rows are adjacent in the image, so they are ONE run of row_px W bytes: bytes up to
//    the first 16-byte boundary, then 16-byte stores (read straight from LDS when W and the base are multiples of 16,
//    else gathered byte by byte with the index wrapping at W), then the last bytes.  Plain stores; every byte of an
//    image is written exactly once.
//  * integer code throughout, no atomics; no packed-FP32 instructions: any stream.
#include <limits.h>
#include "amt_launch.h"
#include "amt_roll_core.h"

#define ROLL_THREADS 256                  /* four waves */
#define ROLL_WAVES (ROLL_THREADS / AMT_WAVE)
/* Odd on purpose: the stride of the item loop is then no multiple of the 128 pitches, so a workgroup's items rotate
 * through the pitches and none is left with only the pitches outside an image's range. */
#define ROLL_MAX_GRID 2047

__device__ __forceinline__ score_i64 roll_clamp(score_i64 v, score_i64 lo, score_i64 hi) {
    return v < lo ? lo : (v > hi ? hi : v);
}

// roll_prefix_max by the whole workgroup: notes [s0, s1) of one pitch -> pmax, parg.  lds_m, lds_i: ROLL_WAVES entries.
__device__ __forceinline__ void roll_scan_segment(const score_notes &N, score_i64 s0, score_i64 s1, score_i64 *pmax,
                                                  int *parg, score_i64 *lds_m, int *lds_i) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    score_i64 carry_m = ROLL_I64_MIN;
    int carry_i = 0;
    for (score_i64 base = s0; base < s1; base += ROLL_THREADS) {          // (the same trip count in every thread)
        const score_i64 k = base + tid;
        const bool valid = k < s1;
        score_i64 m = valid ? roll_end(N.on[k], N.off[k]) : ROLL_I64_MIN;
        int at = valid ? (int)(k - s0) : 0;
#pragma unroll
        for (int off = 1; off < AMT_WAVE; off <<= 1) {
            score_i64 em = (score_i64)__shfl_up(m, off, AMT_WAVE);         // the earlier notes' maximum ...
            int ei = __shfl_up(at, off, AMT_WAVE);
            roll_max_combine(&em, &ei, m, at);                             // ... then this lane's
            if (lane >= off) { m = em; at = ei; }
        }
        __syncthreads();                                                   // (the last step's reads of lds are over)
        if (lane == AMT_WAVE - 1) { lds_m[w] = m; lds_i[w] = at; }
        __syncthreads();
        score_i64 run_m = carry_m, before_m = carry_m;
        int run_i = carry_i, before_i = carry_i;
#pragma unroll
        for (int i = 0; i < ROLL_WAVES; ++i) {
            if (i == w) { before_m = run_m; before_i = run_i; }
            roll_max_combine(&run_m, &run_i, lds_m[i], lds_i[i]);
        }
        carry_m = run_m;
        carry_i = run_i;
        roll_max_combine(&before_m, &before_i, m, at);
        if (valid) { pmax[k] = before_m; parg[k] = before_i; }
    }
}

__global__ __launch_bounds__(ROLL_THREADS) void roll_draw_kernel(
    score_notes E, score_notes G, const score_i64 *__restrict__ est_offsets, const score_i64 *__restrict__ gold_offsets,
    score_i64 n_est, score_i64 n_gold, const score_i64 *__restrict__ meta, const int32_t *__restrict__ group,
    roll_scratch S, score_i64 n_images, unsigned char *out, score_i64 out_bytes) {
    __shared__ __attribute__((aligned(16))) unsigned char row[ROLL_MAX_DIM];
    __shared__ int32_t grp[SCORE_PROGRAMS];
    __shared__ score_i64 lds_m[ROLL_WAVES];
    __shared__ int lds_i[ROLL_WAVES];
    const int tid = threadIdx.x;
    for (int k = tid; k < SCORE_PROGRAMS; k += ROLL_THREADS) grp[k] = group[k];
    const score_i64 items = n_images * SCORE_PITCHES;
    for (score_i64 item = blockIdx.x; item < items; item += gridDim.x) {
        const score_i64 image = item / SCORE_PITCHES;
        const int pitch = (int)(item % SCORE_PITCHES);
        score_i64 m[ROLL_META];
#pragma unroll
        for (int k = 0; k < ROLL_META; ++k) m[k] = meta[image * ROLL_META + k];
        // an image whose geometry or place is not what the host checked is left unwritten (the whole workgroup)
        if (!roll_geometry_ok(m) || pitch < m[ROLL_M_PITCH_LO] || pitch > m[ROLL_M_PITCH_HI]) continue;
        const score_i64 W = m[ROLL_M_W], px = m[ROLL_M_ROW_PX], t0 = m[ROLL_M_T0], span = m[ROLL_M_T1] - m[ROLL_M_T0];
        const score_i64 tick = m[ROLL_M_TICK], at = m[ROLL_M_OUT];
        const int pair = (int)m[ROLL_M_PAIR];
        if (at < 0 || at > out_bytes || W * roll_height(m) > out_bytes - at) continue;
        // the image's ranges, held inside the arrays whatever the offsets say; then the pitch's
        score_i64 e0, e1, g0 = 0, g1 = 0;
        {
            const score_i64 a = roll_clamp(est_offsets[image], 0, n_est), b = roll_clamp(est_offsets[image + 1], a, n_est);
            score_pitch_range(E.pitch, a, b, pitch, &e0, &e1);
            if (e1 - e0 > INT_MAX) e1 = e0 + INT_MAX;
        }
        if (pair) {
            const score_i64 a = roll_clamp(gold_offsets[image], 0, n_gold), b = roll_clamp(gold_offsets[image + 1], a, n_gold);
            score_pitch_range(G.pitch, a, b, pitch, &g0, &g1);
            if (g1 - g0 > INT_MAX) g1 = g0 + INT_MAX;
        }
        roll_scan_segment(E, e0, e1, S.pmax[0], S.parg[0], lds_m, lds_i);
        roll_scan_segment(G, g0, g1, S.pmax[1], S.parg[1], lds_m, lds_i);
        __syncthreads();              // the prefixes are written; the last item's reads of row are over; grp is filled
        for (score_i64 x = tid; x < W; x += ROLL_THREADS) {
            const score_i64 c0 = roll_edge(t0, span, W, x), c1 = roll_edge(t0, span, W, x + 1);
            const roll_hit est = roll_side(E, S.pmax[0], S.parg[0], e0, e1, c0, c1);
            roll_hit gold = {0, 0, 0};
            if (pair) gold = roll_side(G, S.pmax[1], S.parg[1], g0, g1, c0, c1);
            const int32_t g = (est.covered && !pair) ? grp[E.program[est.drawn] & (SCORE_PROGRAMS - 1)] : 0;
            row[x] = roll_pixel(pitch, roll_tick_hit(c0, c1, tick), pair, est, gold, g);
        }
        __syncthreads();
        // the pitch's row_px rows: one run of px * W bytes, byte k of it = row[k mod W]
        unsigned char *dst = out + at + (m[ROLL_M_PITCH_HI] - pitch) * px * W;
        const score_i64 len = px * W;
        score_i64 head = (score_i64)((16 - ((uintptr_t)dst & 15)) & 15);
        if (head > len) head = len;
        const score_i64 chunks = (len - head) / 16, tail_at = head + chunks * 16;
        for (score_i64 k = tid; k < head; k += ROLL_THREADS) dst[k] = row[k % W];
        for (score_i64 k = tail_at + tid; k < len; k += ROLL_THREADS) dst[k] = row[k % W];
        if (head == 0 && W % 16 == 0) {
            for (score_i64 q = tid; q < chunks; q += ROLL_THREADS)
                *(uint4 *)(dst + q * 16) = *(const uint4 *)(row + (q * 16) % W);
        } else {
            for (score_i64 q = tid; q < chunks; q += ROLL_THREADS) {
                score_i64 k = (head + q * 16) % W;
                uint32_t v[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    uint32_t word = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        word |= (uint32_t)row[k] << (8 * b);
                        k = k + 1 == W ? 0 : k + 1;
                    }
                    v[d] = word;
                }
                *(uint4 *)(dst + head + q * 16) = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

extern "C" {

long long amt_roll_scratch_bytes(long long n_est_total, long long n_gold_total) {
    roll_scratch S;
    const score_i64 need = roll_make_layout(nullptr, n_est_total, n_gold_total, &S);
    return need < 0 ? AMT_E_INVALID : need;
}

int amt_roll_draw(const amt_roll_args *a, void *stream) {
    if (!a || !a->est_pitch || !a->est_program || !a->est_on || !a->est_off || !a->gold_pitch || !a->gold_program ||
        !a->gold_on || !a->gold_off || !a->est_offsets_host || !a->gold_offsets_host || !a->est_offsets ||
        !a->gold_offsets || !a->image_meta_host || !a->image_meta || !a->group || !a->scratch ||
        ((uintptr_t)a->scratch & 15) || !a->out || a->n_images < 0 || a->n_images > ROLL_MAX_IMAGES ||
        a->scratch_bytes < 0 || a->out_bytes < 0)
        return AMT_E_INVALID;
    const long long *offs[2] = {(const long long *)a->est_offsets_host, (const long long *)a->gold_offsets_host};
    for (int s = 0; s < 2; ++s) {
        if (offs[s][0] < 0) return AMT_E_INVALID;
        for (long long i = 0; i < a->n_images; ++i) {
            const long long d = offs[s][i + 1] - offs[s][i];               // (both >= 0 once the first is: no overflow)
            if (offs[s][i + 1] < offs[s][i] || d > INT_MAX) return AMT_E_INVALID;
        }
    }
    for (long long i = 0; i < a->n_images; ++i) {
        const score_i64 *m = (const score_i64 *)a->image_meta_host + i * ROLL_META;
        if (!roll_geometry_ok(m) || m[ROLL_M_OUT] < 0 || m[ROLL_M_OUT] > a->out_bytes ||
            m[ROLL_M_W] * roll_height(m) > a->out_bytes - m[ROLL_M_OUT])
            return AMT_E_INVALID;
    }
    const score_i64 n_est = offs[0][a->n_images], n_gold = offs[1][a->n_images];
    roll_scratch S;
    const score_i64 need = roll_make_layout(a->scratch, n_est, n_gold, &S);
    if (need < 0) return AMT_E_INVALID;
    if (a->scratch_bytes < need) return AMT_E_SHAPE;
    if (a->n_images == 0) return AMT_OK;
    const score_notes E = {a->est_pitch, a->est_program, (const score_i64 *)a->est_on, (const score_i64 *)a->est_off};
    const score_notes G = {a->gold_pitch, a->gold_program, (const score_i64 *)a->gold_on, (const score_i64 *)a->gold_off};
    score_i64 grid = a->n_images * SCORE_PITCHES;
    if (grid > ROLL_MAX_GRID) grid = ROLL_MAX_GRID;
    roll_draw_kernel<<<(unsigned)grid, ROLL_THREADS, 0, (hipStream_t)stream>>>(
        E, G, (const score_i64 *)a->est_offsets, (const score_i64 *)a->gold_offsets, n_est, n_gold,
        (const score_i64 *)a->image_meta, a->group, S, a->n_images, a->out, a->out_bytes);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // extern "C"
