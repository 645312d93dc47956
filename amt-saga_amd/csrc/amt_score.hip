// Scoring transcriptions against gold notes on the device for gfx950: any number of (estimate, reference) pairs in one
// launch -> ten integer counts per pair (note true positives of the four matching variants as MAXIMUM matchings, frame
// true / false positives and false negatives, the totals).
//
// Stands where the reference's users would call mir_eval.transcription on the MIDI/audio pairs the reference trains on
// (main.py:7), which builds an n_ref x n_est matrix per song on the host.  The host sorts and packs (amt_saga/score.py);
// every comparison, every matching and every frame count is here.  The rule is amt_score_core.h's.
//
// Design:
//  * the work item is one (pair, pitch); a workgroup of five waves takes items in a grid-stride loop.  Every thread
//    finds the item's two ranges by binary search in the pitch-sorted lists (the same answer in every lane).
//  * all threads: owner = -1 and visited = 0 for the item's estimates, in the four variants' arrays; a reference per
//    thread: its candidate range [lo, hi) by two binary searches in the on-sorted estimates.
//  * waves 0 .. 3: one variant each, score_max_matching with the candidates of a reference spread over the lanes -- 64
//    at a time, matched and not yet visited, __ballot (64-bit) picks a free one, else a held one.  What the search
//    writes (owner, visited, the stack) is written by every lane with the same value: a lane only ever reads what it
//    has itself stored, so no fence stands between a store and the load that follows it.
//  * wave 4, one lane: score_frames, the merge of the two lists.
//  * owner, visited and the stack live in the caller's scratch, indexed by the note's place in the call, so the ranges of
//    two items never meet and a workgroup may begin its next item while a wave still finishes the last.
//  * a lane per wave adds its count to the pair's row with 64-bit integer atomics (a sum and a maximum of integers: the
//    same in any order); the row is zeroed by the call before the launch.
//  * integer code throughout; no packed-FP32 instructions: any stream.
#include <limits.h>
#include "amt_launch.h"
#include "amt_score_core.h"

#define SCORE_THREADS 320                 /* five waves */
#define SCORE_MAX_GRID (1 << 16)

// the candidates of r over the lanes of a wave
struct score_wave_scan {
    const score_notes &E, &R;
    const int32_t *group;
    const int *lo, *hi, *owner, *visited;                      // from the pitch's first reference / estimate
    score_i64 e0, r0;
    int variant, lane;
    __device__ void operator()(int r, int stamp, int *free_e, int *next_e) const {
        const int a = lo[r], b = hi[r];
        for (int base = a; base < b; base += AMT_WAVE) {
            const int e = base + lane;
            const bool ok = e < b && visited[e] != stamp && score_edge(variant, E, e0 + e, R, r0 + r, group);
            const bool is_free = ok && owner[e] < 0;
            const unsigned long long free_mask = __ballot(is_free);
            if (free_mask) {
                *free_e = base + __ffsll(free_mask) - 1;
                return;
            }
            const unsigned long long held_mask = __ballot(ok);
            if (held_mask && *next_e < 0) *next_e = base + __ffsll(held_mask) - 1;
        }
    }
};

__device__ __forceinline__ score_i64 score_clamp(score_i64 v, score_i64 lo, score_i64 hi) {
    return v < lo ? lo : (v > hi ? hi : v);
}

__global__ __launch_bounds__(SCORE_THREADS) void score_pairs_kernel(
    score_notes E, score_notes R, const score_i64 *__restrict__ est_offsets, const score_i64 *__restrict__ ref_offsets,
    score_i64 n_est, score_i64 n_ref, const int32_t *__restrict__ group, score_scratch S, score_i64 n_pairs,
    unsigned long long *out) {
    __shared__ int32_t grp[SCORE_PROGRAMS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int k = tid; k < SCORE_PROGRAMS; k += SCORE_THREADS) grp[k] = group[k];
    __syncthreads();
    const score_i64 items = n_pairs * SCORE_PITCHES;
    for (score_i64 item = blockIdx.x; item < items; item += gridDim.x) {
        const score_i64 pair = item / SCORE_PITCHES;
        const int pitch = (int)(item % SCORE_PITCHES);
        // the pair's ranges, held inside the arrays whatever the offsets say
        const score_i64 ea = score_clamp(est_offsets[pair], 0, n_est), eb = score_clamp(est_offsets[pair + 1], ea, n_est);
        const score_i64 ra = score_clamp(ref_offsets[pair], 0, n_ref), rb = score_clamp(ref_offsets[pair + 1], ra, n_ref);
        score_i64 e0, e1, r0, r1;
        score_pitch_range(E.pitch, ea, eb, pitch, &e0, &e1);
        score_pitch_range(R.pitch, ra, rb, pitch, &r0, &r1);
        if (e1 - e0 > INT_MAX) e1 = e0 + INT_MAX;
        if (r1 - r0 > INT_MAX) r1 = r0 + INT_MAX;
        const int ne = (int)(e1 - e0), nr = (int)(r1 - r0);
        if (ne == 0 && nr == 0) continue;                                  // (the whole workgroup)
        const bool match = ne > 0 && nr > 0;
        if (match) {
            for (int k = tid; k < ne; k += SCORE_THREADS) {
#pragma unroll
                for (int v = 0; v < SCORE_VARIANTS; ++v) {
                    S.owner[v][e0 + k] = -1;
                    S.visited[v][e0 + k] = 0;
                }
            }
            for (int k = tid; k < nr; k += SCORE_THREADS)
                score_candidates(E.on, e0, e1, R.on[r0 + k], &S.lo[r0 + k], &S.hi[r0 + k]);
        }
        __syncthreads();
        unsigned long long *row = out + pair * SCORE_OUT;
        if (wave < SCORE_VARIANTS) {
            if (match) {
                const score_wave_scan scan = {E, R, grp, S.lo + r0, S.hi + r0, S.owner[wave] + e0, S.visited[wave] + e0,
                                              e0, r0, wave, lane};
                const int size = score_max_matching(nr, S.owner[wave] + e0, S.visited[wave] + e0, S.stack_ref[wave] + r0,
                                                    S.stack_via[wave] + r0, scan);
                if (lane == 0 && size) atomicAdd(row + 2 + wave, (unsigned long long)size);
            }
        } else if (lane == 0) {
            score_i64 count[3], top;
            score_frames(E, e0, e1, R, r0, r1, count, &top);
            if (ne) atomicAdd(row + 0, (unsigned long long)ne);
            if (nr) atomicAdd(row + 1, (unsigned long long)nr);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (count[k]) atomicAdd(row + 6 + k, (unsigned long long)count[k]);
            atomicMax(row + 9, (unsigned long long)score_frames_below(top));
        }
    }
}

extern "C" {

long long amt_score_scratch_bytes(long long n_est_total, long long n_ref_total) {
    score_scratch S;
    const score_i64 need = score_make_layout(nullptr, n_est_total, n_ref_total, &S);
    return need < 0 ? AMT_E_INVALID : need;
}

int amt_score_check_notes(const int32_t *pitch, const int32_t *program, long long n) {
    if (n < 0 || (n > 0 && (!pitch || !program))) return AMT_E_INVALID;
    for (long long i = 0; i < n; ++i)
        if (!score_note_ok(pitch[i], program[i])) return AMT_E_INVALID;
    return AMT_OK;
}

int amt_score_pairs(const amt_score_args *a, void *stream) {
    if (!a || !a->est_pitch || !a->est_program || !a->est_on || !a->est_off || !a->ref_pitch || !a->ref_program ||
        !a->ref_on || !a->ref_off || !a->est_offsets_host || !a->ref_offsets_host || !a->est_offsets || !a->ref_offsets ||
        !a->group || !a->scratch || ((uintptr_t)a->scratch & 15) || !a->out || a->n_pairs < 0 ||
        a->n_pairs > SCORE_MAX_NOTES / SCORE_PITCHES || a->scratch_bytes < 0)
        return AMT_E_INVALID;
    const long long *offs[2] = {(const long long *)a->est_offsets_host, (const long long *)a->ref_offsets_host};
    for (int s = 0; s < 2; ++s) {
        if (offs[s][0] < 0) return AMT_E_INVALID;
        for (long long i = 0; i < a->n_pairs; ++i) {
            const long long d = offs[s][i + 1] - offs[s][i];               // (both >= 0 once the first is: no overflow)
            if (offs[s][i + 1] < offs[s][i] || d > INT_MAX) return AMT_E_INVALID;
        }
    }
    const score_i64 n_est = offs[0][a->n_pairs], n_ref = offs[1][a->n_pairs];
    score_scratch S;
    const score_i64 need = score_make_layout(a->scratch, n_est, n_ref, &S);
    if (need < 0) return AMT_E_INVALID;
    if (a->scratch_bytes < need) return AMT_E_SHAPE;
    if (a->n_pairs == 0) return AMT_OK;
    hipStream_t st = (hipStream_t)stream;
    const score_notes E = {a->est_pitch, a->est_program, (const score_i64 *)a->est_on, (const score_i64 *)a->est_off};
    const score_notes R = {a->ref_pitch, a->ref_program, (const score_i64 *)a->ref_on, (const score_i64 *)a->ref_off};
    AMT_HIP_CHECK(hipMemsetAsync(a->out, 0, (size_t)a->n_pairs * SCORE_OUT * sizeof(int64_t), st));
    score_i64 grid = a->n_pairs * SCORE_PITCHES;
    if (grid > SCORE_MAX_GRID) grid = SCORE_MAX_GRID;
    score_pairs_kernel<<<(unsigned)grid, SCORE_THREADS, 0, st>>>(
        E, R, (const score_i64 *)a->est_offsets, (const score_i64 *)a->ref_offsets, n_est, n_ref, a->group, S, a->n_pairs,
        (unsigned long long *)a->out);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // extern "C"
