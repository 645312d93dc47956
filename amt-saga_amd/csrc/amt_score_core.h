// Scoring a transcription against gold notes: the rule, plain C++ behind one macro, so the same functions compile into
// the kernel of amt_score.hip and into a stand-alone CPU program (tests/score_host_main.cpp, built with the address and
// undefined-behaviour sanitizers).  Restated independently in tests/score_reference.py.  It stands where the reference's
// users reach for mir_eval.transcription on the MIDI/audio pairs the reference trains on (main.py:7).  DESIGN.md 27.
//
// TIMES   int64 microseconds, us = rint(seconds * 1e6), made on the host in float64.
// A PAIR  an estimated and a reference note list; a note is {pitch 0..127, program 0..127, on, off}; both lists sorted
//         by (pitch, on, off, program).
// MATCH   e matches r when e.pitch == r.pitch and |e.on - r.on| <= 50000, and
//           in the offset variants   |e.off - r.off| <= max(50000, (r.off - r.on) / 5), the quotient an integer
//                                    division, 0 when r.off <= r.on,
//           in the program variants  group[e.program] == group[r.program], group an int32 table of 128 entries.
//         (mir_eval.transcription's conventions: onset 50 ms, offset 20 % with a 50 ms floor; whole pitches make its
//         50-cent test an equality.)  Variant v = (offset ? 1 : 0) | (program ? 2 : 0).
// TRUE POSITIVES of a variant: the size of a MAXIMUM-cardinality matching of its bipartite graph -- unique whatever
//         finds it, and not what a first-fit pass gives.  Pitches never mix, so it is the sum over pitches.
// FRAMES  frame k >= 0 is the instant 10000 k us; cell (k, pitch) of a list is set when a note of that pitch has
//         on <= 10000 k < off (a note with off <= on sets none).  n_frames = #k with 10000 k below the largest off of
//         either list; frame_tp / fp / fn = popcounts of est & ref, est & ~ref, ~est & ref.
// OUTPUT  int64 [10] per pair: n_est, n_ref, tp_on, tp_onoff, tp_on_prog, tp_onoff_prog, frame_tp, frame_fp, frame_fn,
//         n_frames.
//
// How it is computed.  Per (pair, pitch): the candidates of reference r are the estimates with on in [r.on - 50000,
// r.on + 50000], a contiguous range [lo, hi) of the on-sorted list whose ends never move back from one r to the next
// (score_candidates, two binary searches).  score_max_matching is the augmenting-path algorithm with an explicit stack:
// owner, visited stamps and the stack are the caller's arrays, sized by the list, so neither a list's length nor a
// path's length is bounded by this file.  score_frames never builds a roll: the frames of a note are the integers
// [F(on), F(off)), F(t) = #k >= 0 with 10000 k < t, and one merge of the two on-sorted lists with three running
// maxima gives |est|, |ref| and |est or ref| as unions of such intervals; tp = |est| + |ref| - |est or ref|.
//
// Safety: every function works on the ranges it is handed.  Lists that are not sorted give other counts, never an
// index outside those ranges; the matcher ends after at most n_ref searches of at most n_est descents each.
#ifndef AMT_SCORE_CORE_H
#define AMT_SCORE_CORE_H
#include <stdint.h>
#include "amt_scratch.h"

#ifdef __HIP__
#define AMT_SCORE_HD __host__ __device__ inline
#else
#define AMT_SCORE_HD inline
#endif

#define SCORE_ONSET_TOL 50000          /* us */
#define SCORE_OFFSET_FLOOR 50000       /* us */
#define SCORE_OFFSET_DIV 5             /* 20 % of the reference's duration */
#define SCORE_FRAME_US 10000
#define SCORE_PITCHES 128
#define SCORE_PROGRAMS 128
#define SCORE_VARIANTS 4
#define SCORE_OUT 10                   /* int64 per pair */
#define SCORE_V_OFFSET 1
#define SCORE_V_PROGRAM 2

typedef long long score_i64;
typedef unsigned long long score_u64;

struct score_notes {                   /* one side of a call: four arrays, the notes of all pairs back to back */
    const int32_t *pitch, *program;
    const score_i64 *on, *off;
};

AMT_SCORE_HD int score_note_ok(int pitch, int program) {
    return pitch >= 0 && pitch < SCORE_PITCHES && program >= 0 && program < SCORE_PROGRAMS;
}

// |a - b| without signed overflow
AMT_SCORE_HD score_u64 score_dist(score_i64 a, score_i64 b) {
    return a > b ? (score_u64)a - (score_u64)b : (score_u64)b - (score_u64)a;
}

AMT_SCORE_HD score_u64 score_offset_tol(score_i64 r_on, score_i64 r_off) {
    const score_u64 part = r_off > r_on ? ((score_u64)r_off - (score_u64)r_on) / SCORE_OFFSET_DIV : 0;
    return part > SCORE_OFFSET_FLOOR ? part : SCORE_OFFSET_FLOOR;
}

// the rule of one edge; e and r index E and R; pitches are the caller's business (it hands one pitch's ranges)
AMT_SCORE_HD int score_edge(int variant, const score_notes &E, score_i64 e, const score_notes &R, score_i64 r,
                            const int32_t *group) {
    if (score_dist(E.on[e], R.on[r]) > SCORE_ONSET_TOL) return 0;
    if ((variant & SCORE_V_OFFSET) && score_dist(E.off[e], R.off[r]) > score_offset_tol(R.on[r], R.off[r])) return 0;
    if ((variant & SCORE_V_PROGRAM) &&
        group[E.program[e] & (SCORE_PROGRAMS - 1)] != group[R.program[r] & (SCORE_PROGRAMS - 1)])
        return 0;
    return 1;
}

// first i in [lo, hi) with a[i] >= v (hi if none); a ascending there
AMT_SCORE_HD score_i64 score_first_at_least_i32(const int32_t *a, score_i64 lo, score_i64 hi, int v) {
    while (lo < hi) {
        const score_i64 mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
AMT_SCORE_HD score_i64 score_first_at_least(const score_i64 *a, score_i64 lo, score_i64 hi, score_i64 v) {
    while (lo < hi) {
        const score_i64 mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first i in [lo, hi) with a[i] > v
AMT_SCORE_HD score_i64 score_first_above(const score_i64 *a, score_i64 lo, score_i64 hi, score_i64 v) {
    while (lo < hi) {
        const score_i64 mid = lo + (hi - lo) / 2;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the range of one pitch inside a pair's range [a, b) of a pitch-sorted list
AMT_SCORE_HD void score_pitch_range(const int32_t *pitch, score_i64 a, score_i64 b, int p, score_i64 *p0, score_i64 *p1) {
    *p0 = score_first_at_least_i32(pitch, a, b, p);
    *p1 = score_first_at_least_i32(pitch, *p0, b, p + 1);
}

// the estimates [e0, e1) of one pitch whose onset lies within the tolerance of r_on: [*lo, *hi), counted from e0
AMT_SCORE_HD void score_candidates(const score_i64 *e_on, score_i64 e0, score_i64 e1, score_i64 r_on, int *lo, int *hi) {
    const score_i64 min64 = (score_i64)(~(score_u64)0 >> 1) * -1 - 1, max64 = (score_i64)(~(score_u64)0 >> 1);
    const score_i64 low = r_on < min64 + SCORE_ONSET_TOL ? min64 : r_on - SCORE_ONSET_TOL;
    const score_i64 high = r_on > max64 - SCORE_ONSET_TOL ? max64 : r_on + SCORE_ONSET_TOL;
    const score_i64 l = score_first_at_least(e_on, e0, e1, low);
    *lo = (int)(l - e0);
    *hi = (int)(score_first_above(e_on, l, e1, high) - e0);
}

// Maximum matching of one pitch's graph by augmenting paths; returns its size.  References 0 .. nr - 1 are searched
// from in turn; estimates are named by their index in the pitch's list.  owner[e] (the reference that holds e, -1 at
// entry) and visited[e] (0 at entry; the search that last descended through e) have one entry per estimate;
// stack_ref and stack_via one per reference.  scan(r, stamp, &free_e, &next_e) looks through r's candidates that
// match and have visited != stamp: free_e = one with owner < 0 if there is any, else next_e = one that is held (each
// -1 if none).  A search from r0 walks r0 -> e -> owner[e] -> ... ; on a free estimate the path is flipped from the
// stack.  A reference enters the stack at most once per search (its estimate is stamped on the way in), so the depth
// stays below nr; a frame that is returned to is scanned again, the stamps skipping what it has tried.
template <class Scan>
AMT_SCORE_HD int score_max_matching(int nr, int *owner, int *visited, int *stack_ref, int *stack_via, Scan scan) {
    int size = 0;
    for (int r0 = 0; r0 < nr; ++r0) {
        const int stamp = r0 + 1;
        int depth = 0, r = r0;
        stack_ref[0] = r0;
        stack_via[0] = -1;
        while (depth >= 0) {
            int free_e = -1, next_e = -1;
            scan(r, stamp, &free_e, &next_e);
            if (free_e >= 0) {
                int e = free_e;
                owner[e] = r;
                e = stack_via[depth];
                for (int d = depth - 1; d >= 0; --d) {
                    owner[e] = stack_ref[d];
                    e = stack_via[d];
                }
                ++size;
                break;
            }
            if (next_e >= 0 && depth + 1 < nr) {
                visited[next_e] = stamp;
                r = owner[next_e];
                ++depth;
                stack_ref[depth] = r;
                stack_via[depth] = next_e;
            } else {
                --depth;
                if (depth >= 0) r = stack_ref[depth];
            }
        }
    }
    return size;
}

// F(t): the number of k >= 0 with 10000 k < t
AMT_SCORE_HD score_i64 score_frames_below(score_i64 t) { return t <= 0 ? 0 : (t - 1) / SCORE_FRAME_US + 1; }

// Frame counts of one pitch: estimates [e0, e1) and references [r0, r1), each sorted by on.  count[0 .. 2] = frame_tp,
// frame_fp, frame_fn; *max_off = the largest off of either range (0 if none is positive).
AMT_SCORE_HD void score_frames(const score_notes &E, score_i64 e0, score_i64 e1, const score_notes &R, score_i64 r0,
                               score_i64 r1, score_i64 *count, score_i64 *max_off) {
    score_i64 i = e0, j = r0, end_e = 0, end_r = 0, end_u = 0, n_e = 0, n_r = 0, n_u = 0, top = 0;
    while (i < e1 || j < r1) {
        const bool est = j >= r1 || (i < e1 && E.on[i] <= R.on[j]);
        const score_i64 on = est ? E.on[i] : R.on[j], off = est ? E.off[i] : R.off[j];
        if (est) ++i; else ++j;
        if (off > top) top = off;
        const score_i64 a = score_frames_below(on), b = score_frames_below(off);
        if (b <= a) continue;
        score_i64 &end_s = est ? end_e : end_r, &n_s = est ? n_e : n_r;
        const score_i64 from_s = a > end_s ? a : end_s, from_u = a > end_u ? a : end_u;
        if (b > from_s) { n_s += b - from_s; end_s = b; }
        if (b > from_u) { n_u += b - from_u; end_u = b; }
    }
    const score_i64 tp = n_e + n_r - n_u;
    count[0] = tp;
    count[1] = n_e - tp;
    count[2] = n_r - tp;
    *max_off = top;
}

// The scratch of amt_score_pairs, every array on a 16-byte boundary of the buffer and indexed by the note's place in the
// call: the candidate ranges, then per variant the matcher's arrays.  16 bytes of slack close it, as they always have.
#define SCORE_MAX_NOTES ((score_i64)1 << 40)                   /* per side and call: the scratch stays far inside int64 */
struct score_scratch {
    int *lo, *hi;                                              // [n_ref]: a reference's candidates, from its pitch's first
    int *owner[SCORE_VARIANTS], *visited[SCORE_VARIANTS];      // [n_est]
    int *stack_ref[SCORE_VARIANTS], *stack_via[SCORE_VARIANTS];// [n_ref]
};
inline score_i64 score_make_layout(void *scratch, score_i64 n_est, score_i64 n_ref, score_scratch *S) {
    if (n_est > SCORE_MAX_NOTES || n_ref > SCORE_MAX_NOTES) return -1;
    amt_carver c(scratch);
    S->lo = c.take<int>(n_ref, 16);
    S->hi = c.take<int>(n_ref, 16);
    for (int v = 0; v < SCORE_VARIANTS; ++v) {
        S->owner[v] = c.take<int>(n_est, 16);
        S->visited[v] = c.take<int>(n_est, 16);
        S->stack_ref[v] = c.take<int>(n_ref, 16);
        S->stack_via[v] = c.take<int>(n_ref, 16);
    }
    c.take<unsigned char>(16, 16);
    return c.failed ? -1 : c.at;
}

#endif
