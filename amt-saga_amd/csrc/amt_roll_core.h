// Piano-roll images of note lists: the rule, plain C++ behind one macro, so the same functions compile into the kernel of
// amt_roll.hip and into a stand-alone CPU program (tests/roll_host_main.cpp, built with the address and undefined-
// behaviour sanitizers).  Restated independently in tests/roll_reference.py.  It stands where the reference's users
// reach for a piano-roll plot of the MIDI/audio pairs the reference trains on (main.py:7).  DESIGN.md 29.
//
// AN IMAGE  int64 [ROLL_META]: W, row_px, pitch_lo, pitch_hi, t0, t1, tick, pair, first output byte, reserved.
//           W in 1..16384; 0 <= pitch_lo <= pitch_hi <= 127; row_px >= 1 and H = (pitch_hi - pitch_lo + 1) row_px <=
//           16384; W <= t1 - t0 <= 2^40 and |t0| <= 2^61, so x (t1 - t0) stays inside int64; tick in 0..2^40 (0: none);
//           pair 0 (one list) or 1 (estimate against gold).  Times are int64 microseconds; the lists are score.pack's:
//           sorted by (pitch, on, off, program).
// COLUMNS   edges c_x = t0 + floor(x (t1 - t0) / W), x = 0..W, strictly increasing; column x is [c_x, c_{x+1}).
// ROWS      pitch p owns pixel rows (pitch_hi - p) row_px .. + row_px - 1, all equal; other pitches are not drawn.
// A NOTE    covers [on, end), end = max(off, on + 1): column x iff on < c_{x+1} and end > c_x; its onset is in column x
//           iff c_x <= on < c_{x+1}.
// ONE SIDE  at (p, x): j = the last note of pitch p, in sorted order, with on < c_{x+1}.  None: nothing.  onset =
//           on_j >= c_x; covered = max_{i <= j} end_i > c_x; the drawn note is j if end_j > c_x, else the first i <= j
//           that attains the maximum.
// PIXEL     background (no side covered): 0 on a white-key row, 1 on a black-key row (p mod 12 in {1, 3, 6, 8, 10}),
//           + 2 if tick > 0 and the column holds a multiple of tick: floor((c_{x+1} - 1) / tick) >= ceil(c_x / tick),
//           mathematical floor and ceiling.  One list: 16 + 2 (group[program of the drawn note] mod 16) + onset.
//           Pair: 64 + 4 (est_covered | 2 gold_covered) + est_onset + 2 gold_onset.
//
// How it is computed.  The running maximum of end with its first index, per (image, side, pitch), is made once
// (roll_prefix_max here, a workgroup scan with the same roll_max_combine in the kernel); a pixel is then one binary
// search for j and one read of the prefix: no loop over a row's notes per pixel.
//
// Safety: every function works on the ranges it is handed.  Lists that are not sorted give other pixels, never an index
// outside those ranges.
#ifndef AMT_ROLL_CORE_H
#define AMT_ROLL_CORE_H
#include <stdint.h>
#include "amt_score_core.h"

#define AMT_ROLL_HD AMT_SCORE_HD

#define ROLL_META 10                                   /* int64 per image */
#define ROLL_M_W 0
#define ROLL_M_ROW_PX 1
#define ROLL_M_PITCH_LO 2
#define ROLL_M_PITCH_HI 3
#define ROLL_M_T0 4
#define ROLL_M_T1 5
#define ROLL_M_TICK 6
#define ROLL_M_PAIR 7
#define ROLL_M_OUT 8
#define ROLL_MAX_DIM 16384
#define ROLL_MAX_SPAN ((score_i64)1 << 40)
#define ROLL_MAX_T0 ((score_i64)1 << 61)
#define ROLL_MAX_TICK ((score_i64)1 << 40)
#define ROLL_MAX_IMAGES ((score_i64)1 << 24)           /* per call */
#define ROLL_I64_MIN ((score_i64)(~(score_u64)0 >> 1) * -1 - 1)
#define ROLL_I64_MAX ((score_i64)(~(score_u64)0 >> 1))

#define ROLL_BACKGROUND 0                              /* + 1 black-key row, + 2 tick */
#define ROLL_SINGLE 16                                 /* + 2 (group mod 16) + onset */
#define ROLL_PAIR 64                                   /* + 4 class + est_onset + 2 gold_onset */

// the geometry of one image; the output place is the caller's to check against its buffer
AMT_ROLL_HD int roll_geometry_ok(const score_i64 *m) {
    const score_i64 W = m[ROLL_M_W], px = m[ROLL_M_ROW_PX], lo = m[ROLL_M_PITCH_LO], hi = m[ROLL_M_PITCH_HI];
    const score_i64 t0 = m[ROLL_M_T0], t1 = m[ROLL_M_T1], tick = m[ROLL_M_TICK], pair = m[ROLL_M_PAIR];
    if (W < 1 || W > ROLL_MAX_DIM || lo < 0 || hi < lo || hi >= SCORE_PITCHES) return 0;
    if (px < 1 || px > ROLL_MAX_DIM || (hi - lo + 1) * px > ROLL_MAX_DIM) return 0;
    if (t0 < -ROLL_MAX_T0 || t0 > ROLL_MAX_T0 || t1 <= t0 || t1 - t0 < W || t1 - t0 > ROLL_MAX_SPAN) return 0;
    if (tick < 0 || tick > ROLL_MAX_TICK || (pair != 0 && pair != 1)) return 0;
    return 1;
}
AMT_ROLL_HD score_i64 roll_height(const score_i64 *m) {
    return (m[ROLL_M_PITCH_HI] - m[ROLL_M_PITCH_LO] + 1) * m[ROLL_M_ROW_PX];
}

// c_x, x in 0..W: x span <= 2^14 2^40 and is not negative, so the quotient is the floor
AMT_ROLL_HD score_i64 roll_edge(score_i64 t0, score_i64 span, score_i64 W, score_i64 x) { return t0 + x * span / W; }

// floor(a / b) and ceil(a / b) for b > 0, also for a < 0
AMT_ROLL_HD score_i64 roll_floor_div(score_i64 a, score_i64 b) {
    const score_i64 q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
AMT_ROLL_HD score_i64 roll_ceil_div(score_i64 a, score_i64 b) {
    const score_i64 q = a / b;
    return (a % b != 0 && a > 0) ? q + 1 : q;
}
// does [c0, c1) hold a multiple of tick?  (c1 > c0 >= -2^61: c1 - 1 does not wrap)
AMT_ROLL_HD int roll_tick_hit(score_i64 c0, score_i64 c1, score_i64 tick) {
    return tick > 0 && roll_floor_div(c1 - 1, tick) >= roll_ceil_div(c0, tick);
}

// max(off, on + 1); score.pack keeps times below 2^62, the last value of int64 stays itself
AMT_ROLL_HD score_i64 roll_end(score_i64 on, score_i64 off) {
    return off > on ? off : (on < ROLL_I64_MAX ? on + 1 : on);
}

// the running maximum with its first index: (m, i) of earlier notes, then (bm, bi) of later ones; ties stay early
AMT_ROLL_HD void roll_max_combine(score_i64 *m, int *i, score_i64 bm, int bi) {
    if (bm > *m) { *m = bm; *i = bi; }
}

// One after the other, what the kernel's workgroup scan makes: for the notes [s0, s1) of one pitch, pmax[k] = the
// largest end of s0 .. k and parg[k] = the first index, counted from s0, that attains it.  pmax and parg are indexed
// like the notes.
AMT_ROLL_HD void roll_prefix_max(const score_notes &N, score_i64 s0, score_i64 s1, score_i64 *pmax, int *parg) {
    score_i64 m = ROLL_I64_MIN;
    int at = 0;
    for (score_i64 k = s0; k < s1; ++k) {
        roll_max_combine(&m, &at, roll_end(N.on[k], N.off[k]), (int)(k - s0));
        pmax[k] = m;
        parg[k] = at;
    }
}

struct roll_hit {
    int covered, onset;
    score_i64 drawn;                                   // the drawn note's index in N; meaningful when covered
};

// one side at column [c0, c1) of the pitch whose notes are [s0, s1)
AMT_ROLL_HD roll_hit roll_side(const score_notes &N, const score_i64 *pmax, const int *parg, score_i64 s0, score_i64 s1,
                               score_i64 c0, score_i64 c1) {
    roll_hit h = {0, 0, s0};
    const score_i64 j = score_first_at_least(N.on, s0, s1, c1) - 1;
    if (j < s0) return h;
    h.onset = N.on[j] >= c0;
    h.covered = pmax[j] > c0;
    if (roll_end(N.on[j], N.off[j]) > c0) {
        h.drawn = j;
    } else {
        score_i64 first = s0 + parg[j];                // (held inside [s0, j] whatever the scratch says)
        h.drawn = first < s0 ? s0 : (first > j ? j : first);
    }
    return h;
}

AMT_ROLL_HD int roll_black_key(int pitch) {
    const int k = pitch % 12;
    return k == 1 || k == 3 || k == 6 || k == 8 || k == 10;
}

// The pixel.  gold is looked at in pair mode only; group_of_drawn = group[program of the estimate's drawn note] and is
// looked at only when the estimate is covered in single mode.
AMT_ROLL_HD unsigned char roll_pixel(int pitch, int tick_hit, int pair, const roll_hit &est, const roll_hit &gold,
                                     int32_t group_of_drawn) {
    const int cls = (est.covered ? 1 : 0) | (pair && gold.covered ? 2 : 0);
    if (!cls) return (unsigned char)(ROLL_BACKGROUND + roll_black_key(pitch) + (tick_hit ? 2 : 0));
    if (!pair) return (unsigned char)(ROLL_SINGLE + 2 * (int)((uint32_t)group_of_drawn & 15u) + (est.onset ? 1 : 0));
    return (unsigned char)(ROLL_PAIR + 4 * cls + (est.onset ? 1 : 0) + (gold.onset ? 2 : 0));
}

// The scratch of amt_roll_draw, every array on a 16-byte boundary and indexed by the note's place in the call, per side
// (0 the estimates, 1 the gold notes): the running maximum and its first index.  16 bytes of slack close it.
struct roll_scratch {
    score_i64 *pmax[2];
    int *parg[2];
};
inline score_i64 roll_make_layout(void *scratch, score_i64 n_est, score_i64 n_gold, roll_scratch *S) {
    if (n_est < 0 || n_gold < 0 || n_est > SCORE_MAX_NOTES || n_gold > SCORE_MAX_NOTES) return -1;
    amt_carver c(scratch);
    const score_i64 n[2] = {n_est, n_gold};
    for (int s = 0; s < 2; ++s) {
        S->pmax[s] = c.take<score_i64>(n[s], 16);
        S->parg[s] = c.take<int>(n[s], 16);
    }
    c.take<unsigned char>(16, 16);
    return c.failed ? -1 : c.at;
}

#endif
