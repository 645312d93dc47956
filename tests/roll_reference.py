"""The piano-roll rule of csrc/amt_roll_core.h, restated independently: Python integers and numpy int64, no
code shared with the package.  A note is the tuple (pitch, program, on, off) of tests/score_reference.py, times in
microseconds.  A case is a dict: name, est, gold (None: a single list; a list, even an empty one: a pair), W, row_px,
pitch_lo, pitch_hi, t0, t1, tick, group.

pixel_slow is the rule word by word -- `covered` by looking at every note of the pitch -- for small images; draw is the
same rule with numpy's searchsorted and maximum.accumulate, for the large ones.  test_roll_cpu.py holds them equal on
every small case and holds both to answers drawn by hand (EXPECTED)."""
import numpy as np

MAX_DIM = 16384
MAX_SPAN = 2 ** 40
MAX_T0 = 2 ** 61
MAX_TICK = 2 ** 40
BLACK = (1, 3, 6, 8, 10)
IDENTITY = list(range(128))
# the three instrument groups of the transcription loop: guitars 24-31, strings and ensembles 40-55, the rest
MERGED = [2 if 24 <= p <= 31 else (1 if 40 <= p <= 55 else 0) for p in range(128)]
SINGLE, PAIR = 16, 64
THREADS = 256                                          # the kernel's workgroup (ROLL_THREADS)
GRID_CAP = 2047                                        # ... and its grid cap (ROLL_MAX_GRID)


def sort_key(n):
    return (n[0], n[2], n[3], n[1])


def case(name, est, gold=None, W=8, row_px=1, lo=0, hi=127, t0=0, t1=None, tick=0, group=IDENTITY):
    return dict(name=name, est=list(est), gold=None if gold is None else list(gold), W=W, row_px=row_px, pitch_lo=lo,
                pitch_hi=hi, t0=t0, t1=t0 + 1000 * W if t1 is None else t1, tick=tick, group=list(group))


def height(c):
    return (c['pitch_hi'] - c['pitch_lo'] + 1) * c['row_px']


def inside_limits(c):
    """The geometry limits of the rule, and notes the packer takes."""
    span = c['t1'] - c['t0']
    ok = 1 <= c['W'] <= MAX_DIM and 0 <= c['pitch_lo'] <= c['pitch_hi'] <= 127 and c['row_px'] >= 1
    ok = ok and height(c) <= MAX_DIM and c['W'] <= span <= MAX_SPAN and abs(c['t0']) <= MAX_T0
    ok = ok and 0 <= c['tick'] <= MAX_TICK and len(c['group']) == 128
    for n in c['est'] + (c['gold'] or []):
        ok = ok and 0 <= n[0] <= 127 and 0 <= n[1] <= 127 and abs(n[2]) < 2 ** 61 and abs(n[3]) < 2 ** 61
    return bool(ok)


def edges(c):
    return [c['t0'] + x * (c['t1'] - c['t0']) // c['W'] for x in range(c['W'] + 1)]


def tick_hit(c0, c1, tick):
    """Does [c0, c1) hold a multiple of tick?  Python's // is the mathematical floor."""
    return tick > 0 and (c1 - 1) // tick >= -((-c0) // tick)


def background(p, c0, c1, tick):
    return (1 if p % 12 in BLACK else 0) + (2 if tick_hit(c0, c1, tick) else 0)


def side_slow(notes, p, c0, c1):
    """(covered, onset, drawn note or None) of one side at pitch p and column [c0, c1): the rule read literally."""
    ns = sorted((n for n in notes if n[0] == p), key=sort_key)
    end = [max(n[3], n[2] + 1) for n in ns]
    started = [i for i, n in enumerate(ns) if n[2] < c1]
    if not started:
        assert not any(n[2] < c1 and e > c0 for n, e in zip(ns, end))
        return False, False, None
    j = started[-1]
    covered = any(n[2] < c1 and e > c0 for n, e in zip(ns, end))       # "some note covers the column"
    top = max(end[:j + 1])
    assert covered == (top > c0)                                       # ... which is the prefix maximum's test
    onset = ns[j][2] >= c0
    drawn = ns[j] if end[j] > c0 else ns[end.index(top)]
    return covered, onset, drawn


def pixel_slow(c, p, x, e=None):
    e = edges(c) if e is None else e
    c0, c1 = e[x], e[x + 1]
    ec, eo, ed = side_slow(c['est'], p, c0, c1)
    if c['gold'] is None:
        if not ec:
            return background(p, c0, c1, c['tick'])
        return SINGLE + 2 * (c['group'][ed[1]] % 16) + int(eo)
    gc, go, _ = side_slow(c['gold'], p, c0, c1)
    if not (ec or gc):
        return background(p, c0, c1, c['tick'])
    return PAIR + 4 * (int(ec) | 2 * int(gc)) + int(eo) + 2 * int(go)


def draw_slow(c):
    e = edges(c)
    rows = []
    for p in range(c['pitch_hi'], c['pitch_lo'] - 1, -1):
        row = [pixel_slow(c, p, x, e) for x in range(c['W'])]
        rows += [row] * c['row_px']
    return np.array(rows, dtype=np.uint8).reshape(height(c), c['W'])


def _by_pitch(notes):
    out = {}
    for n in sorted(notes, key=sort_key):
        out.setdefault(n[0], []).append(n)
    return out


def _side_fast(ns, e):
    """covered, onset (bool [W]) and the drawn note's program (int64 [W]) from one pitch's sorted notes."""
    W = len(e) - 1
    if not ns:
        z = np.zeros(W, dtype=bool)
        return z, z, np.zeros(W, dtype=np.int64)
    a = np.array(ns, dtype=np.int64).reshape(len(ns), 4)
    on, program = a[:, 2], a[:, 1]
    end = np.maximum(a[:, 3], on + 1)
    top = np.maximum.accumulate(end)
    fresh = np.concatenate([[True], end[1:] > top[:-1]])
    first = np.maximum.accumulate(np.where(fresh, np.arange(len(ns)), 0))
    c0, c1 = e[:-1], e[1:]
    j = np.searchsorted(on, c1, side='left') - 1
    has = j >= 0
    j = np.maximum(j, 0)
    onset = has & (on[j] >= c0)
    covered = has & (top[j] > c0)
    drawn = np.where(end[j] > c0, j, first[j])
    return covered, onset, program[drawn]


def draw(c):
    """uint8 [H, W]: the image of the case."""
    e = np.array(edges(c), dtype=np.int64)
    c0, c1 = e[:-1], e[1:]
    tick = c['tick']
    ticks = ((c1 - 1) // tick >= -((-c0) // tick)) if tick > 0 else np.zeros(c['W'], dtype=bool)
    group = np.asarray(c['group'], dtype=np.int64)
    est, gold = _by_pitch(c['est']), _by_pitch(c['gold'] or [])
    rows = []
    for p in range(c['pitch_hi'], c['pitch_lo'] - 1, -1):
        back = (1 if p % 12 in BLACK else 0) + 2 * ticks.astype(np.int64)
        ec, eo, prog = _side_fast(est.get(p, []), e)
        if c['gold'] is None:
            row = np.where(ec, SINGLE + 2 * (group[prog] % 16) + eo, back)
        else:
            gc, go, _ = _side_fast(gold.get(p, []), e)
            row = np.where(ec | gc, PAIR + 4 * (ec + 2 * gc.astype(np.int64)) + eo + 2 * go, back)
        rows.append(row.astype(np.uint8))
    return np.repeat(np.stack(rows), c['row_px'], axis=0)


def class_counts(img):
    """(both, estimate only, gold only) pixel counts of a pair image."""
    cls = np.where(img >= PAIR, (img.astype(np.int64) - PAIR) // 4, 0)
    return [int((cls == 3).sum()), int((cls == 1).sum()), int((cls == 2).sum())]


def grid_case(name, est, gold, frame_us=10000):
    """The image whose class counts are the frame counts of the scoring rule: a column per frame, every pitch."""
    top = max([n[3] for n in est + gold] + [0])
    n_frames = max(1, 0 if top <= 0 else (top - 1) // frame_us + 1)
    return case(name, est, gold, W=n_frames, t0=0, t1=frame_us * n_frames)


def grid_pairs(count, seed, pitches=(60, 61, 62, 72), most=14, frames=120):
    """Seeded random pairs with every time on the 10 ms grid and every note at least a frame long (a note with off <= on
    is a visible microsecond here and no frame of the scoring rule)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        sides = []
        for _s in range(2):
            notes = []
            for _k in range(int(rng.integers(0, most + 1))):
                on = int(rng.integers(0, frames)) * 10000
                notes.append((int(rng.choice(pitches)), int(rng.integers(0, 128)), on,
                              on + int(rng.integers(1, 30)) * 10000))
            sides.append(notes)
        out.append(tuple(sides))
    return out


def random_notes(rng, n, lo, hi, t0, t1, longest=None):
    span = t1 - t0
    longest = max(2, span // 4) if longest is None else longest
    notes = []
    for _ in range(n):
        on = int(rng.integers(t0 - span // 8, t1 + span // 8))
        notes.append((int(rng.integers(lo, hi + 1)), int(rng.integers(0, 128)), on,
                      on + int(rng.integers(-3, longest))))
    return notes


FOLD = [16 + (7 * p) % 112 for p in range(128)]        # every group above 15


def by_hand():
    """The cases whose images are written out in EXPECTED."""
    edge_notes = [(60, 0, 1000, 1500),                 # on == c_1
                  (61, 0, 999, 1001),                  # on == c_1 - 1, off == c_1 + 1
                  (62, 0, 0, 2000),                    # off == c_2
                  (63, 0, 0, 2001),                    # off == c_2 + 1
                  (64, 0, 2500, 2500),                 # zero length: one microsecond at its onset
                  (65, 0, 3000, 100),                  # negative length: the same
                  (66, 0, -500, -100), (66, 0, 5000, 6000),     # wholly before t0, wholly after t1
                  (67, 0, -1000, 9000),                # across the whole span
                  (59, 0, 0, 4000), (68, 0, 0, 4000)]  # outside the pitch range
    under = [(60, 3, 0, 10000), (60, 5, 1000, 1500), (60, 7, 3000, 3200),
             (62, 2, 0, 4000), (62, 4, 0, 4000), (62, 9, 2000, 2100)]
    return [
        case('two_notes', [(60, 0, 1000, 3000), (61, 5, 2500, 2600)], W=8, row_px=2, lo=60, hi=61, tick=4000),
        case('edges', edge_notes, W=4, lo=60, hi=67),
        case('ticks_negative_t0', [], W=4, lo=60, hi=61, t0=-2500, t1=1500, tick=2000),
        case('ticks_on_an_edge', [], W=4, lo=60, hi=60, t0=-2500, t1=1500, tick=1500),
        case('span_equals_w', [(60, 0, 9, 10)], W=5, lo=60, hi=60, t0=7, t1=12),
        case('span_not_divisible', [(60, 0, 5, 6), (61, 0, 6, 7)], W=3, lo=60, hi=61, t0=0, t1=10),
        case('long_under_short', under, W=5, lo=60, hi=62),
        case('groups_fold', [(60, 33, 0, 2000)], W=3, lo=60, hi=60, group=FOLD),
        case('pair_small', [(60, 0, 0, 2000)], [(60, 0, 1000, 3000)], W=4, lo=60, hi=60),
        case('pair_empty_gold', [(60, 0, 0, 2000)], [], W=4, lo=60, hi=60),
        case('single_of_the_same', [(60, 0, 0, 2000)], None, W=4, lo=60, hi=60),
        case('empty_single', [], None, W=3, lo=60, hi=61),
        case('empty_pair', [], [], W=3, lo=60, hi=61, tick=1000),
        case('empty_est_pair', [], [(61, 0, 1000, 1001)], W=3, lo=60, hi=61),
    ]


# Drawn by hand from the rule's text; rows from the highest pitch down.
EXPECTED = {
    # pitch 61 (a black key): the note covers [2500, 2600), column 2 alone; ticks at 0 and 4000: columns 0 and 4.
    # pitch 60: [1000, 3000) covers columns 1 (its onset) and 2; each pitch twice (row_px = 2)
    'two_notes': [[3, 1, 27, 1, 3, 1, 1, 1]] * 2 + [[2, 17, 16, 0, 2, 0, 0, 0]] * 2,
    'edges': [[16, 16, 16, 16],                        # 67: sounding everywhere, its onset before the image
              [1, 1, 1, 1],                            # 66: nothing reaches the span
              [0, 0, 0, 17],                           # 65: [3000, 3001)
              [0, 0, 17, 0],                           # 64: [2500, 2501)
              [17, 16, 16, 1],                         # 63: [0, 2001) still covers column 2
              [17, 16, 0, 0],                          # 62: [0, 2000) ends with column 1
              [17, 16, 1, 1],                          # 61: [999, 1001): onset in column 0, one microsecond of column 1
              [0, 17, 0, 0]],                          # 60: the onset belongs to the column it opens
    # edges -2500, -1500, -500, 500, 1500; multiples of 2000: -2000 (column 0) and 0 (column 2)
    'ticks_negative_t0': [[3, 1, 3, 1], [2, 0, 2, 0]],
    # multiples of 1500: -1500 opens column 1, 0 in column 2, 1500 is t1 and outside
    'ticks_on_an_edge': [[0, 2, 2, 0]],
    'span_equals_w': [[0, 0, 17, 0, 0]],
    # edges 0, 3, 6, 10
    'span_not_divisible': [[1, 1, 17], [0, 17, 0]],
    # 62: programs 2 and 4 begin together and end together, 9 is short: column 0 the last begun (4), column 2 the short
    # one, column 3 the FIRST that attains the maximum (2), column 4 nothing (both end at 4000).  61: a black key.
    # 60: the long note (3) under two short ones (5, 7): 3, 5, 3 again, 7, 3 again
    'long_under_short': [[25, 24, 35, 20, 0], [1, 1, 1, 1, 1], [23, 27, 22, 31, 22]],
    # program 33 -> group 16 + 231 mod 112 = 23 -> 7
    'groups_fold': [[31, 30, 0]],
    'pair_small': [[69, 78, 72, 0]],
    'pair_empty_gold': [[69, 68, 0, 0]],
    'single_of_the_same': [[17, 16, 0, 0]],
    'empty_single': [[1, 1, 1], [0, 0, 0]],
    'empty_pair': [[3, 3, 3], [2, 2, 2]],
    'empty_est_pair': [[1, 74, 1], [0, 0, 0]],
}


def shapes():
    """The sizes at which the kernel can go wrong, each with seeded random notes."""
    rng = np.random.default_rng(29)
    out = []
    out.append(case('w1', random_notes(rng, 30, 58, 63, 0, 50000), W=1, row_px=3, lo=58, hi=63, t1=50000, tick=7000))
    for W in (63, 64, 65, THREADS - 1, THREADS, THREADS + 1):
        t1 = 977 * W + 13
        out.append(case('w%d' % W, random_notes(rng, 60, 59, 62, 0, t1), random_notes(rng, 60, 59, 62, 0, t1),
                        W=W, lo=59, hi=62, t1=t1, tick=9973))
    t1 = 3 * MAX_DIM + 1
    out.append(case('widest', random_notes(rng, 400, 60, 60, 0, t1, longest=900), W=MAX_DIM, lo=60, hi=60, t1=t1,
                    tick=1000, group=MERGED))
    out.append(case('tallest', random_notes(rng, 300, 0, 127, 0, 3000), random_notes(rng, 300, 0, 127, 0, 3000), W=3,
                    row_px=128, t1=3000))
    for px in (1, 2, 5):
        out.append(case('odd_w_px%d' % px, random_notes(rng, 80, 40, 52, -5000, 90000), W=37, row_px=px, lo=40, hi=52,
                        t0=-5000, t1=90000, tick=10000, group=FOLD))
    # past any block size and past 16 bits, at one pitch
    on = np.sort(rng.integers(0, 7000000, 70000))
    dur = rng.integers(1, 300, 70000)
    many = [(64, int(k % 128), int(a), int(a + d)) for k, (a, d) in enumerate(zip(on, dur))]
    out.append(case('many_notes', many, W=THREADS + 1, lo=63, hi=65, t1=7000000, group=FOLD))
    out.append(case('many_notes_pair', many[:40000], many[30000:], W=301, lo=64, hi=64, t0=2000000, t1=5000000))
    # a note that lasts the whole span under 20 000 short ones: between them the long one is drawn, found in one read
    short = [(60, 2, 1000 * k, 1000 * k + 500) for k in range(20000)]
    out.append(case('long_under_many', [(60, 1, -10, 20000000)] + short, W=1000, lo=60, hi=60, t0=5000000, t1=5100000))
    out.append(case('long_under_many_wide', [(60, 1, -10, 20000000)] + short, W=640, row_px=2, lo=59, hi=61, t0=0,
                    t1=20000000, tick=1000000))
    # times past 2^32 and a negative origin
    far = 2 ** 40
    out.append(case('late', [(p, p, far + 100 * k, far + 100 * k + 250) for k, p in enumerate((0, 127, 60, 60, 61))],
                    [(60, 0, far - 50, far + 130)], W=12, lo=0, hi=127, t0=far - 100, t1=far + 620, tick=200))
    return out


def corpus():
    """Every case of the GPU tests: the hand-drawn ones, the shapes, and grid-aligned pairs."""
    grid = [grid_case('grid%02d' % k, e, g) for k, (e, g) in enumerate(grid_pairs(12, seed=3))]
    return by_hand() + shapes() + grid
