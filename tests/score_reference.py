"""Test infrastructure: the scoring rule of DESIGN 27 restated in plain Python, and the corpus the tests share.  Nothing
here imports the product.

A note is a tuple (pitch, program, on_us, off_us); a pair is (estimates, references).

  * matched(e, r, offset, program, group): the rule of one edge.
  * max_matching(...): an iterative augmenting-path matcher; true positives are the size of a MAXIMUM matching.
  * first_fit(...): every reference in sorted order takes the first unused estimate that matches -- kept only to show that
    it is the wrong rule.
  * frame_counts(...): rolls as sets of (frame, pitch) cells.
  * score(est, ref, group): the ten integers of one pair.
"""
import bisect

import numpy as np

ONSET_TOL, OFFSET_FLOOR, FRAME_US = 50000, 50000, 10000
COLUMNS = ('n_est', 'n_ref', 'tp_on', 'tp_onoff', 'tp_on_prog', 'tp_onoff_prog', 'frame_tp', 'frame_fp', 'frame_fn',
           'n_frames')
IDENTITY = list(range(128))
# the three instrument groups of the transcription loop: guitars 24-31, strings and ensembles 40-55, the rest
MERGED = [2 if 24 <= p <= 31 else (1 if 40 <= p <= 55 else 0) for p in range(128)]
VARIANTS = ((False, False), (True, False), (False, True), (True, True))     # (offset, program) of columns 2 .. 5


def sort_key(n):
    return (n[0], n[2], n[3], n[1])


def matched(e, r, offset, program, group):
    if e[0] != r[0] or abs(e[2] - r[2]) > ONSET_TOL:
        return False
    if offset:
        part = (r[3] - r[2]) // 5 if r[3] > r[2] else 0
        if abs(e[3] - r[3]) > max(OFFSET_FLOOR, part):
            return False
    if program and group[e[1]] != group[r[1]]:
        return False
    return True


def _adjacency(est, ref, offset, program, group):
    """adj[j] = the indices into sorted(est) that sorted(ref)[j] matches, ascending."""
    est, ref = sorted(est, key=sort_key), sorted(ref, key=sort_key)
    keys = [(e[0], e[2]) for e in est]
    adj = []
    for r in ref:
        lo = bisect.bisect_left(keys, (r[0], r[2] - ONSET_TOL))
        hi = bisect.bisect_right(keys, (r[0], r[2] + ONSET_TOL))
        adj.append([i for i in range(lo, hi) if matched(est[i], r, offset, program, group)])
    return adj, len(est)


def max_matching(est, ref, offset=False, program=False, group=IDENTITY, paths=None):
    """Size of a maximum matching.  paths (a list) receives the length, in references, of every augmenting path."""
    adj, n_est = _adjacency(est, ref, offset, program, group)
    owner = [-1] * n_est
    size = 0
    for root in range(len(adj)):
        seen = set()
        stack = [(root, -1, 0)]                                     # (reference, the estimate it was reached through, cursor)
        while stack:
            r, via, at = stack[-1]
            free = [e for e in adj[r] if owner[e] < 0 and e not in seen]
            if free:
                e = free[0]
                if paths is not None:
                    paths.append(len(stack))
                while stack:
                    r, via, _ = stack.pop()
                    owner[e] = r
                    e = via
                size += 1
                break
            while at < len(adj[r]) and adj[r][at] in seen:
                at += 1
            if at == len(adj[r]):
                stack.pop()
                continue
            e = adj[r][at]
            seen.add(e)
            stack[-1] = (r, via, at + 1)
            stack.append((owner[e], e, 0))
    return size


def first_fit(est, ref, offset=False, program=False, group=IDENTITY):
    adj, n_est = _adjacency(est, ref, offset, program, group)
    used = [False] * n_est
    size = 0
    for cand in adj:
        for e in cand:
            if not used[e]:
                used[e] = True
                size += 1
                break
    return size


def roll(notes):
    cells = set()
    for pitch, _, on, off in notes:
        if off <= on:
            continue
        k = max(0, -(-on // FRAME_US))
        while k * FRAME_US < off:
            cells.add((k, pitch))
            k += 1
    return cells


def frame_counts(est, ref):
    a, b = roll(est), roll(ref)
    top = max([n[3] for n in est] + [n[3] for n in ref] + [0])
    n_frames = 0 if top <= 0 else (top - 1) // FRAME_US + 1
    return [len(a & b), len(a - b), len(b - a), n_frames]


def score(est, ref, group=IDENTITY):
    return [len(est), len(ref)] + [max_matching(est, ref, o, p, group) for o, p in VARIANTS] + frame_counts(est, ref)


# ---------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------
CHAIN_SEGMENTS, CHAIN_LENGTH, CHAIN_STEP = 10, 300, 30000
RANDOM_SEED = 0


def long_chain():
    """3000 notes per side on one pitch, 30 ms apart, in ten chains of 300.  In a chain, reference i matches (onset +
    offset) the estimates i - 1 and i only; reference 0 also matches an extra estimate x that sorts right behind
    estimate 0; the last reference has estimate n - 1 alone.  Taking references in order with the first free estimate
    gives 0-0, 1-1, ..., and the last reference then needs the path back through every one of them to x."""
    est, ref = [], []
    dur = 100000
    for s in range(CHAIN_SEGMENTS):
        base = s * (CHAIN_LENGTH * CHAIN_STEP + 1000000)
        n = CHAIN_LENGTH - 1
        for i in range(n + 1):
            ref.append((64, 0, base + CHAIN_STEP * i, base + CHAIN_STEP * i + dur))
        for j in range(n):
            est.append((64, 0, base + CHAIN_STEP * j, base + CHAIN_STEP * j + dur + 25000))
        est.append((64, 0, base + 1, base + dur - 40000))
    return est, ref


def random_pairs(count=200, seed=RANDOM_SEED):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        sides = []
        for _side in range(2):
            n = int(rng.integers(6, 13))
            sides.append([(int(rng.choice((60, 62))), int(rng.choice((0, 24))), 1000000 + int(rng.integers(0, 120001)), 0)
                          for _ in range(n)])
            sides[-1] = [(p, g, on, on + int(rng.integers(300000, 700001))) for p, g, on, _ in sides[-1]]
        out.append(tuple(sides))
    return out


def corpus():
    """[(name, estimates, references)]; the 200 random pairs come last, named random000 .. random199."""
    rng = np.random.default_rng(27)
    out = []
    one = [(60, 0, 0, 500000)]
    out.append(('empty_both', [], []))
    out.append(('empty_est', [], one + [(72, 3, 250000, 900000)]))
    out.append(('empty_ref', one + [(72, 3, 250000, 900000)], []))
    out.append(('augment', [(60, 0, 0, 850000), (60, 0, 10000, 1100000)], [(60, 0, 0, 1000000), (60, 0, 5000, 800000)]))
    est, ref = [], []
    r_on = 1000000
    for pitch, e_on, r_off, e_off in (
            (60, r_on + 50000, r_on + 250000, r_on + 250000),          # onset off by exactly 50 000
            (61, r_on + 50001, r_on + 250000, r_on + 250000),          # ... by 50 001: no variant matches
            (62, r_on, r_on + 250000, r_on + 250000 + 50000),          # duration 250 000: floor and 20 % coincide
            (63, r_on, r_on + 250000, r_on + 250000 + 50001),
            (64, r_on, r_on + 250005, r_on + 250005 + 50001),          # 250 005 // 5 = 50 001
            (65, r_on, r_on + 250005, r_on + 250005 + 50002),
            (66, r_on, r_on + 1000000, r_on + 1000000 - 200000),       # 1 000 000 // 5 = 200 000
            (67, r_on, r_on + 1000000, r_on + 1000000 - 200001),
            (68, r_on, r_on - 100000, r_on - 100000 + 50000),          # off <= on: the floor alone
            (69, r_on, r_on - 100000, r_on - 100000 + 50001)):
        ref.append((pitch, 0, r_on, r_off))
        est.append((pitch, 0, e_on, e_off))
    out.append(('tolerance_edges', est, ref))
    out.append(('program_split',
                [(60, 0, 0, 500000), (61, 40, 0, 500000), (62, 5, 0, 500000), (64, 0, 0, 400000), (64, 24, 0, 400000)],
                [(60, 24, 0, 500000), (61, 48, 0, 500000), (62, 5, 0, 500000), (64, 24, 1000, 400000), (64, 0, 2000, 400000)]))
    sides = []
    for _ in range(2):
        sides.append([(55, int(rng.choice((0, 24, 40))), 2000000 + int(rng.integers(0, 40001)),
                       2000000 + int(rng.integers(100000, 1000001))) for _ in range(70)])
    out.append(('dense_cluster', sides[0], sides[1]))
    out.append(('long_chain',) + long_chain())
    out.append(('late', [(70, 0, 2 ** 31 + 5000, 2 ** 31 + 400000), (71, 0, 2 ** 32 + 100, 2 ** 32 + 300000)],
                [(70, 0, 2 ** 31, 2 ** 31 + 405000), (71, 0, 2 ** 32 + 50100, 2 ** 32 + 300000)]))
    out.append(('pitch_edges', [(0, 0, 0, 300000), (127, 127, 100000, 600000), (127, 0, 140000, 200000)],
                [(0, 127, 20000, 310000), (127, 127, 120000, 590000), (0, 0, 700000, 800000)]))
    out.append(('frame_edges',
                [(50, 0, 20000, 50000),                                 # starts exactly on frame 2: frames 2, 3, 4
                 (51, 0, 9999, 10001),                                  # frame 1 alone
                 (52, 0, 10000, 20000),                                 # frame 1
                 (53, 0, 30000, 30000), (53, 0, 40000, 35000)],         # off <= on: no cell
                [(50, 0, 10001, 40000),                                 # ends exactly on frame 4: frames 2, 3
                 (52, 0, 0, 30000), (52, 0, 20000, 50000),              # overlapping: frames 0 .. 4 once
                 (54, 0, 0, 1005000)]))                                 # frames 0 .. 100: n_frames = 101, no multiple of 64
    for k, (e, r) in enumerate(random_pairs(200, RANDOM_SEED)):
        out.append(('random%03d' % k, e, r))
    return out


# the by-hand answers
AUGMENT_ROW = [2, 2, 2, 2, 2, 2, 100, 10, 0, 110]
TOLERANCE_EDGES_NOTES = [10, 10, 9, 5, 9, 5]
FRAME_EDGES_ROW = [5, 4, 2, 2, 2, 2, 3, 2, 105, 101]
