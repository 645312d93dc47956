"""Test infrastructure: WHICH windows of a metric-size batch the GPU tests compare with the same windows run in a small
batch (tests/test_gpu_workload_batches.py).  Host integers only; tests/test_workload_positions_cpu.py checks the
positions against the product's own geometry.

A batch of B windows holds mag [B, T, ldf] float32 and, when an iteration resynthesises, ph [B, T, ldf, 2] float32
(unit complex, read as float2).  The places where a kernel of such a batch can go wrong and a 70-window test cannot:

  * a multiple of `chunk`: the networks walk a batch in chunks of that many windows through one workspace layout
    (RD_CHUNK of amt_rdcnn.hip);
  * the window inside which a running index of mag or ph passes a limit of 32-bit arithmetic: the element index in
    floats (and, for ph, in float2 = ph floats / 2) passes 2^31, the byte offset passes 2^32 or 2^33;
  * both ends of the batch, and sub-batches of a ragged size (5) and of one window.
"""
import numpy as np


def limit_windows(B, T, ldf, with_phase):
    """[(label, window)] for every limit a running index passes inside the batch: the first window that holds an
    element whose index (or whose byte offset) is >= the limit."""
    n = T * ldf                                             # floats of mag per window = float2 of ph per window
    steps = [('mag element index passes 2^31', n, 1 << 31),
             ('mag byte offset passes 2^32', 4 * n, 1 << 32),
             ('mag byte offset passes 2^33', 4 * n, 1 << 33)]
    if with_phase:
        steps += [('ph element index (floats) passes 2^31', 2 * n, 1 << 31),
                  ('ph float2 index passes 2^31', n, 1 << 31),
                  ('ph byte offset passes 2^32', 8 * n, 1 << 32),
                  ('ph byte offset passes 2^33', 8 * n, 1 << 33)]
    return [(what, limit // step) for what, step, limit in steps if limit // step < B]     # window w covers [w step, (w + 1) step)


def _around(w, B, group):
    return max(0, w - group // 2), min(B, w + group // 2)


def _merge(ranges):
    out = []
    for a, b in sorted(r for r in ranges if r[1] > r[0]):
        if out and a < out[-1][1]:                          # overlapping (touching ranges stay apart)
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def marked_ranges(B, T, ldf, with_phase, chunk=1024, group=16):
    """[(label, (start, stop))] of the ranges a batch's geometry marks, before merging."""
    out = [('first', (0, min(group, B))), ('last', (max(0, B - group), B))]
    out += [('chunk %d' % m, _around(m, B, group)) for m in range(chunk, B, chunk)]
    out += [(what, _around(w, B, group)) for what, w in limit_windows(B, T, ldf, with_phase)]
    return out


def groups_for(B, T, ldf, with_phase, chunk=1024, group=16, seed=0, n_random=4):
    """Sorted, non-overlapping (start, stop) window ranges of a batch of B windows: the first and the last `group`
    windows, a `group`-window range straddling every multiple of `chunk` below B and every window of limit_windows()
    (overlapping ones merged into one range), and, placed by a seeded generator where they touch none of those, one
    ragged range of 5 windows, one single window and n_random ranges of `group` windows.  A seeded range that finds no
    free place (a batch too small to hold it apart from the others) is left out."""
    ranges = _merge(r for _, r in marked_ranges(B, T, ldf, with_phase, chunk, group))
    rng = np.random.default_rng(seed)
    for n in (5, 1) + (group,) * n_random:
        for _ in range(256):
            if n > B:
                break
            a = int(rng.integers(0, B - n + 1))
            if all(a + n <= lo or a >= hi for lo, hi in ranges):
                ranges.append((a, a + n))
                break
    return sorted(ranges)


def fixture_rows(B, T, ldf, with_phase, n, chunk=1024, group=16, seed=0):
    """n distinct rows of a B-window batch for oracle-fixture windows, spread over the positions groups_for() marks, in
    this order of preference: both sides of every chunk boundary, every window of limit_windows() and the one before
    it, the two ends of the batch, the first and the last window of every range, then the ranges' other windows.
    Ascending."""
    want = []
    for m in range(chunk, B, chunk):
        want += [m - 1, m]
    for _, w in limit_windows(B, T, ldf, with_phase):
        want += [w, w - 1]
    want += [0, B - 1]
    groups = groups_for(B, T, ldf, with_phase, chunk, group, seed)
    want += [a for a, _ in groups] + [b - 1 for _, b in groups] + [w for a, b in groups for w in range(a, b)]
    rows = []
    for w in want:
        if 0 <= w < B and w not in rows and len(rows) < n:
            rows.append(int(w))
    if len(rows) < n:
        raise ValueError('a batch of %d windows has no %d marked rows' % (B, n))
    return sorted(rows)
