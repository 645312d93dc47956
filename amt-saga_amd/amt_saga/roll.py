"""Piano-roll images of transcriptions: note lists -> uint8 palette-index images on the device, any number
of them through ONE call of the HIP rasteriser (amt_roll_draw), alone or against gold notes, and from there through the
device PNG encoder (audio.png_encode, palette 'roll').

Stands where the reference's users would plot a piano roll of a transcription over the gold MIDI of the MIDI/audio pairs
the reference trains on (main.py:7) with matplotlib.  The rule is csrc/amt_roll_core.h's, all integers: times in int64
microseconds, W equal columns over [t0, t1), a pitch per row_px rows with the highest pitch on top, a note visible from
its onset to max(off, on + 1).  One list: the colour is the instrument group of the note drawn, darker in the column of
its onset.  A pair: estimate only (a false-positive cell), gold only (a miss) or both.
"""
import ctypes

import numpy as np

from . import png as _png
from . import score as _score

BACKGROUND, SINGLE, PAIR = 0, 16, 64                   # first pixel value of each kind
CLASS_NAMES = {1: 'estimate only', 2: 'gold only', 3: 'both'}
MAX_SPAN_US = 2 ** 40
MAX_T0_US = 2 ** 61
MAX_TICK_US = 2 ** 40
META = 10                                              # int64 per image (ROLL_META)


class RollArgs(ctypes.Structure):
    """amt_roll_args of include/amt_saga.h."""
    _fields_ = [(name, ctypes.c_void_p) for name in (
        'est_pitch', 'est_program', 'est_on', 'est_off', 'gold_pitch', 'gold_program', 'gold_on', 'gold_off',
        'est_offsets_host', 'gold_offsets_host', 'est_offsets', 'gold_offsets', 'image_meta_host', 'image_meta', 'group',
        'scratch')] + \
        [('scratch_bytes', ctypes.c_int64), ('out', ctypes.c_void_p), ('out_bytes', ctypes.c_int64),
         ('n_images', ctypes.c_int64)]


def roll_args(**fields):
    """RollArgs from keyword arguments (_lib.args): a tensor gives its device pointer, the host tables are passed as
    addresses."""
    from . import _lib
    return _lib.args(RollArgs, **fields)


def legend():
    """{pixel value: meaning} for every value the rule can produce."""
    out = {0: 'background, white-key row', 1: 'background, black-key row', 2: 'tick, white-key row',
           3: 'tick, black-key row'}
    for g in range(16):
        out[SINGLE + 2 * g] = 'group %d' % g
        out[SINGLE + 2 * g + 1] = 'group %d, onset' % g
    for cls, name in CLASS_NAMES.items():
        for onsets in range(4):
            if (onsets & 1 and not cls & 1) or (onsets & 2 and not cls & 2):
                continue                                               # an onset is covered by its own note
            what = [w for bit, w in ((1, 'estimate onset'), (2, 'gold onset')) if onsets & bit]
            out[PAIR + 4 * cls + onsets] = ', '.join([name] + what)
    return out


def _int(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError('Invalid Input shape. Expected: %s in %d .. %d . Got: %r' % (what, lo, hi, v))
    return int(v)


def _us(sec, what):
    s = float(sec)
    if not np.isfinite(s) or abs(s) >= 2.0 ** 62 / 1e6:
        raise ValueError('Invalid Input shape. Expected: a finite %s . Got: %r' % (what, sec))
    return int(np.rint(s * 1e6))


def _default_span(est, gold):
    """0 to the largest off of either list, up to a whole second, at least one."""
    top = max([int(p[3].max()) for p in (est, gold) if p is not None and len(p[3])] + [0])
    return 0, max(1, -(-top // 1000000)) * 1000000


def geometry(n, width=1200, row_px=5, pitch=(21, 108), span=None, tick=1.0):
    """The checked geometry of n images: (W, row_px, pitch_lo, pitch_hi, H, tick in us, spans in us or None).  Every
    refusal is a ValueError; nothing here touches a device."""
    W = _png._dim(width, 'width')
    if not (hasattr(pitch, '__len__') and len(pitch) == 2):
        raise ValueError('Invalid Input shape. Expected: pitch = (lowest, highest) . Got: %r' % (pitch,))
    lo, hi = _int(pitch[0], 'the lowest pitch', 0, 127), _int(pitch[1], 'the highest pitch', 0, 127)
    if lo > hi:
        raise ValueError('Invalid Input shape. Expected: lowest pitch <= highest pitch . Got: %d > %d' % (lo, hi))
    px = _int(row_px, 'row_px', 1, _png.MAX_DIM)
    H = (hi - lo + 1) * px
    if H > _png.MAX_DIM:
        raise ValueError('Invalid Input shape. Expected: (pitches) x row_px <= %d . Got: %d x %d' % (_png.MAX_DIM, hi - lo + 1, px))
    tick_us = _us(tick, 'tick')
    if not 0 <= tick_us <= MAX_TICK_US:
        raise ValueError('Invalid Input shape. Expected: tick in 0 .. %d us . Got: %r' % (MAX_TICK_US, tick))
    spans = None
    if span is not None:
        items = list(span)
        if len(items) == 2 and not hasattr(items[0], '__len__'):
            items = [items] * n
        if len(items) != n or any(not hasattr(s, '__len__') or len(s) != 2 for s in items):
            raise ValueError('Invalid Input shape. Expected: one (t0, t1) or one per image (%d) . Got: %r' % (n, span))
        spans = [_check_span(_us(s[0], 'span'), _us(s[1], 'span'), W) for s in items]
    return W, px, lo, hi, H, tick_us, spans


def _check_span(t0, t1, W):
    if not (abs(t0) <= MAX_T0_US and W <= t1 - t0 <= MAX_SPAN_US):
        raise ValueError('Invalid Input shape. Expected: a span of %d .. %d us that begins within 2^61 us of 0 . Got: '
                         '%d .. %d us' % (W, MAX_SPAN_US, t0, t1))
    return t0, t1


def _lists(est_lists, gold_lists):
    """The packed lists of a call: ([estimates], [gold or None])."""
    if isinstance(est_lists, tuple) or not hasattr(est_lists, '__len__'):
        raise ValueError('Invalid Input shape. Expected: a list of note lists . Got: %s' % type(est_lists).__name__)
    if gold_lists is not None and len(gold_lists) != len(est_lists):
        raise ValueError('Invalid Input shape. Expected: as many gold lists as estimate lists . Got: %d and %d'
                         % (len(gold_lists), len(est_lists)))

    def packed(p):
        return p if isinstance(p, tuple) else _score.pack(p)
    est = [packed(p) for p in est_lists]
    gold = [None] * len(est) if gold_lists is None else [None if p is None else packed(p) for p in gold_lists]
    return est, gold


def piano_rolls(est_lists, gold_lists=None, width=1200, row_px=5, pitch=(21, 108), span=None, tick=1.0, group=None):
    """One uint8 device image [H, W] per list of est_lists, H = (pitch[1] - pitch[0] + 1) * row_px, W = width: the
    palette indices of legend().  A list is a list of note dicts or what score.pack returned for one.  gold_lists: None
    (every image shows one list, coloured by group[program] mod 16), or one entry per image -- a list (even an empty
    one) draws the pair: estimate only, gold only, both; None leaves that image in single mode.  span: (t0, t1) in
    seconds for all, or one per image; by default from 0 to the largest off of either list, up to a whole second, at
    least one.  tick: seconds between the background ticks, 0 for none.  group: int32 [128], program -> group (the
    identity by default; the command lines pass score.loop_groups()).
    ONE amt_roll_draw launch on the current stream for the whole list; the images are views of one allocation.  Every
    refusal is a ValueError, raised before any device work."""
    call = prepare(est_lists, gold_lists, width, row_px, pitch, span, tick, group)
    return [] if call is None else call()


def prepare(est_lists, gold_lists=None, width=1200, row_px=5, pitch=(21, 108), span=None, tick=1.0, group=None):
    """The checks, the packing and the uploads of piano_rolls; returns a function that enqueues the ONE launch on the
    current stream and returns the images (views of one allocation, the same one at every call), or None for an empty
    list.  scripts/roll_bench.py times the launch alone through it."""
    est, gold = _lists(est_lists, gold_lists)
    n = len(est)
    W, px, lo, hi, H, tick_us, spans = geometry(n, width, row_px, pitch, span, tick)
    g = _score.group_table(group)
    if spans is None:
        spans = [_check_span(*_default_span(e, r), W) for e, r in zip(est, gold)]
    if n == 0:
        return None
    empty = _score.pack([])
    sides = [_score._side(est), _score._side([empty if r is None else r for r in gold])]
    meta = np.zeros((n, META), dtype=np.int64)
    for i, (t0, t1) in enumerate(spans):
        meta[i] = [W, px, lo, hi, t0, t1, tick_us, int(gold[i] is not None), i * W * H, 0]
    import torch
    from . import _lib
    from .device import require_gpu, stream_ptr
    lib = _lib.load()
    for s in sides:                                                    # what a caller packed itself is checked here
        _lib.check(lib.amt_score_check_notes(s[0].ctypes.data, s[1].ctypes.data, len(s[0])))
    need = int(lib.amt_roll_scratch_bytes(int(sides[0][4][-1]), int(sides[1][4][-1])))
    if need < 0:
        _lib.check(need)
    dev = require_gpu()

    def up(a):                                                         # (never empty: an empty tensor has no address)
        t = torch.zeros(max(1, a.size), dtype=torch.from_numpy(a).dtype, device=dev)
        if a.size:
            t[:a.size] = torch.from_numpy(a).to(dev)
        return t
    d_est, d_gold = [up(a) for a in sides[0]], [up(a) for a in sides[1]]
    d_group, d_meta = up(g), up(meta.reshape(-1))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty((n * W * H,), dtype=torch.uint8, device=dev)
    a = roll_args(est_pitch=d_est[0], est_program=d_est[1], est_on=d_est[2], est_off=d_est[3],
                  gold_pitch=d_gold[0], gold_program=d_gold[1], gold_on=d_gold[2], gold_off=d_gold[3],
                  est_offsets_host=sides[0][4].ctypes.data, gold_offsets_host=sides[1][4].ctypes.data,
                  est_offsets=d_est[4], gold_offsets=d_gold[4], image_meta_host=meta.ctypes.data, image_meta=d_meta,
                  group=d_group, scratch=scratch, scratch_bytes=need, out=out, out_bytes=n * W * H, n_images=n)
    keep = (sides, meta, d_est, d_gold, d_group, d_meta, scratch)     # what `a` points into lives as long as the call

    def call(_keep=keep):
        _lib.check(lib.amt_roll_draw(ctypes.byref(a), stream_ptr()))
        return list(out.view(n, H, W).unbind(0))
    return call


def piano_roll_png(est_lists, gold_lists=None, **kw):
    """piano_rolls and audio.png_encode (palette 'roll') together: one rasteriser launch for the whole list and one
    encode call per audio.MAX_SIGNALS images; returns one PNG file (bytes) per list."""
    images = piano_rolls(est_lists, gold_lists, **kw)
    from . import audio
    files = []
    for k in range(0, len(images), audio.MAX_SIGNALS):
        files += audio.png_encode(images[k:k + audio.MAX_SIGNALS], palette='roll')
    return files


def save_piano_rolls(est_lists, paths, gold_lists=None, **kw):
    """piano_roll_png(est_lists, gold_lists, ...) written to `paths`, one file per list, one write per file."""
    paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, '__fspath__') else list(paths)
    if len(paths) != len(est_lists):
        raise ValueError('Invalid Input shape. Expected: one path per image (%d) . Got: %d' % (len(est_lists), len(paths)))
    files = piano_roll_png(est_lists, gold_lists, **kw)
    for data, path in zip(files, paths):
        with open(path, 'wb') as f:
            f.write(data)
