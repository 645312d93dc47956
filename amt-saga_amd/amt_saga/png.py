"""Host side of the spectrogram images: the tables the level kernel reads -- thresholds, pixel rows to bins,
pixel columns to frames -- and the palettes of the PNG encoder.  numpy only; nothing here touches a GPU.

Stands where the reference hands audio_complete.D to librosa.display.specshow(y_axis='log') with matplotlib's colour map
(plot_spec, util_audio.py:509-518; plot_specs, util_audio.py:938-960)."""
import math

import numpy as np

MAX_DIM = 16384                       # PNG_MAX_DIM: width and height of an image
THRESHOLDS = 255
AXES = ('log', 'linear')
PALETTES = ('cubehelix', 'gray', 'roll')
FMIN = 27.5                           # the lowest frequency of the log axis: A0

# The piano-roll palette, entry by entry; every entry that is not named here is black.
ROLL_COLOURS = {
    # background: white-key row, black-key row, and the tick shade of each
    0: (250, 250, 250), 1: (232, 232, 236), 2: (205, 205, 210), 3: (190, 190, 197),
    # one list: sixteen group hues at 16 + 2 g, the darker onset variant at 16 + 2 g + 1
    16: (66, 133, 244), 17: (26, 82, 168), 18: (219, 68, 55), 19: (150, 35, 28),
    20: (15, 157, 88), 21: (8, 100, 54), 22: (244, 160, 0), 23: (170, 105, 0),
    24: (171, 71, 188), 25: (110, 35, 125), 26: (0, 172, 193), 27: (0, 110, 125),
    28: (255, 112, 67), 29: (190, 70, 35), 30: (124, 179, 66), 31: (78, 120, 35),
    32: (92, 107, 192), 33: (50, 62, 130), 34: (240, 98, 146), 35: (170, 50, 95),
    36: (0, 137, 123), 37: (0, 85, 76), 38: (192, 202, 51), 39: (128, 136, 25),
    40: (141, 110, 99), 41: (90, 66, 58), 42: (120, 144, 156), 43: (72, 92, 102),
    44: (255, 202, 40), 45: (185, 140, 10), 46: (126, 87, 194), 47: (80, 50, 135),
    # a pair, 64 + 4 class + estimate onset + 2 gold onset: estimate only (red), gold only (blue), both (green)
    68: (229, 57, 53), 69: (140, 20, 20),
    72: (30, 136, 229), 74: (13, 71, 161),
    76: (67, 160, 71), 77: (27, 94, 32), 78: (0, 77, 64), 79: (10, 50, 15),
}


def thresholds(top_db=80.0):
    """float32 [255]: thr[k - 1] = 10^(-(top_db / 20)(1 - (k - 0.5) / 255)), k = 1 .. 255, in float64, rounded once.
    A magnitude v relative to ref has level #{k: v >= thr[k - 1] ref}: amplitude_to_db(v, ref) over [-top_db, 0] cut
    into 256 equal steps, the boundaries half a step in."""
    top_db = float(top_db)
    if not (top_db > 0 and math.isfinite(top_db)):
        raise ValueError('Invalid Input shape. Expected: top_db > 0 . Got: %r' % top_db)
    k = np.arange(1, THRESHOLDS + 1, dtype=np.float64)
    thr = (10.0 ** (-(top_db / 20.0) * (1.0 - (k - 0.5) / 255.0))).astype(np.float32)
    if not np.all(np.diff(thr) > 0):
        raise ValueError('Invalid Input shape. Expected: a top_db whose thresholds differ in float32 . Got: %r' % top_db)
    return thr


def _dim(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_DIM:
        raise ValueError('Invalid Input shape. Expected: %s in 1 .. %d . Got: %r' % (what, MAX_DIM, v))
    return int(v)


def axis_cols(T, W):
    """int32 [W, 2]: pixel column i covers frames [i T // W, max(i T // W + 1, (i + 1) T // W)) -- every frame once when
    W <= T (the cell's maximum decimates), frames repeated when W > T."""
    W = _dim(W, 'W')
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
        raise ValueError('Invalid Input shape. Expected: T >= 1 . Got: %r' % (T,))
    i = np.arange(W, dtype=np.int64)
    lo = i * int(T) // W
    hi = np.maximum(lo + 1, (i + 1) * int(T) // W)
    return np.stack([lo, hi], axis=1).astype(np.int32)


def axis_rows(F, H, sr, n_fft, axis='log', fmin=FMIN):
    """int32 [H, 2]: pixel row j covers bins [lo, hi) of the F = n_fft // 2 + 1 (or fewer) bins at b sr / n_fft Hz;
    row 0 is the highest frequency.
    'linear': equal bin counts, the columns' rule upside down.
    'log' (specshow's y_axis='log'): H equal ratios from fmin to sr / 2; a row takes the bins whose centre lies in its
    interval [low edge, high edge) -- the top row to bin F - 1 -- and a row whose interval holds no centre takes the one
    bin nearest to the interval's geometric middle.  Every row is non-empty, lo and hi never decrease upwards."""
    H = _dim(H, 'H')
    if isinstance(F, bool) or not isinstance(F, (int, np.integer)) or F < 1:
        raise ValueError('Invalid Input shape. Expected: F >= 1 . Got: %r' % (F,))
    if axis not in AXES:
        raise ValueError('Requested attribute does not exist: axis must be one of %s' % (AXES,))
    F = int(F)
    r = np.arange(H, dtype=np.int64)                                  # rows from the bottom
    if axis == 'linear':
        lo = r * F // H
        hi = np.maximum(lo + 1, (r + 1) * F // H)
    else:
        sr, n_fft, fmin = float(sr), float(n_fft), float(fmin)
        if not (sr > 0 and n_fft > 0 and 0 < fmin < sr / 2):
            raise ValueError('Invalid Input shape. Expected: 0 < fmin < sr / 2 . Got: fmin %r, sr %r' % (fmin, sr))
        edge = fmin * (sr / 2 / fmin) ** (np.arange(H + 1, dtype=np.float64) / H) * (n_fft / sr)     # in bins
        lo = np.ceil(edge[:-1]).astype(np.int64)
        hi = np.ceil(edge[1:]).astype(np.int64)
        hi[-1] = F
        near = np.floor(np.sqrt(edge[:-1] * edge[1:]) + 0.5).astype(np.int64)
        lo, hi = np.clip(lo, 0, F), np.clip(hi, 0, F)
        empty = hi <= lo
        near = np.clip(near, 0, F - 1)
        lo = np.where(empty, near, lo)
        hi = np.where(empty, near + 1, hi)
        lo = np.minimum(lo, F - 1)
        lo, hi = np.maximum.accumulate(lo), np.maximum.accumulate(hi)
        hi = np.maximum(hi, lo + 1)
    return np.stack([lo, hi], axis=1)[::-1].astype(np.int32).copy()


def palette(name='cubehelix'):
    """uint8 [256, 3] (R, G, B per level), or None for 'gray' (the encoder then writes a greyscale file).
    'cubehelix': Green's closed form (D. A. Green, Bull. Astron. Soc. India 39, 289, 2011) in float64 with start 0.5,
    rotations -1.5, hue 1, gamma 1: phi = 2 pi (start / 3 + rotations x), a = hue x (1 - x) / 2,
    R = x + a (-0.14861 cos phi + 1.78277 sin phi), G = x + a (-0.29227 cos phi - 0.90649 sin phi),
    B = x + a 1.97294 cos phi, clipped to [0, 1]; 8-bit by floor(255 v + 0.5).  Black at level 0, white at 255, the
    luminance 0.30 R + 0.59 G + 0.11 B rising with the level.
    'roll': the literal table ROLL_COLOURS of the piano-roll pixel values (amt_saga.roll.legend()), black elsewhere."""
    if name not in PALETTES:
        raise ValueError('Requested attribute does not exist: palette must be one of %s' % (PALETTES,))
    if name == 'gray':
        return None
    if name == 'roll':
        table = np.zeros((256, 3), dtype=np.uint8)
        for value, rgb in ROLL_COLOURS.items():
            table[value] = rgb
        return table
    x = np.arange(256, dtype=np.float64) / 255.0
    phi = 2.0 * np.pi * (0.5 / 3.0 + -1.5 * x)
    a = 1.0 * x * (1.0 - x) / 2.0
    c, s = np.cos(phi), np.sin(phi)
    rgb = np.stack([x + a * (-0.14861 * c + 1.78277 * s), x + a * (-0.29227 * c - 0.90649 * s), x + a * (1.97294 * c)], 1)
    return np.floor(255.0 * np.clip(rgb, 0.0, 1.0) + 0.5).astype(np.uint8)


def parse_size(text):
    """'1200x500' -> (1200, 500); ValueError for anything else or a side outside 1 .. 16384."""
    parts = str(text).lower().split('x')
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError('Invalid Input shape. Expected: WxH, e.g. 1200x500 . Got: %r' % (text,))
    return _dim(int(parts[0]), 'W'), _dim(int(parts[1]), 'H')
