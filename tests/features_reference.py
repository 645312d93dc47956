"""Plain numpy restatement of the feature kernels (amt_features.hip) and the integer glue (amt_loop.hip), the error
measures and bars the feature tests assert, and the geometry lists they walk.  Test infrastructure: imported by
test_features_reference_cpu.py (no GPU), test_gpu_features_geometry.py and test_gpu_loop.py.

The float functions work on the device layout -- spectra [B][rows >= T][ldf] frame-major, rows and pad bins beyond
[T][F] never read -- take the arguments of the C entries and run in the dtype they are given: float64 is the reference,
float32 the "float32 numpy" side of a bar.  The inputs are converted, not recomputed: both runs see the same float32
values.  Independent of oracle/audio.py (test_features_reference_cpu.py ties the two together).

Bars (u = 2^-24, the unit roundoff of float32):

  compress_bands   |got - ref64| <= c u mean|x| / |ref|   per band and frame, mean|x| the float64 mean of the band's
      magnitudes.  Derived, first order in u: a float32 sum in which no term passes through more than k additions is off
      by at most k u sum|x|.  The kernel's lane adds MAXQ registers one after the other (masked ones contribute an exact
      0) and the wave reduction adds six levels: k = MAXQ + 6.  The two divisions (by the width, by ref) are correctly
      rounded, u of the result each, and |result| <= sum|x| / (width |ref|): c = MAXQ + 8.  A band inside the first 64
      bins is, on the generic path, walked by ONE lane: width - 1 sequential additions and the two divisions, taken as
      c = width + 2.  MAXQ is the kernel's template argument: 5 (F <= 320), 17 (F <= 1088), 33 (F <= 2112).
  exact            frame_max, short_window mode 0 (one correctly rounded division), gather_frames, the integer glue.
  transcendental   short_window modes 1 / 2, dB, inverse dB, flatness rest on the device's log10f / atan2f / exp10f /
      logf / expf: e_gpu <= 2.5 e_f32numpy + 4 u scale, e = the largest distance from the float64 run over a window,
      e_f32numpy that of the float32 run of the same restatement, scale the float64 output's largest magnitude -- the
      convention of the convolution tests (2.5 = the margin granted to another evaluation order).
"""
import numpy as np

U = 2.0 ** -24
SENT = -7.0


# ---------------------------------------------------------------------------------------------------------------------
# geometry lists
# ---------------------------------------------------------------------------------------------------------------------
CB_BINS = (129, 257, 320, 321, 513, 1025, 1088, 1089, 2049, 2112)       # both sides of 64 * 5 / 17 / 33; 320, 1088, 2112
CB_FRAMES = (1, 3, 4, 5, 9)                                             # have no masked lane
CB_RESIZE_SOURCES = (0, 1, 2, 3, 7, 8, 13)
CB_STD_EDGES = (0, 1, 2, 3, 4, 5, 8, 11, 16, 22, 32, 45, 64, 90, 128, 181, 256, 362, 512, 724, 1025)
SW_BINS = (257, 1025)
SW_FRAMES = (1, 8, 33)
SW_BANDS = (1, 348)
DB_BINS = (257, 1025)
FLAT_BINS = (129, 1025)
RESIZE_T = 12
RESIZE_FRAMES = (3, 4, 8, 32)


def ldf_of_bins(F):
    """Row pitch of a spectrogram of F bins (amt_saga.audio.ldf_of for F = n_fft // 2 + 1)."""
    return (F + 3) // 4 * 4


def maxq_of(F):
    """Template argument of compress_bands_kernel serving F bins; None where the entry refuses."""
    for q in (5, 17, 33):
        if F <= 64 * q:
            return q
    return None


def band_edges(n_rows, bands):
    """util_audio.py:451-456: geomspace(1, n_rows, bands + 1) truncated, first edge 0, every band at least one row."""
    ind = np.geomspace(1, n_rows, bands + 1).astype(np.int64)
    ind[0] = 0
    for i in range(bands):
        if ind[i + 1] - ind[i] < 1:
            ind[i + 1] = ind[i] + 1
    return ind.astype(np.int32)


def linear_edges(n_rows, bands):
    """compress_bands(log=False): bands of n_rows // bands rows (util_audio.py:458-461)."""
    return (n_rows // bands * np.arange(bands + 1)).astype(np.int32)


def edge_sets(F):
    """name -> edges [bands + 1] int32 of every edge set of the matrix at F bins."""
    sets = {'log20': band_edges(F, 20), 'log40': band_edges(F, 40), 'log80': band_edges(F, 80),
            'lin8': linear_edges(F, 8), 'one': np.array([0, F], np.int32)}
    if F > 129:
        # a band ending on 64, a one-bin band at 64, one starting on a register boundary (128), wide ones
        sets['hand'] = np.array([0, 1, 63, 64, 65, 70, 128, 129, F], np.int32)
    return sets


def frame_maps(T):
    """name -> (src_frame int32 [target] or None for the identity, target) of every frame map of the matrix."""
    maps = {'identity': (None, T)}
    for t in CB_RESIZE_SOURCES:
        maps['resize%d' % t] = (resize_table([0], [t], 64, 8)[0], 8)
    maps['beyond'] = (np.array([0, T, T - 1, T + 5, -1, 0], np.int32), 6)
    return maps


# ---------------------------------------------------------------------------------------------------------------------
# the float operations
# ---------------------------------------------------------------------------------------------------------------------
def _ref(ref, B, dtype):
    return np.ones(B, dtype) if ref is None else np.asarray(ref).astype(dtype)


def compress_bands(mag, T, F, edges, ref=None, src_frame=None, target=None, dtype=np.float64):
    """(out [B][bands][target], frame_max [B][T]): out[b][i][j] = mean of mag[b][src_frame[j]][edges[i]:edges[i + 1]] /
    ref[b], a zero column where src_frame[j] is outside [0, T); frame_max[b][t] = the largest of the frame's F bins, in
    the input's own type (a maximum rounds nothing).  Spectra hold no NaN (the header's precondition): on one the kernel's
    fmaxf passes over it while np.max here hands it on, so the two part only outside the contract."""
    mag = np.asarray(mag)
    B = mag.shape[0]
    target = T if target is None else target
    src = np.arange(target) if src_frame is None else np.asarray(src_frame, np.int64)
    assert len(src) == target
    x = mag[:, :T, :F].astype(dtype)
    bands = len(edges) - 1
    means = np.zeros((B, bands, T), dtype)
    for i in range(bands):
        lo, hi = int(edges[i]), int(edges[i + 1])
        means[:, i, :] = x[:, :, lo:hi].sum(axis=2, dtype=dtype) / dtype(hi - lo)
    ok = (src >= 0) & (src < T)
    out = np.where(ok[None, None, :], means[:, :, np.where(ok, src, 0)], dtype(0))
    out = out / _ref(ref, B, dtype)[:, None, None]
    return out.astype(dtype), mag[:, :T, :F].max(axis=2)


def band_abs_means(mag, T, F, edges, src_frame=None, target=None):
    """[B][bands][target] float64: mean |x| of every band, the scale of the compress_bands bar."""
    return compress_bands(np.abs(np.asarray(mag, np.float64)), T, F, edges, None, src_frame, target)[0]


def compress_bands_bar(F, edges, absmean, ref, fast_path=False):
    """[B][bands][target]: the bar of the module docstring.  fast_path: the compile-time edges, where every band is
    summed over registers and reduced across the wave."""
    q = maxq_of(F)
    lo, hi = np.asarray(edges[:-1], np.int64), np.asarray(edges[1:], np.int64)
    c = np.where((hi <= 64) & (not fast_path), hi - lo + 2, q + 8).astype(np.float64)
    return c[None, :, None] * U * absmean / np.abs(_ref(ref, absmean.shape[0], np.float64))[:, None, None]


def _select(spec, T, F, src_frame, band_min, bands, fill):
    """[B][bands][frames] (+ trailing axes of spec): spec[b][src_frame[b][j]][band_min[b] + r], `fill` outside."""
    B, frames = src_frame.shape
    lo = np.zeros(B, np.int64) if band_min is None else np.asarray(band_min, np.int64)
    t = np.asarray(src_frame, np.int64)[:, None, :]                     # [B][1][frames]
    f = lo[:, None, None] + np.arange(bands)[None, :, None]             # [B][bands][1]
    ok = (t >= 0) & (t < T) & (f >= 0) & (f < F)
    got = spec[np.arange(B)[:, None, None], np.where(ok, t, 0), np.where(ok, f, 0)]
    ok = ok.reshape(ok.shape + (1,) * (got.ndim - 3))
    return np.where(ok, got, fill)


def short_window(mag, phase, T, F, src_frame, band_min, bands, ref, mode, dtype=np.float64):
    """out [B][bands][frames].  mag [B][rows][ldf]; phase [B][rows][ldf][2] (re, im).  mode 0: mag / ref;
    1: log10(1000 mag + 1) / its largest value over the window (0 / 0 = NaN for a window of zeros, as the reference);
    2: (atan2(im, re) + 3.15) / 6.3, a cell outside the spectrogram being 0 + 0i."""
    src_frame = np.asarray(src_frame)
    B = src_frame.shape[0]
    if mode == 2:
        q = _select(np.asarray(phase), T, F, src_frame, band_min, bands, 0.0).astype(dtype)
        return ((np.arctan2(q[..., 1], q[..., 0]) + dtype(3.15)) / dtype(6.3)).astype(dtype)
    m = _select(np.asarray(mag), T, F, src_frame, band_min, bands, 0.0).astype(dtype)
    if mode == 0:
        return m if ref is None else (m / _ref(ref, B, dtype)[:, None, None]).astype(dtype)
    assert mode == 1
    lg = np.log10(m * dtype(1000.0) + dtype(1.0)).astype(dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (lg / lg.max(axis=(1, 2), keepdims=True)).astype(dtype)


def gather_frames(src, T, F, elem, src_frame, table_stride, n_out, band_min, bands, ldf_out):
    """out [B][n_out][ldf_out][elem]: src[b][src_frame[b * table_stride + j]][band_min + k], zero where the frame is
    outside [0, T), the bin outside [0, F) or k >= bands.  src [B][rows][ldf * elem].  Copies: the input's type."""
    src = np.asarray(src)
    B = src.shape[0]
    s = src.reshape(B, src.shape[1], -1, elem)
    tab = np.asarray(src_frame, np.int64).ravel()
    out = np.zeros((B, n_out, ldf_out, elem), src.dtype)
    for b in range(B):
        for j in range(n_out):
            t = tab[b * table_stride + j]
            if not 0 <= t < T:
                continue
            for k in range(bands):
                if 0 <= band_min + k < F:
                    out[b, j, k] = s[b, t, band_min + k]
    return out


def amplitude_to_db(mag, T, F, ref, window_max, amin, top_db, dtype=np.float64):
    """out [B][T][ldf]: 20 log10(max(amin, |mag|)) - 20 log10(max(amin, |ref|)), floored at the same expression of
    window_max minus top_db when top_db >= 0; pad bins 0."""
    mag = np.asarray(mag)
    B, ldf = mag.shape[0], mag.shape[2]
    amin = dtype(amin)
    lref = dtype(20.0) * np.log10(np.maximum(amin, np.abs(_ref(ref, B, dtype))))
    out = np.zeros((B, T, ldf), dtype)
    v = dtype(20.0) * np.log10(np.maximum(amin, np.abs(mag[:, :T, :F].astype(dtype)))) - lref[:, None, None]
    if top_db >= 0:
        floor = (dtype(20.0) * np.log10(np.maximum(amin, np.asarray(window_max).astype(dtype))) - lref) - dtype(top_db)
        v = np.maximum(v, floor[:, None, None])
    out[:, :, :F] = v
    return out


def db_to_amplitude(db, T, F, ref, dtype=np.float64):
    """out [B][T][ldf]: ref 10^(db / 20); pad bins 0."""
    db = np.asarray(db)
    B, ldf = db.shape[0], db.shape[2]
    out = np.zeros((B, T, ldf), dtype)
    out[:, :, :F] = _ref(ref, B, dtype)[:, None, None] * np.power(dtype(10.0), dtype(0.05) * db[:, :T, :F].astype(dtype))
    return out


def spectral_flatness(mag, T, F, amin, dtype=np.float64):
    """out [B][T]: exp(mean log max(amin, mag^2)) / mean max(amin, mag^2) over the F bins of a frame."""
    x = np.asarray(mag)[:, :T, :F].astype(dtype)
    pw = np.maximum(dtype(amin), x * x)
    return (np.exp(np.log(pw).mean(axis=2, dtype=dtype)) / pw.mean(axis=2, dtype=dtype)).astype(dtype)


def window_errors(got, ref64):
    """[B]: largest |got - ref64| of every window; NaNs must sit at the same places."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref64))
    d = np.where(np.isnan(ref64), 0.0, np.abs(got - ref64)).reshape(len(got), -1)
    return d.max(axis=1)


def window_scales(ref64):
    r = np.asarray(ref64, np.float64).reshape(len(ref64), -1)
    return np.where(np.isnan(r), 0.0, np.abs(r)).max(axis=1)


def transcendental_bar(e_f32numpy, scale):
    return 2.5 * np.asarray(e_f32numpy) + 4.0 * U * np.asarray(scale)


# ---------------------------------------------------------------------------------------------------------------------
# the integer glue (exact)
# ---------------------------------------------------------------------------------------------------------------------
def round_clamp(x, lo, hi):
    """int32 [n]: clamp(rint(x), lo, hi), half to even; NaN -> lo."""
    v = np.rint(np.asarray(x, np.float64))
    out = np.empty(v.shape, np.int64)
    nan = np.isnan(v)
    out[nan] = lo
    out[~nan] = np.clip(v[~nan], lo, hi).astype(np.int64)
    return out.astype(np.int32)


def argmax_rows(p):
    """int32 [n]: the first largest element among those of the row that are no NaN; 0 for a row of NaNs."""
    p = np.asarray(p)
    out = np.zeros(len(p), np.int32)
    for i, row in enumerate(p):
        valid = np.flatnonzero(~np.isnan(row))
        if len(valid):
            out[i] = valid[np.argmax(row[valid])]
    return out


def resize_table(start, end, T, frames):
    """int32 [n][frames]: source frame of column j of _resize(X[:, start:end], frames) (util_audio.py:384-409) with
    numpy's slice clamping to [0, T]; -1 = zero column.  Written per column from the rule's four cases:
    empty -> zeros; len >= frames -> the first `frames`; len < 3 -> the first once, then the last; else the first, the
    inner len - 2 tiled floor((frames - 2) / (len - 2)) times, then as many of the last frames as are still missing."""
    out = np.empty((len(start), frames), np.int32)
    for b, (s, t) in enumerate(zip(start, end)):
        s = min(max(int(s), 0), T)
        t = min(max(int(t), s), T)
        n = t - s
        if n == 0:
            row = [-1] * frames
        elif n >= frames:
            row = list(range(s, s + frames))
        elif n < 3:
            row = [s] + [t - 1] * (frames - 1)
        else:
            inner = list(range(s + 1, t - 1)) * ((frames - 2) // (n - 2))
            tail = frames - 1 - len(inner)
            row = [s] + inner + list(range(t - tail, t))
        out[b] = row
    return out


def note_select(program, pitch, onset, end, prog_group, n_prog, pitch_lo, n_pitch, tail_frames, bank_frames):
    """(guess_index, guess_frames) int32 [n]: prog_group[clamp(program)] * n_pitch + clamp(pitch - pitch_lo);
    min(max(end - onset, 0) + tail_frames, bank_frames).  program / prog_group None => group 0."""
    pitch = np.asarray(pitch, np.int64)
    pr = np.zeros(len(pitch), np.int64) if program is None else np.clip(np.asarray(program, np.int64), 0, n_prog - 1)
    g = np.zeros(len(pitch), np.int64) if prog_group is None else np.asarray(prog_group, np.int64)[pr]
    idx = g * n_pitch + np.clip(pitch - pitch_lo, 0, n_pitch - 1)
    d = np.maximum(np.asarray(end, np.int64) - np.asarray(onset, np.int64), 0) + tail_frames
    return idx.astype(np.int32), np.minimum(d, bank_frames).astype(np.int32)


def pack_events(n, window0, it, pitch, program, velocity, onset, end):
    """int32 [n][7]: {window0 + i, iter, pitch, program, velocity, onset, end}; a None column is -1."""
    ev = np.full((n, 7), -1, np.int32)
    ev[:, 0] = window0 + np.arange(n)
    ev[:, 1] = it
    for c, col in enumerate((pitch, program, velocity, onset, end)):
        if col is not None:
            ev[:, 2 + c] = col
    return ev


def affine_i32(x, mul, add):
    """int32 [n]: x * mul + add in 32-bit two's complement."""
    v = np.asarray(x, np.int64) * mul + add
    return ((v + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def spectra(B, T, F, seed, kind='mixed', gap_rows=2, pad=8):
    """float32 [B][T + gap_rows][ldf_of_bins(F) + pad]: NaN in the gap rows and the pad bins (a read of either poisons
    the output); windows scaled 1, 3, 1e-3.  kind 'mixed': window 0 non-negative, 1 of both signs, 2 negative
    throughout; 'mag': all non-negative with exact zeros; 'wide': non-negative, log-uniform over 1e-9 .. 10."""
    rng = np.random.default_rng(seed)
    ldf = ldf_of_bins(F) + pad
    h = np.full((B, T + gap_rows, ldf), np.nan, np.float32)
    scale = np.array([1.0, 3.0, 1e-3])
    for b in range(B):
        if kind == 'wide':
            x = 10.0 ** rng.uniform(-9.0, 1.0, (T, F))
        else:
            x = rng.standard_normal((T, F)) * scale[b % 3]
            if kind == 'mag':
                x = np.abs(x)
                x[rng.random((T, F)) < 0.05] = 0.0
            elif b % 3 == 0:
                x = np.abs(x)
            elif b % 3 == 2:
                x = -np.abs(x) - 1e-6
        h[b, :T, :F] = x
    return h


def phases(B, T, F, seed, gap_rows=2, pad=8):
    """float32 [B][T + gap_rows][ldf][2] unit phases with angles in (-pi + 0.01, pi - 0.01); frame 0, bins 12 .. 16 of
    every window hold 1, i, -1, -i and 0 + 0i; NaN in the gap rows and pad bins."""
    rng = np.random.default_rng(seed)
    ldf = ldf_of_bins(F) + pad
    h = np.full((B, T + gap_rows, ldf, 2), np.nan, np.float32)
    a = rng.uniform(-np.pi + 0.01, np.pi - 0.01, (B, T, F))
    h[:, :T, :F, 0], h[:, :T, :F, 1] = np.cos(a), np.sin(a)
    h[:, 0, 12:17] = np.array([[1, 0], [0, 1], [-1, 0], [0, -1], [0, 0]], np.float32)
    return h
