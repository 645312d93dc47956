"""The beat tracker's rule (csrc/amt_beat_core.h) restated in numpy and Python integers, independently of the
core: Ellis's dynamic programme (2007) in the form of librosa.beat.beat_track, all-integer after one float32 step per
cell.  Also the host tables (restated from amt_saga.beat), the corpora the CPU program and the GPU tests share, and the
click songs.  No device, no amt_saga import."""
import math

import numpy as np

E_MAX = 65535
MAX_LAG = 1024


# ---- the envelope ----
def compress(mag, ref):
    """c [T, F] int64 in 0..1024: float32 division, minimum, square root, scale, truncation."""
    mag = np.asarray(mag, np.float32)
    with np.errstate(all='ignore'):
        x = mag / np.float32(ref)
        ok = x > 0
        x = np.where(ok, np.minimum(x, np.float32(1)), np.float32(0)).astype(np.float32)
        c = np.sqrt(x) * np.float32(1024) + np.float32(0.5)
    assert c.dtype == np.float32
    return np.where(ok, c.astype(np.int64), 0)


def flux_of(mag, ref):
    T = mag.shape[0]
    if not ref > 0:
        return [0] * T
    c = compress(mag, ref)
    out = [0] * T
    for t in range(1, T):
        out[t] = int(np.maximum(c[t] - c[t - 1], 0).sum())
    return out


def envelope_from_flux(flux, w, live=True):
    """e (list of int) from the flux: local mean, excess, scale."""
    T = len(flux)
    if T == 0 or not live:
        return [0] * T
    d = []
    for t in range(T):
        lo, hi = max(0, t - w), min(T - 1, t + w)
        d.append(max(0, flux[t] - sum(flux[lo:hi + 1]) // (hi - lo + 1)))
    q = math.isqrt(sum(v * v for v in d) // T)
    if q == 0:
        return [0] * T
    return [min(E_MAX, v * 256 // q) for v in d]


def envelope(mag, ref, w):
    """(flux, e) of one song, lists of int."""
    flux = flux_of(mag, ref)
    return flux, envelope_from_flux(flux, w, bool(ref > 0))


# ---- the host tables ----
def tables(sr, hop, bpm=(40, 240), tightness=100, mean_s=0.5, centre=120.0, octaves=1.0):
    fps = sr / hop
    lag_lo, lag_hi = max(1, int(math.floor(60.0 * fps / bpm[1]))), int(math.ceil(60.0 * fps / bpm[0]))
    return (lag_lo, lag_hi, int(round(mean_s * fps))) + lag_tables(lag_lo, lag_hi, fps, tightness, centre, octaves)


def lag_tables(lag_lo, lag_hi, fps, tightness=100, centre=120.0, octaves=1.0):
    prior = []
    for L in range(lag_lo, lag_hi + 1):
        z = math.log2(60.0 * fps / L / centre) / octaves
        prior.append(int(round(32767 * math.exp(-0.5 * z * z))))
    pitch = 2 * lag_hi + 1
    pen = np.zeros((lag_hi - lag_lo + 1, pitch), np.int32)
    for P in range(lag_lo, lag_hi + 1):
        for tau in range((P + 1) // 2, 2 * P + 1):
            pen[P - lag_lo, tau] = int(round(tightness * 1024 * math.log(tau / P) ** 2))
    return np.asarray(prior, np.int32), pen


# ---- the track ----
def autocorrelation(e, lag_hi):
    T = len(e)
    v = np.asarray(e, np.int64)
    a = [0] * (2 * lag_hi + 2)
    for L in range(1, 2 * lag_hi + 2):
        if T - L > 0:
            a[L] = int((v[:T - L] * v[L:]).sum()) // (T - L)
    return a


def tempo(e, lag_lo, lag_hi, prior):
    """The period, or 0 for a song without beats."""
    a = autocorrelation(e, lag_hi)
    best, P = 0, 0
    for L in range(lag_lo, lag_hi + 1):
        s = int(prior[L - lag_lo]) * (2 * a[L] + a[2 * L])
        if s > best:                         # (a tie stays with the smaller lag; nothing above 0: no beats)
            best, P = s, L
    return P


def local_score(e):
    T = len(e)
    return [(e[t - 1] if t else 0) + 2 * e[t] + (e[t + 1] if t + 1 < T else 0) for t in range(T)]


def track(e, lag_lo, lag_hi, prior, pen):
    """dict(period, beats, C, back) of one envelope (a sequence of int)."""
    e = [int(v) for v in e]
    T = len(e)
    P = tempo(e, lag_lo, lag_hi, prior) if T else 0
    if P == 0:
        return dict(period=0, beats=[], C=[0] * T, back=[-1] * T)
    ls = local_score(e)
    H = (P + 1) // 2
    row = np.asarray(pen[P - lag_lo], np.int64)
    C, back = np.zeros(T, np.int64), [-1] * T             # (C < 2^38: int64 holds it)
    for t in range(T):
        best, arg = 0, -1
        hi = min(2 * P, t)
        if hi >= H:
            v = C[t - hi:t - H + 1][::-1] - row[H:hi + 1]             # tau ascending
            k = int(np.argmax(v))                        # the first maximum: a tie stays with the smaller tau
            if v[k] > 0:                                 # ... and with the 0
                best, arg = int(v[k]), t - (H + k)
        C[t], back[t] = ls[t] + best, arg
    C = [int(v) for v in C]
    lo = max(0, T - P)
    b = lo + max(range(T - lo), key=lambda i: (C[lo + i], -i))
    found = []
    while b >= 0:
        found.append(b)
        b = back[b]
    found.reverse()
    n, total = len(found), sum(ls[b] ** 2 for b in found)
    keep = [k for k, b in enumerate(found) if 4 * ls[b] ** 2 * n >= total]
    beats = found[keep[0]:keep[-1] + 1] if keep else []
    return dict(period=P, beats=beats, C=C, back=back)


def bound(T, lag_lo):
    return T // ((lag_lo + 1) // 2) + 1


# ---- corpora ----
ENV_F = (1, 7, 513, 1025, 2049)
ENV_T = (1, 2, 3, 63, 64, 65, 300)
ENV_W = (0, 1, 43, 1000)


def env_content(kind, T, F, seed):
    rng = np.random.default_rng(seed)
    if kind == 'silent':
        return np.zeros((T, F), np.float32)
    S = rng.random((T, F), dtype=np.float32) ** 2
    if kind == 'onsets':                     # bursts every 11 frames over a floor
        S *= np.float32(0.05)
        S[::11] += rng.random((len(S[::11]), F), dtype=np.float32)
    return S.astype(np.float32)


def env_corpus():
    """[(name, S [T, F], ref, ldf)]: every F x T, random and bursty content, refs at, below and above the maximum."""
    out = []
    for i, F in enumerate(ENV_F):
        for j, T in enumerate(ENV_T):
            kind = ('random', 'onsets')[(i + j) % 2]
            S = env_content(kind, T, F, 100 * i + j)
            top = float(S.max())
            ref = (top, top * 0.5, top * 2.0)[(i + 2 * j) % 3]          # 0.5: magnitudes above ref
            out.append(('%s F=%d T=%d' % (kind, F, T), S, np.float32(ref), (F + 3) // 4 * 4 + 4 * (j % 2)))
    out.insert(3, ('silent', env_content('silent', 40, 513, 0), np.float32(0.0), 516))
    out.insert(9, ('ref nan', env_content('random', 12, 7, 1), np.float32('nan'), 8))
    return out


DEFAULT_LAGS = (21, 130, 44100.0 / 512)


def impulses(T, period, first=0, height=1000):
    e = np.zeros(T, np.int64)
    e[first::period] = height
    return e


def track_corpus():
    """[(name, (lag_lo, lag_hi, fps), keyword arguments of the tables, [envelopes])]: one device call each.  Under the
    flat prior (1000 octaves wide) the own lag of an impulse train with silence behind it is its period, so every lag of a range is a period there."""
    rng = np.random.default_rng(11)
    out = []
    for lags in ((2, 4, 10.0), (5, 40, 30.0), DEFAULT_LAGS):
        lo, hi, _ = lags
        envs = [np.zeros(50, np.int64), np.full(3 * hi + 7, 300, np.int64), impulses(4 * hi, 10 ** 6, first=hi),
                np.zeros(0, np.int64), np.full(1, 9, np.int64)]
        for L in range(lo, hi + 1):
            envs.append(impulses(6 * L + 3, L, first=L // 3))
        envs += [np.full(lo - 1, 500, np.int64), np.full(lo, 500, np.int64), np.full(lo + 1, 500, np.int64)]
        for P in sorted({lo, lo + 1, (lo + hi) // 2, (lo + hi) // 2 + 1, hi}):
            H = (P + 1) // 2
            envs.append(impulses(P + H // 2 + 1, P))                     # P / 2 < T < 2 P
            for k in (-1, 0, 1):
                if 7 * H + k > 0:
                    envs.append(impulses(7 * H + k, P, first=1, height=4000) + rng.integers(0, 40, 7 * H + k))
        for T in (17, 200, 1111):
            envs.append(rng.integers(0, 2000, T))
            envs.append(np.minimum(E_MAX, (rng.random(T) ** 8 * 70000).astype(np.int64)))
        out.append(('lags %d..%d' % (lo, hi), lags, {}, envs))
        out.append(('lags %d..%d, flat prior' % (lo, hi), lags, dict(octaves=1000.0, tightness=400),
                    [np.concatenate([impulses(6 * L, L, first=L // 3), np.zeros(2 * L + 3, np.int64)]) for L in range(lo, hi + 1)]))
    return out


# ---- click songs ----
def click_song(bpm, sr=44100, seconds=20.0, first=0.7, tail=2.0, jitter_s=0.0, slow=0.0, seed=0):
    """(wave float32, gold beat times): a decaying two-partial note plus a noise click per beat, a weaker off-beat eighth
    on every second beat; the last `tail` seconds silent.  jitter_s: Gaussian jitter per beat; slow: every beat interval
    longer than the last by that fraction."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    y = np.zeros(n, np.float64)
    times, t, step = [], first, 60.0 / bpm
    while t < seconds - tail:
        times.append(t)
        t += step
        step *= 1.0 + slow
    gold = np.asarray(times)
    if jitter_s:
        gold = gold + rng.normal(0.0, jitter_s, len(gold))

    def hit(at, gain, pitch):
        i0 = int(round(at * sr))
        m = min(n - i0, int(0.25 * sr))
        if m <= 0:
            return
        k = np.arange(m) / sr
        y[i0:i0 + m] += gain * np.exp(-k / 0.08) * (np.sin(2 * np.pi * pitch * k) + 0.5 * np.sin(2 * np.pi * 2 * pitch * k))
        c = min(m, int(0.01 * sr))
        y[i0:i0 + c] += gain * 0.8 * rng.standard_normal(c) * np.exp(-np.arange(c) / (0.003 * sr))
    for i, at in enumerate(gold):
        hit(at, 0.5, 220.0 * 2 ** ((i % 4) / 12.0))
        if i % 2 == 1 and i + 1 < len(gold):
            hit(0.5 * (at + gold[i + 1]), 0.05, 440.0)
    y[int((seconds - tail) * sr):] = 0.0
    return (y / max(1.0, np.abs(y).max())).astype(np.float32), gold


def stft_mag(wave, n_fft=2048, hop=512):
    """Centred, reflect-padded, periodic-Hann magnitudes [1 + len // hop, n_fft // 2 + 1] float32 (numpy, host)."""
    y = np.pad(np.asarray(wave, np.float64), n_fft // 2, mode='reflect')
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    T = 1 + len(wave) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(T)[:, None]
    return np.abs(np.fft.rfft(y[idx] * win, axis=1)).astype(np.float32)


def beat_track_mag(mag, sr, hop, **kw):
    """dict(period, beats (frames), times) of one spectrogram under the default tables."""
    lag_lo, lag_hi, w, prior, pen = tables(sr, hop, **kw)
    _, e = envelope(mag, np.float32(mag.max()) if mag.size else np.float32(0), w)
    r = track(e, lag_lo, lag_hi, prior, pen)
    r['times'] = [b * hop / sr for b in r['beats']]
    return r


def click_conditions(times, period, gold, bpm, sr=44100, hop=512, count=None, half=False):
    """The conditions of the click songs; raises AssertionError with the figures."""
    times, two_hops = np.asarray(times), 2.0 * hop / sr
    want = 60.0 * sr / hop / bpm * (2 if half else 1)
    assert abs(period - want) <= 1.0, ('period', period, want)
    if half:
        assert all(np.abs(gold - t).min() <= two_hops for t in times), 'a beat off the gold beats'
        assert count is None or len(times) == count, ('count', len(times), count)
        return
    assert len(times) == len(gold), ('count', len(times), len(gold))
    assert all(np.abs(gold - t).min() <= two_hops for t in times), ('beat -> gold', float(max(np.abs(gold - t).min() for t in times)))
    assert all(np.abs(times - g).min() <= two_hops for g in gold), ('gold -> beat', float(max(np.abs(times - g).min() for g in gold)))
