"""Float64 definition of the device resampler (amt_resample.hip, amt_saga.audio.Resampler), a float32 CPU restatement of
the kernel's arithmetic, the error bar the GPU tests assert and the tone measurements of the quality tests.  Test
infrastructure: imported by test_resample_reference_cpu.py (no GPU) and test_gpu_resample.py.  numpy only.

Rational polyphase resampling with a Kaiser-windowed sinc, zero phase:

    g = gcd(sr_in, sr_out);  L = sr_out / g;  M = sr_in / g;  R = max(L, M)
    Z = 32 (zero crossings per side),  beta = 10.0,  rolloff = 0.88
    h[k] = L (rolloff / R) sinc(rolloff k / R) I0(beta sqrt(1 - (k / (Z R))^2)) / I0(beta),   integer |k| <= Z R
    y[n] = sum over m with |n M - m L| <= Z R of  x[m] h[n M - m L],     x[m] = 0 outside [0, n_in)
    n_out = ceil(n_in L / M),   n = 0 .. n_out - 1

With C interleaved channels x[m] is the mean over the channels.  Output n sits at time n / sr_out.

Bar for every output sample against this definition (u = 2^-24, the unit roundoff of float32):

    |y_gpu - y_f64| <= (taps_n + C + 2) u sum_m |h[n M - m L]| mean_c |x[m][c]|

over that sample's own taps inside the signal: the forward bound of a float32 dot product of taps_n terms (any order,
with or without fused multiply-adds: taps_n u), the rounding of the coefficients to float32 (u), of the products' input
x[m] as a float32 mean of C channels (C - 1 additions and a division: C u), and one u of slack for the float64 side.
"""
import math

import numpy as np

U = 2.0 ** -24
Z = 32
BETA = 10.0
ROLLOFF = 0.88
R_MAX = 2048

# the rate pairs of the tests (the first seven are the issue's; the last walks several LDS pieces per tile and L = 40)
PAIRS = [(48000, 44100), (96000, 44100), (22050, 44100), (16000, 44100), (8000, 44100), (44100, 48000), (44100, 22050)]
STEEP = (44100, 4000)
TILE = 1024                    # outputs per workgroup of the kernel (AMT_RS_TILE)


def ratio(sr_in, sr_out):
    """(L, M, R) of a rate pair."""
    g = math.gcd(int(sr_in), int(sr_out))
    L, M = int(sr_out) // g, int(sr_in) // g
    return L, M, max(L, M)


def out_len(n_in, sr_in, sr_out):
    L, M, _ = ratio(sr_in, sr_out)
    return -((-int(n_in) * L) // M)


def taps_max(sr_in, sr_out):
    """Most input samples one output uses: 2 Z R / L + 1."""
    L, _, R = ratio(sr_in, sr_out)
    return 2 * Z * R // L + 1


def h_of(k, sr_in, sr_out):
    """The filter at integer offsets k (any shape), float64; 0 outside |k| <= Z R."""
    L, _, R = ratio(sr_in, sr_out)
    k = np.asarray(k, dtype=np.int64)
    kf = k.astype(np.float64)
    inside = np.abs(k) <= Z * R
    u = np.where(inside, kf / (Z * R), 0.0)
    w = np.i0(BETA * np.sqrt(1.0 - u * u)) / np.i0(BETA)
    return np.where(inside, L * (ROLLOFF / R) * np.sinc(ROLLOFF * kf / R) * w, 0.0)


def mono(x):
    """float64 mean over the channels of [n] or [n, C]."""
    x = np.asarray(x, dtype=np.float64)
    return x if x.ndim == 1 else x.mean(axis=1)


def _taps(ns, n_in, sr_in, sr_out):
    """For outputs ns: m [len(ns), T] (ascending), h [len(ns), T] float64 and valid [len(ns), T] (the tap exists: inside
    the filter's support and inside the signal)."""
    L, M, R = ratio(sr_in, sr_out)
    ns = np.asarray(ns, dtype=np.int64)
    m_lo = -((-(ns * M - Z * R)) // L)                                   # ceil((n M - Z R) / L)
    m = m_lo[:, None] + np.arange(taps_max(sr_in, sr_out), dtype=np.int64)[None, :]
    k = ns[:, None] * M - m * L
    valid = (np.abs(k) <= Z * R) & (m >= 0) & (m < n_in)
    return m, h_of(k, sr_in, sr_out), valid


def resample_at(x, sr_in, sr_out, ns=None, block=4096):
    """The definition at outputs ns (default: all n_out of them).  x: [n_in] or [n_in, C].  Returns (y, scale, taps):
    y float64, scale = sum_m |h| mean_c |x[m][c]| over each sample's own taps, taps = how many there are."""
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[0]
    xm = mono(x)
    xa = np.abs(x) if x.ndim == 1 else np.abs(x).mean(axis=1)
    ns = np.arange(out_len(n_in, sr_in, sr_out), dtype=np.int64) if ns is None else np.asarray(ns, dtype=np.int64)
    y, scale, taps = (np.zeros(len(ns)) for _ in range(3))
    for i in range(0, len(ns), block):
        m, h, valid = _taps(ns[i:i + block], n_in, sr_in, sr_out)
        mc = np.clip(m, 0, n_in - 1)
        hv = np.where(valid, h, 0.0)
        y[i:i + block] = (xm[mc] * hv).sum(axis=1)
        scale[i:i + block] = (xa[mc] * np.abs(hv)).sum(axis=1)
        taps[i:i + block] = valid.sum(axis=1)
    return y, scale, taps


def bar(scale, taps, channels=1):
    return (taps + channels + 2) * U * scale


def resample_f32(x, sr_in, sr_out, ns=None):
    """The kernel's arithmetic in float32 on the CPU: coefficients rounded to float32, the channel mean as a float32 sum
    in channel order divided by C, every product rounded, added one by one in ascending m."""
    x = np.asarray(x, dtype=np.float32)
    n_in = x.shape[0]
    if x.ndim == 2:
        s = x[:, 0].copy()
        for c in range(1, x.shape[1]):
            s = s + x[:, c]
        x = s / np.float32(x.shape[1])
    ns = np.arange(out_len(n_in, sr_in, sr_out), dtype=np.int64) if ns is None else np.asarray(ns, dtype=np.int64)
    m, h, valid = _taps(ns, n_in, sr_in, sr_out)
    h32 = np.where(valid, h, 0.0).astype(np.float32)
    xv = x[np.clip(m, 0, n_in - 1)]
    acc = np.zeros(len(ns), dtype=np.float32)
    for j in range(m.shape[1]):
        acc = acc + xv[:, j] * h32[:, j]
    return acc


def phase_sums(sr_in, sr_out):
    """Sum of the coefficients of every phase p = n M mod L (an output's weights on a constant input)."""
    L, _, R = ratio(sr_in, sr_out)
    p = np.arange(L, dtype=np.int64)
    d = np.arange(-(Z * R // L) - 1, Z * R // L + 2, dtype=np.int64)
    return h_of(p[:, None] + d[None, :] * L, sr_in, sr_out).sum(axis=1)


def tone(f, sr, seconds, phase=0.3):
    return np.sin(2.0 * np.pi * f * np.arange(int(round(seconds * sr))) / sr + phase)


def middle_rms(y):
    """RMS over the middle half of a signal."""
    n = len(y)
    mid = np.asarray(y[n // 4:n - n // 4], dtype=np.float64)
    return float(np.sqrt(np.mean(mid * mid)))


def db(r):
    return 20.0 * np.log10(max(float(r), 1e-300))


def image_db(y, sr_out, f_tone, f_image):
    """Level of the spectral line at f_image relative to the one at f_tone, in dB, in the Hann-windowed spectrum of
    the middle half of y (each line taken as the largest bin within two bins of its frequency)."""
    n = len(y)
    mid = np.asarray(y[n // 4:n - n // 4], dtype=np.float64)
    spec = np.abs(np.fft.rfft(mid * np.hanning(len(mid))))

    def line(f):
        b = int(round(f * len(mid) / sr_out))
        return spec[max(b - 2, 0):b + 3].max()
    return db(line(f_image) / line(f_tone))
