"""Float64 restatement of the STFT / iSTFT the HIP kernels compute (amt_stft.hip), the same operations in float32 on
the CPU, the error measures the STFT tests assert, and the geometry matrix they walk.  Test infrastructure: imported
by test_stft_reference_cpu.py (no GPU) and test_gpu_stft_geometry.py.

Independent of oracle/audio.py (test_stft_reference_cpu.py ties the two together): reflect padding of n_fft // 2 when
centred, periodic Hann window, numpy's float64 rfft / irfft, librosa's window-sum-of-squares normalisation.

Bars (all relative to float64; u = 2^-24, the unit roundoff of float32):

  STFT   for every frame t:  ||got_t - ref_t||_2 <= 8 u log2(n_fft) max(||ref_t||_2, ||ref_partner||_2)
         -- Higham's bound for a radix FFT with float32 twiddles, eta log2(N) ||x||_2, taken with the constant 8.
         `partner` is the other frame of the pair (2j, 2j + 1) the kernel packs into ONE complex transform: a quiet frame
         beside a loud one inherits the loud one's rounding, a quiet PAIR must be accurate at its own scale.
  iSTFT  with wgt = min(wss, 1):  max |(got - ref) wgt| <= 8 u log2(n_fft) max |ref wgt|
         -- the weight removes only the ill-conditioning of x / w where one frame with a tiny window value covers a
         sample; where wss > 1 (all of a centred hop <= N/2 output) the weight is 1.  Where wss is not above float32
         tiny (librosa leaves those samples undivided, and the accumulator is 0): |got| <= bar max |ref|.
"""
import numpy as np
import scipy.fft

U = 2.0 ** -24
TINY32 = float(np.finfo(np.float32).tiny)

N_FFTS = (256, 512, 1024, 2048, 4096)


def hops_of(n_fft):
    """N/8, N/4, N/2, N and one hop that is not a power of two."""
    return (n_fft // 8, n_fft // 4, n_fft // 2, n_fft, 100 if n_fft == 256 else 441)


GEOMETRIES = [(n, h, c) for n in N_FFTS for h in hops_of(n) for c in (1, 0)]


def bar(n_fft):
    return 8.0 * U * np.log2(n_fft)


def n_frames(L, n_fft, hop, center):
    return 1 + L // hop if center else 1 + (L - n_fft) // hop


def out_len(T, n_fft, hop, center):
    return hop * (T - 1) if center else n_fft + hop * (T - 1)


def lengths_of(n_fft, hop, center):
    """The shortest signal the entry accepts, an odd and an even frame count, one length off the hop grid."""
    if center:
        return [n_fft // 2 + 1, 36 * hop, 37 * hop, 21 * hop + hop // 3 + 1]
    return [n_fft, n_fft + 36 * hop, n_fft + 37 * hop, n_fft + 21 * hop + hop // 3 + 1]


def generic_gh(hop):
    """Output hops per workgroup of the generic iSTFT kernel (launch_istft: 8192 floats of LDS accumulator)."""
    return min(16, 8192 // hop)


def stream_gh(n_fft, hop, center, T, B):
    """Output hops per workgroup of the streaming iSTFT kernel (launch_istft: 32, halved down to 4 while fewer than
    2048 workgroups would result); None where the generic kernel runs."""
    if n_fft % 1024 or hop * 4 != n_fft:
        return None
    total = (n_fft // 2 if center else 0) + out_len(T, n_fft, hop, center)
    gh = 32
    while gh > 4 and ((total + gh * hop - 1) // (gh * hop)) * B < 2048:
        gh >>= 1
    return gh


def inverse_frames(n_fft, hop, center):
    """T = 1, 2, 3 and the frame counts that put the last frame one before, on and one after the first segment boundary
    of the kernel that serves the geometry at a small batch (GH hops: 4 for the streaming kernel)."""
    gh = 4 if stream_gh(n_fft, hop, center, 8, 1) is not None else generic_gh(hop)
    return sorted({1, 2, 3, gh, gh + 1, gh + 2})


# ---------------------------------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------------------------------
def hann64(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def _frames(y, n_fft, hop, center):
    if center:
        y = np.pad(y, n_fft // 2, mode='reflect')
    T = 1 + (len(y) - n_fft) // hop
    return y[np.arange(n_fft)[:, None] + hop * np.arange(T)[None, :]]


def stft64(y, n_fft, hop, center):
    """complex128 [1 + n_fft // 2, T]."""
    fr = _frames(np.asarray(y, dtype=np.float64), n_fft, hop, center)
    return np.fft.rfft(fr * hann64(n_fft)[:, None], axis=0)


def stft32(y, n_fft, hop, center):
    """The same in float32 (pocketfft's single-precision transform): complex64."""
    fr = _frames(np.asarray(y, dtype=np.float32), n_fft, hop, center)
    out = scipy.fft.rfft(fr * hann64(n_fft).astype(np.float32)[:, None], axis=0)
    assert out.dtype == np.complex64
    return out


def _overlap_add(ytmp, w2, hop, dtype):
    n_fft, T = ytmp.shape
    acc = np.zeros(n_fft + hop * (T - 1), dtype=dtype)
    wss = np.zeros_like(acc)
    for t in range(T):
        acc[t * hop:t * hop + n_fft] += ytmp[:, t]
        wss[t * hop:t * hop + n_fft] += w2
    y = acc.copy()
    nz = wss > TINY32
    y[nz] /= wss[nz]
    return y, wss, acc


def _trim(arrs, n_fft, center):
    return tuple(a[n_fft // 2:len(a) - n_fft // 2] for a in arrs) if center else tuple(arrs)


def istft64(F, hop, center):
    """(y, wss, acc), float64: the overlap-add divided by the window sum of squares where that exceeds float32 tiny,
    the window sum of squares, the un-normalised accumulator -- all trimmed by n_fft // 2 when centred."""
    F = np.asarray(F, dtype=np.complex128)
    n_fft = 2 * (F.shape[0] - 1)
    win = hann64(n_fft)
    ytmp = win[:, None] * np.fft.irfft(F, n=n_fft, axis=0)
    return _trim(_overlap_add(ytmp, win * win, hop, np.float64), n_fft, center)


def istft32(F, hop, center):
    F = np.asarray(F, dtype=np.complex64)
    n_fft = 2 * (F.shape[0] - 1)
    win = hann64(n_fft).astype(np.float32)
    x = scipy.fft.irfft(F, n=n_fft, axis=0)
    assert x.dtype == np.float32
    return _trim(_overlap_add(win[:, None] * x, win * win, hop, np.float32), n_fft, center)


# ---------------------------------------------------------------------------------------------------------------------
# signals
# ---------------------------------------------------------------------------------------------------------------------
def tonal(L, seed):
    """Two partials + noise under a decay (test_gpu_audio._signal)."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / 44100.0
    y = 0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.3 * np.sin(2 * np.pi * 1333.7 * t + 1.0)
    y += 0.05 * rng.standard_normal(L)
    y *= np.exp(-t * 1.5)
    return y.astype(np.float32)


def white(L, seed):
    return np.random.default_rng(seed).standard_normal(L).astype(np.float32)


def loud_quiet_switch(L, n_fft, hop, center):
    """First sample of an even frame near the middle of the signal (at least one sample in)."""
    pad = n_fft // 2 if center else 0
    j = max(n_frames(L, n_fft, hop, center) // 4, 1)
    while 2 * j * hop - pad <= 0:
        j += 1
    return min(2 * j * hop - pad, L)


def loud_quiet(L, seed, n_fft, hop, center):
    """Noise + a partial, x 1e3 before the first sample of an even frame and x 1e-3 from it on: every frame pair
    (2j, 2j + 1) that starts there or later is quiet as a whole."""
    rng = np.random.default_rng(seed)
    y = 0.3 * rng.standard_normal(L) + 0.5 * np.sin(2 * np.pi * 997.0 * np.arange(L) / 44100.0)
    s = loud_quiet_switch(L, n_fft, hop, center)
    y[:s] *= 1e3
    y[s:] *= 1e-3
    return y.astype(np.float32)


def signals(L, seed, n_fft, hop, center):
    """The three test signals as one batch [3, L] (names in SIGNALS)."""
    return np.stack([tonal(L, seed), white(L, seed + 1), loud_quiet(L, seed + 2, n_fft, hop, center)])


SIGNALS = ('tonal', 'white', 'loud_quiet')


def ramped_spectrum(L, seed, n_fft, hop, center, which=1):
    """A spectrogram that is NOT a consistent STFT: stft64 of a test signal times a ramp over the bins."""
    y = signals(L, seed, n_fft, hop, center)[which]
    return stft64(y, n_fft, hop, center) * np.linspace(0.2, 1.0, n_fft // 2 + 1)[:, None]


def split_magphase32(F):
    """float32 magnitudes and float32 unit phases of a complex128 spectrogram (1 + 0i where it is 0), and the float64
    product of the two AS ROUNDED -- what an iSTFT fed with them is asked to invert."""
    F = np.asarray(F, dtype=np.complex128)
    mag = np.abs(F)
    ph = np.where(mag > 0, F / np.where(mag > 0, mag, 1.0), 1.0 + 0.0j)
    mag32 = mag.astype(np.float32)
    ph32 = ph.astype(np.complex64)
    return mag32, ph32, mag32.astype(np.float64) * ph32.astype(np.complex128)


# ---------------------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------------------
def pair_norms(ref):
    """[T]: max(||ref_t||, ||ref_partner||), partner = the other frame of the pair (2j, 2j + 1); a last odd frame has
    none."""
    nrm = np.sqrt((np.abs(np.asarray(ref)) ** 2).sum(axis=0))
    T = len(nrm)
    partner = np.arange(T) ^ 1
    partner[partner >= T] = T - 1
    return np.maximum(nrm, nrm[partner])


def stft_frame_errors(got, ref):
    """[T]: ||got_t - ref_t||_2 / max(||ref_t||_2, ||ref_partner||_2); got, ref [F, T] (magnitudes or complex).  A pair
    of silent frames must be reproduced exactly (0), else inf."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    d = np.sqrt((np.abs(got.astype(ref.dtype) - ref) ** 2).sum(axis=0))
    pn = pair_norms(ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(pn > 0, d / np.where(pn > 0, pn, 1.0), np.where(d > 0, np.inf, 0.0))


def stft_error(got, ref):
    return float(stft_frame_errors(got, ref).max())


def istft_error(got, y, wss):
    """max of: max |(got - y) wgt| / max |y wgt| with wgt = min(wss, 1); and, over the samples whose wss does not exceed
    float32 tiny, max |got| / max |y|."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == y.shape == wss.shape
    wgt = np.minimum(wss, 1.0)
    e = float(np.abs((got - y) * wgt).max() / np.abs(y * wgt).max())
    zero = wss <= TINY32
    if zero.any():
        e = max(e, float(np.abs(got[zero]).max() / np.abs(y).max()))
    return e


def relmax_of_window(got, ref):
    """The measure test_gpu_audio.py uses (REL = 1e-4): largest difference over the window's largest magnitude."""
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max() / np.abs(ref).max())


def phase_compared(mag64):
    """Bins whose phase is compared: float64 magnitude above 1e-3 of its frame's largest."""
    return mag64 > 1e-3 * mag64.max(axis=0, keepdims=True)
