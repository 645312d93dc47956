"""audio_complete (reference call surface) and AudioBatch (B windows at once).

Mirrors /root/reference/util_audio.py:32-527.  Spectra live in HBM frame-major
([T][ldf], ldf = F rounded up to 4) and are transposed to the reference's
[F, T] numpy layout only at the property boundary.  Every numeric step runs in
the HIP library (include/amt_saga.h); numpy is used for the host-visible views
and the integer index maps (_resize tables, frame<->second maps).
"""
import bisect
import ctypes as C
import math

import os

import numpy as np
import torch

from . import _lib, flac as _flac, png as _png, wav as _wav
from .device import empty, per_device, ptr, require_gpu, stream_ptr, to_dev, zeros

_PLANS = {}


def _stride0(t):
    """Elements between consecutive items of dim 0 (size-1 dims may carry stride 0)."""
    return t.stride(0) if t.shape[0] > 1 else max(t[0].numel(), 1)


def _plan(n_fft, hop, center):
    def build():
        lib = _lib.load()
        require_gpu()
        h = C.c_void_p()
        _lib.check(lib.amt_stft_plan_create(C.byref(h), int(n_fft), int(hop), int(bool(center))))
        return h
    return per_device(_PLANS, (int(n_fft), int(hop), bool(center)), build)


# Row pitch of the spectrograms in floats.  AMT_LDF_ALIGN=32 (128-byte rows) is a measured experiment, not a supported
# mode: the STFT's write traffic drops from 2.39 to 2.25 MB per window (3.55 -> 3.41 in total, PMC) at unchanged speed, the
# other kernels carry 2.7 % more bytes, and the host-side window-management helpers (gather_frames) assume the default
_LDF_ALIGN = int(os.environ.get('AMT_LDF_ALIGN', '4'))


def ldf_of(n_fft):
    return ((n_fft // 2 + 1) + _LDF_ALIGN - 1) // _LDF_ALIGN * _LDF_ALIGN


def fft_frequencies(sr, n_fft):
    return np.linspace(0, float(sr) / 2, int(1 + n_fft // 2), endpoint=True)


def midi_to_hz(m):
    return 440.0 * (2.0 ** ((np.asanyarray(m, dtype=np.float64) - 69.0) / 12.0))


def tone_to_fft_bin(fft_freq, tone):
    """audio_complete.midi_tone_to_FFT (util_audio.py:278-284): two bins below the first FFT bin above the tone, not
    below bin 0."""
    return max(bisect.bisect_right(fft_freq, midi_to_hz(tone)) - 2, 0)


def tone_bin_table(sr, n_fft, tone_lo, tone_hi):
    """int32 [tone_hi - tone_lo + 1]: tone_to_fft_bin of every MIDI tone tone_lo .. tone_hi -- the host table
    amt_note_features indexes with the step's decided pitches."""
    freq = fft_frequencies(sr, n_fft)
    return np.array([tone_to_fft_bin(freq, t) for t in range(int(tone_lo), int(tone_hi) + 1)], dtype=np.int32)


def resize_source_frames(t, target):
    """Index form of audio_complete._resize (util_audio.py:384-409): for a
    source of t frames, the source frame of each of `target` output columns;
    -1 = zero column (t == 0)."""
    if t <= 0:
        return np.full(target, -1, dtype=np.int32)
    if t == target:
        return np.arange(target, dtype=np.int32)
    if t < 3:
        return np.array([0] + [t - 1] * (target - 1), dtype=np.int32)
    if t < target:
        lim = min(1, int(round(t / 3)))            # always 1 for t >= 3 (:395)
        reps = (target - 2 * lim) // (t - 2 * lim)
        mid = list(range(lim, t - lim)) * reps
        n_tail = target - len(mid) - lim
        return np.array(list(range(lim)) + mid + list(range(t - n_tail, t)), dtype=np.int32)
    return np.arange(target, dtype=np.int32)


def band_edges(n_rows, bands):
    """Row ranges of compress_bands(log=True) (util_audio.py:451-456)."""
    ind = np.geomspace(1, n_rows, bands + 1).astype(np.int64)
    ind[0] = 0
    for i in range(bands):
        sub = ind[i + 1] - ind[i]
        if sub < 1:
            ind[i + 1] += -sub + 1
    return ind.astype(np.int32)


# ======================================================================================
# Batched, device-resident windows
# ======================================================================================
_DEV_TABLES = {}


def _dev_table(key, build):
    """Small constant index tables live on the device once: a pageable host-to-device copy
    inside the loop would drain the stream on every call."""
    return per_device(_DEV_TABLES, key, lambda: to_dev(build(), torch.int32))


class AudioBatch:
    """B equally long windows processed together.  State: wave [B, L] f32,
    mag [B, T, ldf] f32, ph [B, T, ldf, 2] f32 (unit complex), ref_max [B] f32."""

    def __init__(self, wave, n_fft, hop_length=None, center=True, sample_rate=44100):
        self.dev = require_gpu()
        self.N = int(n_fft)
        self.hl = int(hop_length) if hop_length is not None else int(math.floor(n_fft / 4))
        self.center = bool(center)
        self.sr = sample_rate
        self.F = self.N // 2 + 1
        self.ldf = ldf_of(self.N)
        self.plan = _plan(self.N, self.hl, self.center)
        self.lib = _lib.load()
        self.wave = None
        self.mag = self.ph = self.ref_max = None
        self._fmax = None            # (per-frame maxima [B, T], data_ptr of the mag they describe): compress_bands(fmax=True)
        self._max_scratch = None
        if wave is not None:
            w = to_dev(wave)
            if w.dim() == 1:
                w = w[None, :]
            self.wave = w.contiguous()
            self.B, self.L = self.wave.shape
            self.T = self.lib.amt_stft_frames(self.plan, int(self.L))
            if self.T < 0:
                _lib.check(self.T)

    # -- STFT / iSTFT --------------------------------------------------------------
    def stft(self, with_phase=True):
        """audio_complete.mag/.ph/.ref_mag for all windows (util_audio.py:139-174)."""
        B, T, ldf = self.B, self.T, self.ldf
        self._fmax = None
        self.mag = empty((B, T, ldf))
        self.ph = empty((B, T, ldf, 2)) if with_phase else None
        self.ref_max = empty((B,))
        _lib.check(self.lib.amt_stft_mag(
            self.plan, ptr(self.wave), B, int(self.L), _stride0(self.wave), ptr(self.mag),
            ptr(self.ph), ptr(self.ref_max), T, ldf, T * ldf, stream_ptr()))
        return self

    def istft(self):
        """audio_complete.wf from mag*ph (util_audio.py:94-97): [B, hop*(T-1)]."""
        B, T = self.mag.shape[0], self.mag.shape[1]
        lout = self.hl * (T - 1) if self.center else self.N + self.hl * (T - 1)
        out = empty((B, lout))
        # without phases `mag` is interleaved complex [B, T, ldf, 2] and the stride counts its floats
        stride = T * self.ldf * (1 if self.ph is not None else 2)
        _lib.check(self.lib.amt_istft(self.plan, ptr(self.mag), ptr(self.ph), B, T, self.ldf,
                                      stride, ptr(out), lout, stream_ptr()))
        return out

    def window_max(self):
        out = empty((self.mag.shape[0],))
        T = self.mag.shape[1]
        _lib.check(self.lib.amt_window_max(ptr(self.mag), self.mag.shape[0], T, self.ldf,
                                           T * self.ldf, ptr(out), stream_ptr()))
        return out

    # -- subtraction -----------------------------------------------------------------
    def subtract(self, guess_mag, guess_max=None, guess_index=None, guess_frames=None,
                 offset_frames=None, normalize=True, relu=True, overkill_factor=1.0, span=False, stems=None):
        """audio_complete.subtract for every window (util_audio.py:221-259).
        guess_mag [G, Tg, ldf] f32 frame-major; guess_index [B] int32 selects the
        guess per window; offset_frames [B] int32 is the already-clamped first frame
        max(_seconds_to_frames(offset) - attack_compensation, 0).
        span=True (the caller vouches that mag is non-negative and unchanged since the compress_bands(fmax=True) that
        left its per-frame maxima): amt_subtract_span touches only the frames the guess covers; same residual, same
        maxima, ~2.5 x fewer bytes.  Falls back to the whole-window kernel when the maxima are not there.
        stems: None, or a _lib.StemArgs (SongState.step builds it) -- the step also adds what it removed into the
        instrument stems of the song walk (amt_subtract_span_stems).  Only the span step has that form: ValueError
        without span / relu, RuntimeError when the per-frame maxima are not there (no fall-back to the whole window)."""
        if stems is not None and not (span and relu):
            raise ValueError('subtract: stems need the span subtraction (span=True, relu=True)')
        B, T = self.mag.shape[0], self.mag.shape[1]
        new_max = empty((B,))
        per_window = isinstance(guess_frames, torch.Tensor)         # else one frame count for every window
        a = _lib.args(_lib.SubtractArgs, resid=self.mag, resid_max=self.ref_max if normalize else None, guess=guess_mag,
                      guess_max=guess_max if normalize else None, guess_index=guess_index,
                      guess_frames=guess_frames if per_window else None,
                      guess_frames_all=0 if per_window else int(guess_mag.shape[1] if guess_frames is None else guess_frames),
                      offset_frames=offset_frames, new_max=new_max, resid_stride=T * self.ldf,
                      guess_stride=_stride0(guess_mag), B=B, T=T, ldf=self.ldf, F=self.F, normalize=int(bool(normalize)),
                      relu=int(bool(relu)), overkill_factor=float(overkill_factor))
        fm = self._fmax
        # the cached maxima describe `mag` only while it is the same tensor AND unedited since (the key holds its address
        # and torch's in-place version counter; the kernels behind this class write through raw pointers, which the counter
        # does not see -- those writers are this class's own and refresh or drop the cache themselves)
        if span and relu and fm is not None and fm[1] == (self.mag.data_ptr(), self.mag._version) and fm[0].shape == (B, T):
            if stems is not None:
                _lib.check(self.lib.amt_subtract_span_stems(C.byref(a), ptr(fm[0]), int(guess_mag.shape[1]),
                                                            C.byref(stems), stream_ptr()))
            else:
                _lib.check(self.lib.amt_subtract_span(C.byref(a), ptr(fm[0]), int(guess_mag.shape[1]), stream_ptr()))
        elif stems is not None:
            raise RuntimeError('subtract: stems need the per-frame maxima of compress_bands(fmax=True) on this '
                               'spectrogram; there is no whole-window form that keeps stems')
        else:
            self._fmax = None
            _lib.check(self.lib.amt_subtract(C.byref(a), stream_ptr()))
        self.ref_max = new_max
        return self

    # -- features -------------------------------------------------------------------
    def compress_bands(self, bands, ref=None, target_frames=None, fmax=False):
        """_resize(compress_bands(mag, bands), target)/ref -> [B, bands, target]
        (training.py:333-336).  fmax=True (identity frame map only): the kernel also leaves every frame's maximum, for
        subtract(span=True)."""
        B, T = self.mag.shape[0], self.mag.shape[1]
        target = T if target_frames is None else int(target_frames)
        edges = _dev_table(('edges', self.F, bands), lambda: band_edges(self.F, bands))
        src = None if target == T else _dev_table(('resize', T, target),
                                                  lambda: resize_source_frames(T, target))
        out = empty((B, bands, target))
        if fmax and src is None:
            fm = empty((B, T))
            _lib.check(self.lib.amt_compress_bands_fmax(
                ptr(self.mag), B, T, self.F, self.ldf, T * self.ldf, ptr(edges), bands, ptr(ref),
                None, ptr(out), target, ptr(fm), stream_ptr()))
            self._fmax = (fm, (self.mag.data_ptr(), self.mag._version))
            return out
        _lib.check(self.lib.amt_compress_bands(
            ptr(self.mag), B, T, self.F, self.ldf, T * self.ldf, ptr(edges), bands, ptr(ref),
            ptr(src), ptr(out), target, stream_ptr()))
        return out

    def short_window(self, src_frame, band_min, bands, ref=None, mode=0):
        """resize(['mag','ph']) + section_power + scaling (training.py:337-363):
        [B, bands, frames]."""
        B, T = self.mag.shape[0], self.mag.shape[1]
        frames = src_frame.shape[1]
        out = empty((B, bands, frames))
        _lib.check(self.lib.amt_short_window(
            ptr(self.mag), ptr(self.ph), B, T, self.F, self.ldf, T * self.ldf, ptr(src_frame),
            frames, ptr(band_min), bands, ptr(ref), int(mode), ptr(out), stream_ptr()))
        return out

    def note_features(self, src_frame, pitch, tone_bin, tone_lo, bands, ref=None, want=('lin', 'log10', 'phase'),
                      const_tone=60):
        """The FFT-side instrument towers of a step in one launch (amt_note_features; training.py:347-363): the band of
        `bands` bins from tone_bin[pitch - tone_lo] over the frames of src_frame, as any of 'lin' (mag / ref), 'log10'
        and 'phase'.  pitch [B] int32 device, or None: const_tone for every window.  Returns {kind: [B, bands, frames]}."""
        B, T = self.mag.shape[0], self.mag.shape[1]
        frames = src_frame.shape[1]
        if not want or any(k not in ('lin', 'log10', 'phase') for k in want):
            raise ValueError('Requested attribute does not exist')
        out = {k: empty((B, bands, frames)) for k in want}
        _lib.check(self.lib.amt_note_features(
            ptr(self.mag), ptr(self.ph) if 'phase' in out else None, B, T, self.F, self.ldf, T * self.ldf, ptr(src_frame),
            frames, ptr(pitch), int(const_tone), ptr(tone_bin), int(tone_lo), int(tone_bin.shape[0]), int(bands), ptr(ref),
            ptr(out.get('lin')), ptr(out.get('log10')), ptr(out.get('phase')), stream_ptr()))
        return out


def gather_frames(src, index, F, elem=1, band_min=0, bands=None):
    """Frame / band selection on the device (amt_gather_frames).  src: device [T, ldf] (elem 1) or
    [T, ldf, 2] (elem 2), or batched with a leading B; index: int sequence or device int32 tensor of
    source frames (-1 = zero frame), one table for all windows.  Returns [n, ldf_out(, 2)] (or batched),
    ldf_out = `bands` rounded up to 4; bins outside [0, F) and frames outside [0, T) read as zero."""
    lib = _lib.load()
    batched = src.dim() == (3 if elem == 1 else 4)
    s = src if batched else src[None]
    B, T, ldf = s.shape[0], s.shape[1], s.shape[2]
    bands = F if bands is None else int(bands)
    ldo = (bands + 3) & ~3
    idx = index if isinstance(index, torch.Tensor) else to_dev(np.asarray(index, dtype=np.int32), torch.int32)
    n = int(idx.shape[-1])
    shape = (B, n, ldo) if elem == 1 else (B, n, ldo, 2)
    out = empty(shape)
    if n:
        if T == 0:
            out.zero_()
        else:
            _lib.check(lib.amt_gather_frames(ptr(s), B, T, int(F), ldf, T * ldf * elem, elem, ptr(idx), 0, n,
                                             int(band_min), bands, ptr(out), ldo, n * ldo * elem, stream_ptr()))
    return out if batched else out[0]


def amplitude_to_db(mag, ref, F, window_max=None, amin=1e-5, top_db=80.0):
    """librosa.amplitude_to_db on the device for [B, T, ldf] magnitudes; ref / window_max: [B] tensors."""
    lib = _lib.load()
    B, T, ldf = mag.shape
    if window_max is None:
        window_max = empty((B,))
        _lib.check(lib.amt_window_max(ptr(mag), B, T, ldf, T * ldf, ptr(window_max), stream_ptr()))
    out = empty((B, T, ldf))
    _lib.check(lib.amt_amplitude_to_db(ptr(mag), B, T, int(F), ldf, T * ldf, ptr(ref), ptr(window_max),
                                       float(amin), -1.0 if top_db is None else float(top_db), ptr(out),
                                       stream_ptr()))
    return out


def db_to_amplitude(db, ref, F):
    lib = _lib.load()
    B, T, ldf = db.shape
    out = empty((B, T, ldf))
    _lib.check(lib.amt_db_to_amplitude(ptr(db), B, T, int(F), ldf, T * ldf, ptr(ref), ptr(out), stream_ptr()))
    return out


def cqt_slices(wave, src_frame, table, n_bins, hop, bin0=None, ref=None, complex_out=False):
    """slice_C for a batch (util_audio.py:411-434, build-defined CQT):
    wave [B, L] f32 device; src_frame [B, frames] int32; table = cqt_table(..., device) =
    (phase_inc, length, coef).  Returns [B, n_bins, frames]; with complex_out the pair (real, imaginary) of that
    shape, phase referred to each frame's centre (util_audio.py:428: magnitude_only=False keeps librosa's complex C)."""
    lib = _lib.load()
    B, L = wave.shape
    frames = src_frame.shape[1]
    out = empty((B, n_bins, frames))
    a = _lib.args(_lib.CqtArgs, wave=wave, src_frame=src_frame, bin0=bin0, phase_inc=table[0], length=table[1], ref=ref,
                  coef=table[2], out=out, wave_stride=_stride0(wave), B=B, L=L, hop=int(hop), frames=frames,
                  n_bins=int(n_bins), n_table=int(table[0].shape[0]))
    if complex_out:
        out_im = empty((B, n_bins, frames))
        _lib.check(lib.amt_cqt_slices_complex(C.byref(a), ptr(out_im), stream_ptr()))
        return out, out_im
    _lib.check(lib.amt_cqt_slices(C.byref(a), stream_ptr()))
    return out


_MFMA_TABLES = {}          # (phase_inc ptr, length ptr, n_bins, hop) -> (device table, the tensors it was built from)


def cqt_window_max(wave, table, hop, form='auto'):
    """max over every bin of `table` and every STFT-grid frame 0 .. L // hop of the signals' CQT: the song-level
    normalisers np.max(slice_C(0, duration, n_frames, ...)) of training.py:271-282.  wave [B, L] f32 device --
    windows, or a whole song as one row; table from cqt_table(..., device).  Returns [B].
    form: 'auto' = the MFMA form (one GEMM per window against a phasor table, amt_cqt_window_max_mfma) where its
    geometry fits -- batches of windows of at most 544 hop-blocks -- else the O(L)-per-bin VALU form
    (amt_cqt_window_max: any length, a whole song included); 'valu' / 'mfma' force one."""
    lib = _lib.load()
    B, L = wave.shape
    n_bins = int(table[0].shape[0])
    out = empty((B,))
    if form not in ('auto', 'valu', 'mfma'):
        raise ValueError('Requested attribute does not exist')
    if form != 'valu':
        key = (table[0].data_ptr(), table[1].data_ptr(), n_bins, int(hop))
        ent = _MFMA_TABLES.get(key)
        nbytes = int(lib.amt_cqt_mfma_table_bytes(int(hop), n_bins))
        if ent is None and nbytes:
            tab = empty(((nbytes + 3) // 4,), torch.int32)
            _lib.check(lib.amt_cqt_mfma_table(ptr(table[0]), ptr(table[1]), n_bins, int(hop), ptr(tab), stream_ptr()))
            ent = _MFMA_TABLES[key] = (tab, table[0], table[1])       # keeps the source tensors (and their addresses) alive
        if ent is not None:
            scratch = empty((B,))
            st = lib.amt_cqt_window_max_mfma(ptr(wave), B, L, _stride0(wave), int(hop), ptr(table[0]), ptr(table[1]),
                                             ptr(ent[0]), n_bins, ptr(out), ptr(scratch), stream_ptr())
            if st == _lib.AMT_OK:
                return out
            if st != _lib.AMT_E_UNSUPPORTED or form == 'mfma':
                _lib.check(st)
        elif form == 'mfma':
            _lib.check(_lib.AMT_E_UNSUPPORTED)
    need = int(lib.amt_cqt_window_max_workspace(L, int(hop), n_bins, B))
    ws = empty(((need + 7) // 8,), torch.float64) if need else None
    _lib.check(lib.amt_cqt_window_max(ptr(wave), B, L, _stride0(wave), int(hop), ptr(table[0]), ptr(table[1]),
                                      ptr(table[2]), n_bins, ptr(out), ptr(ws) if need else None, need,
                                      stream_ptr()))
    return out


FILTER_SCALE = 2.0     # slice_C hard-codes filter_scale=2 (util_audio.py:426)


def cqt_table(sr, fmin_hz, n_bins, bins_per_octave, device=None):
    """Per-bin oscillator increment (uint32 cycles/sample * 2^32) and filter
    length N_k = ceil(Q sr / f_k), Q = 2/(2^(1/bpo)-1)."""
    k = np.arange(n_bins, dtype=np.float64)
    freq = float(fmin_hz) * 2.0 ** (k / bins_per_octave)
    q = FILTER_SCALE / (2.0 ** (1.0 / bins_per_octave) - 1.0)
    length = np.ceil(q * sr / freq).astype(np.int32)
    inc = (np.rint(freq / sr * 2.0 ** 32).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if device is None:
        return inc, length
    # device form: (phase_inc, length, coef) -- coef = the per-bin phasor table the CQT kernels read through the
    # scalar cache (amt_cqt_coef), built once here
    inc_d, len_d = torch.from_numpy(inc.view(np.int32)).to(device), torch.from_numpy(length).to(device)
    coef = empty((int(n_bins), 192))
    _lib.check(_lib.load().amt_cqt_coef(ptr(inc_d), ptr(len_d), int(n_bins), ptr(coef), stream_ptr()))
    return (inc_d, len_d, coef)


_NOTE = {'C': 0, 'D': 2, 'E': 4, 'F': 5, 'G': 7, 'A': 9, 'B': 11}


def note_to_midi(note):
    if isinstance(note, (int, np.integer)):
        return int(note)
    name, rest, acc = note[0].upper(), note[1:], 0
    while rest and rest[0] in '#b':
        acc += 1 if rest[0] == '#' else -1
        rest = rest[1:]
    return 12 * ((int(rest) if rest else 0) + 1) + _NOTE[name] + acc


# ======================================================================================
# Reference call surface: one window
# ======================================================================================
def _to_tm(a, ldf, complex_=False):
    """numpy [F, T] -> device frame-major [T, ldf] (float) or [T, ldf, 2]."""
    a = np.asarray(a)
    Fb, T = a.shape
    if complex_:
        a = a.astype(np.complex64)
        h = np.zeros((T, ldf, 2), dtype=np.float32)
        h[:, :Fb, 0] = a.real.T
        h[:, :Fb, 1] = a.imag.T
    else:
        h = np.zeros((T, ldf), dtype=np.float32)
        h[:, :Fb] = a.T
    return to_dev(h)


def _from_tm(t, Fb, complex_=False):
    h = t.detach().cpu().numpy()
    if complex_:
        return np.ascontiguousarray((h[:, :Fb, 0] + 1j * h[:, :Fb, 1]).astype(np.complex64).T)
    return np.ascontiguousarray(h[:, :Fb].T)


SPECTRAL = ('mag', 'ph', 'D')          # attributes with a device copy; elem floats per bin: 1, 2, 1
_ELEM = {'mag': 1, 'ph': 2, 'D': 1}


class audio_complete:
    """Same constructor, properties and methods as util_audio.audio_complete (util_audio.py:32-527).

    Every spectral attribute (mag, ph, D) has two faces: a device tensor in the frame-major layout
    (``_d[name]``: [T, ldf] or [T, ldf, 2]), which all numeric work reads and writes, and a host
    array in the reference's [F, T] layout (``_h[name]``), materialised only when the caller looks
    at it or hands one in.  Window management (section / slice / concat / resize / section_power) is
    expressed as frame index maps executed by amt_gather_frames -- a column range of the
    reference's arrays is a row range here, zero padding is the index -1 -- so a window never
    travels to the host to be cut."""

    def __init__(self, waveform, n_fft, hop_length=None, center=True, sample_rate=44100):
        self._wf = waveform
        self._F = None
        self._h = {k: None for k in SPECTRAL}       # host views, [F, T]
        self._d = {k: None for k in SPECTRAL}       # device tensors, frame-major
        self._ref_mag = None
        self.sr = sample_rate
        self.N = n_fft
        self.center = center
        self.hl = hop_length if hop_length is not None else int(np.floor(n_fft / 4))
        self._fft_freq = fft_frequencies(sample_rate, n_fft)

    # ---- the two faces of a spectral attribute --------------------------------------
    @property
    def _Fb(self):
        return self.N // 2 + 1

    @property
    def _ldf(self):
        return ldf_of(self.N)

    def _has(self, name):
        return self._h[name] is not None or self._d[name] is not None

    def _dev(self, name):
        """Device tensor of a present attribute (uploads a host-set array once)."""
        if self._d[name] is None and self._h[name] is not None:
            self._d[name] = _to_tm(self._h[name], self._ldf, complex_=(name == 'ph'))
        return self._d[name]

    def _host(self, name):
        if self._h[name] is None and self._d[name] is not None:
            self._h[name] = _from_tm(self._d[name], self._Fb, complex_=(name == 'ph'))
        return self._h[name]

    def _put(self, name, host=None, dev=None):
        self._h[name], self._d[name] = host, dev

    def _frames_of(self, name):
        if self._d[name] is not None:
            return int(self._d[name].shape[0])
        return int(self._h[name].shape[1])

    # the reference's private fields, for callers (and tests) that poke them directly
    _mag = property(lambda self: self._host('mag'), lambda self, v: self._put('mag', host=v))
    _ph = property(lambda self: self._host('ph'), lambda self, v: self._put('ph', host=v))
    _D = property(lambda self: self._host('D'), lambda self, v: self._put('D', host=v))

    def _batch(self):
        return AudioBatch(None, self.N, self.hl, self.center, self.sr)

    def _scalar(self, v):
        return to_dev(np.array([v], dtype=np.float32))

    def _run_stft(self):
        wf = np.asarray(self.wf, dtype=np.float32)
        b = AudioBatch(wf[None, :], self.N, self.hl, self.center, self.sr).stft(True)
        self._put('mag', dev=b.mag[0])
        self._put('ph', dev=b.ph[0])

    def _mag_from_db(self):
        """mag = db_to_amplitude(D, ref_mag or 1) (util_audio.py:99-101,122-124,143-145), on the device."""
        if self._ref_mag is None:
            self._ref_mag = 1.0
        m = db_to_amplitude(self._dev('D')[None], self._scalar(self._ref_mag), self._Fb)[0]
        self._put('mag', dev=m)

    def clone(self):                                        # util_audio.py:69-87
        ac = audio_complete(None if self._wf is None else np.array(self._wf, copy=True),
                            sample_rate=self.sr, n_fft=self.N, center=self.center,
                            hop_length=self.hl)
        ac._F = None if self._F is None else np.array(self._F, copy=True)
        for k in SPECTRAL:
            ac._put(k, None if self._h[k] is None else np.array(self._h[k], copy=True),
                    None if self._d[k] is None else self._d[k].clone())
        ac._ref_mag = self._ref_mag
        return ac

    # ---- properties ---------------------------------------------------------------
    @property
    def wf(self):                                           # util_audio.py:88-106
        if self._wf is None:
            if self._F is not None:
                self._wf = self._istft_complex(self._F)
            elif self._has('mag') and self._has('ph'):
                self._wf = self._istft_magph()
            elif self._has('D') and self._has('ph'):
                self._mag_from_db()
                self._wf = self._istft_magph()
        return self._wf

    @wf.setter
    def wf(self, value):                                    # util_audio.py:107-114
        for k in SPECTRAL:
            self._put(k)
        self._ref_mag = None
        self._F = None
        self._wf = value

    def _istft_magph(self):
        b = self._batch()
        b.mag = self._dev('mag')[None]
        b.ph = self._dev('ph')[None]
        return b.istft()[0].cpu().numpy()

    def _istft_complex(self, Fc):
        b = self._batch()
        b.mag = _to_tm(Fc, self._ldf, True)[None]     # interleaved complex, pitch 2*ldf
        b.ph = None
        return b.istft()[0].cpu().numpy()

    @property
    def F(self):                                            # util_audio.py:116-129
        if self._F is None:
            if not (self._has('mag') and self._has('ph')):
                if self._has('D') and self._has('ph'):
                    self._mag_from_db()
                elif self.wf is not None:
                    self._run_stft()
            if self._has('mag') and self._has('ph'):
                self._F = self.mag * self.ph
        return self._F

    @F.setter
    def F(self, value):                                     # util_audio.py:130-137
        for k in SPECTRAL:
            self._put(k)
        self._ref_mag = None
        self._F = value
        self._wf = None

    def _magphase_of_F(self):
        # librosa.core.magphase of a caller-supplied F (util_audio.py:147): host numpy, off the hot path
        # (the hot path gets mag and ph straight from the STFT kernel)
        Fc = np.asarray(self._F)
        self._put('mag', host=np.abs(Fc))
        self._put('ph', host=np.exp(1.j * np.angle(Fc)).astype(Fc.dtype if np.iscomplexobj(Fc) else np.complex64))

    @property
    def mag(self):                                          # util_audio.py:139-148
        if not self._has('mag'):
            if self._has('D') and self._has('ph'):
                self._mag_from_db()
            elif self._F is not None:
                self._magphase_of_F()
            else:
                self._run_stft()
        return self._host('mag')

    @mag.setter
    def mag(self, val):                                     # util_audio.py:149-157
        self._put('D')
        self._ref_mag = None
        self._put('mag', host=val)
        if self._has('ph') and self.ph.shape != val.shape:
            self._put('ph')
        self._F = None
        self._wf = None

    @property
    def ph(self):                                           # util_audio.py:159-163
        if not self._has('ph'):
            if self._F is not None:
                self._magphase_of_F()
            else:
                self._run_stft()
        return self._host('ph')

    @ph.setter
    def ph(self, val):                                      # util_audio.py:164-168
        self._put('ph', host=val)
        self._F = None
        self._wf = None

    @property
    def ref_mag(self):                                      # util_audio.py:170-174
        if self._ref_mag is None:
            self.mag
            b = self._batch()
            b.mag = self._dev('mag')[None]
            self._ref_mag = np.float32(b.window_max()[0].item())
        return self._ref_mag

    @property
    def D(self):                                            # util_audio.py:176-180
        if not self._has('D'):
            self.mag
            m = self._dev('mag')[None]
            d = amplitude_to_db(m, self._scalar(self.ref_mag), self._Fb)      # max(D) from the window's own maximum
            self._put('D', dev=d[0])
        return self._host('D')

    @D.setter
    def D(self, val):                                       # util_audio.py:181-190
        self._put('D', host=val)
        if self._has('ph') and self.ph.shape != np.shape(val):
            self._put('ph')
        self._put('mag')
        self._F = None
        self._wf = None

    def _P(self, name):                                     # util_audio.py:192-207
        if name == 'wf':
            return self._wf
        if name == 'F':
            return self._F
        if name in SPECTRAL:
            return self._host(name)
        raise ValueError('Requested attribute does not exist')

    @property
    def shape(self):                                        # util_audio.py:209-218
        for k in SPECTRAL:
            if self._h[k] is not None:
                return tuple(self._h[k].shape)
            if self._d[k] is not None:
                return (self._Fb, int(self._d[k].shape[0]))
        return self.F.shape

    def _wf_len(self):
        """len(self.wf) without forcing the iSTFT the reference triggers here
        (util_audio.py:264): librosa.istft returns hop*(T-1) samples."""
        if self._wf is not None:
            return len(self._wf)
        T = self.shape[1]
        return self.hl * (T - 1) if self.center else self.N + self.hl * (T - 1)

    # ---- the subtraction step --------------------------------------------------
    def subtract(self, subtrahend, offset=0, attack_compensation=0,
                 normalize=True, relu=True, overkill_factor=1):
        """util_audio.py:221-259, executed by amt_subtract."""
        if isinstance(subtrahend, audio_complete):
            subtrahend.mag
            gmag = subtrahend._dev('mag')
            gmax = subtrahend.ref_mag if normalize else None
        else:
            g = np.asarray(subtrahend)
            gmag = _to_tm(g, self._ldf)
            gmax = np.float32(np.max(g)) if normalize else None
        self.mag
        T = self.shape[1]
        off = max(self._seconds_to_frames(offset) - attack_compensation, 0)
        if off > T:
            # the reference fails here with a negative np.zeros dimension (:250-257)
            raise ValueError('negative dimensions are not allowed')
        b = self._batch()
        b.mag = self._dev('mag')[None]                   # in place, as the reference's `self.mag -= ...`
        b.ref_max = self._scalar(self.ref_mag if normalize else 0.0)
        gm = self._scalar(gmax if normalize else 1.0)
        offs = to_dev(np.array([off], dtype=np.int32), torch.int32)
        b.subtract(gmag[None], gm, None, None, offs, normalize, relu, overkill_factor)
        # mag setter semantics (:149-157): dependants cleared, phase kept (same shape)
        self._put('D')
        self._put('mag', dev=b.mag[0])
        self._F = None
        self._wf = None
        self._ref_mag = None             # re-evaluated lazily, as np.max(self.mag) is in the reference

    def _seconds_to_frames(self, time):                     # util_audio.py:261-264
        return int(np.floor(time * self.shape[1] * self.sr / self._wf_len()))

    def _frames_to_seconds(self, frames):                   # util_audio.py:269-272
        return frames / self.shape[1] / self.sr * self._wf_len()

    def midi_tone_to_FFT(self, tone):                       # util_audio.py:278-284
        """Two bins below the first FFT bin above the tone, not below bin 0."""
        return tone_to_fft_bin(self._fft_freq, tone)

    # ---- window management: frame index maps on the device -------------------------------
    def _take(self, index, names=SPECTRAL, with_F=True):
        """{attribute: selected frames} for every present attribute.  index[j] = source frame of
        output frame j, -1 = a frame of zeros.  Device attributes go through amt_gather_frames."""
        index = np.asarray(index, dtype=np.int32)
        out = {}
        for k in names:
            if self._has(k):
                out[k] = gather_frames(self._dev(k), index, self._Fb, _ELEM[k])
        if with_F and self._F is not None:
            Fc = np.asarray(self._F)
            sel = np.where(index[None, :] >= 0, Fc[:, np.clip(index, 0, max(Fc.shape[1] - 1, 0))], 0) \
                if Fc.shape[1] else np.zeros((Fc.shape[0], len(index)), Fc.dtype)
            out['F'] = sel
        return out

    def _wave_span(self, first, last):
        return (int(np.floor(self._frames_to_seconds(first) * self.sr)),
                int(np.floor(self._frames_to_seconds(last) * self.sr)))

    def section(self, start, end, duration_in_frames=None):  # util_audio.py:286-328
        """A copy of [start, end) seconds (or `duration_in_frames` frames from start); frames past the
        end of the spectra are zeros."""
        first = self._seconds_to_frames(start)
        last = self._seconds_to_frames(end) if duration_in_frames is None else first + duration_in_frames
        wave = None
        if self._wf is not None:
            a, b = self._wave_span(first, last)
            wave = np.array(self._wf[a:b], copy=True)
            if len(wave) < b - a:                           # the reference pads by (b - len), not (b - a - len)
                wave = np.concatenate((wave, np.zeros(b - len(wave))))
        cut = audio_complete(wave, self.N, hop_length=self.hl, center=self.center, sample_rate=self.sr)
        cut._ref_mag = self._ref_mag
        if any(self._has(k) for k in SPECTRAL) or self._F is not None:
            T = self.shape[1]
            # columns first:last that exist, then one zero frame for every frame `last` lies past the end
            index = list(range(T))[first:last] + [-1] * max(last - T, 0)
            for k, v in self._take(index).items():
                if k == 'F':
                    cut._F = v
                else:
                    cut._put(k, dev=v)
        return cut

    def section_power(self, name, band_min, band_max):      # util_audio.py:334-349
        """Rows [band_min, band_max) of an attribute, zero rows past the last bin: [bands, T]."""
        if name in SPECTRAL and self._has(name):
            T = self._frames_of(name)
            g = gather_frames(self._dev(name), np.arange(T), self._Fb, _ELEM[name], band_min, band_max - band_min)
            return _from_tm(g, band_max - band_min, complex_=(name == 'ph'))
        P = self._P(name)                                   # 'F' / 'wf' (host arrays), or an absent attribute
        rows = np.zeros((band_max - band_min,) + P.shape[1:], dtype=P.dtype)
        got = P[band_min:band_max]
        rows[:got.shape[0]] = got
        return rows

    def slice(self, start_in_frames, end_in_frames):        # util_audio.py:351-365
        """Keep frames [start, end) in place.  A frame range of the frame-major device tensors is a
        contiguous row range: a view, nothing is copied."""
        keep = slice(start_in_frames, end_in_frames)
        if self._wf is not None:
            self._wf = self._wf[int(self._frames_to_seconds(start_in_frames) * self.sr):
                                int(self._frames_to_seconds(end_in_frames) * self.sr)]
        if self._F is not None:
            self._F = self._F[:, keep]
        for k in SPECTRAL:
            if self._d[k] is not None:
                self._put(k, None if self._h[k] is None else self._h[k][:, keep], self._d[k][keep])
            elif self._h[k] is not None:
                self._put(k, host=self._h[k][:, keep])

    def concat(self, ac):                                   # util_audio.py:374-382
        """Append another window; an attribute only one side has is dropped (None)."""
        both = lambda a, b: a is not None and b is not None
        self._wf = np.concatenate((self._wf, ac._wf), axis=0) if both(self._wf, ac._wf) else None
        self._F = np.concatenate((self._F, ac._F), axis=1) if both(self._F, ac._F) else None
        for k in SPECTRAL:
            if self._has(k) and ac._has(k):
                a, b = self._dev(k), ac._dev(k)
                joined = empty((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]))
                for part, at in ((a, 0), (b, a.shape[0])):
                    if part.shape[0]:
                        joined[at:at + part.shape[0]] = gather_frames(part, np.arange(part.shape[0]),
                                                                      self._Fb, _ELEM[k])
                self._put(k, dev=joined)
            else:
                self._put(k)

    @staticmethod
    def _resize(P, target_frame_count):                     # util_audio.py:384-409
        P = np.asarray(P)
        t = P.shape[1]
        if t == 0:
            return np.zeros((P.shape[0], target_frame_count))
        if t == target_frame_count:
            return P
        return P[:, resize_source_frames(t, target_frame_count)]

    def slice_C(self, start, duration, target_frame_count, magnitude_only=True,
                bins_per_tone=1, filter_scale=2, highest_note='C8', lowest_note='A0',
                nbins=None):
        """util_audio.py:411-434 with the build-defined CQT (oracle/cqt.py); like the reference, `filter_scale` is
        ignored (:426).  magnitude_only=False returns the complex CQT (:428 skips the np.abs), complex64, its phase
        referred to each frame's centre."""
        if nbins is None:
            nbins = int((note_to_midi(highest_note) - note_to_midi(lowest_note)) * bins_per_tone)
        fmin = float(midi_to_hz(note_to_midi(lowest_note)))
        dev = require_gpu()
        wf = to_dev(np.asarray(self.wf, dtype=np.float32))[None]
        src = self._resize_index(start, duration, target_frame_count)
        table = cqt_table(self.sr, fmin, nbins, int(12 * bins_per_tone), dev)
        out = np.zeros((nbins, target_frame_count), dtype=np.float32 if magnitude_only else np.complex64)
        for c0 in range(0, target_frame_count, 8):
            cols = src[c0:c0 + 8]
            o = cqt_slices(wf, to_dev(cols[None], torch.int32), table, nbins, self.hl, complex_out=not magnitude_only)
            if magnitude_only:
                out[:, c0:c0 + len(cols)] = o[0].cpu().numpy()
            else:
                out[:, c0:c0 + len(cols)] = o[0][0].cpu().numpy() + 1j * o[1][0].cpu().numpy()
        return out

    @staticmethod
    def compress_bands(spectrum, bands=80, log=True):       # util_audio.py:436-466
        spectrum = np.asarray(spectrum)
        Fb, T = spectrum.shape
        lib = _lib.load()
        if log:
            edges = band_edges(Fb, bands)
        else:
            r = Fb // bands
            edges = (np.arange(bands + 1) * r).astype(np.int32)
        ldf = (Fb + 3) & ~3
        d = _to_tm(spectrum, ldf)
        out = empty((1, bands, T))
        _lib.check(lib.amt_compress_bands(ptr(d), 1, T, Fb, ldf, T * ldf,
                                          ptr(to_dev(edges, torch.int32)), bands, None, None,
                                          ptr(out), T, stream_ptr()))
        return out[0].cpu().numpy().astype(np.float64)

    def _resize_index(self, start, duration, target):
        """Source frame of every column of _resize(X[:, s:t], target) (util_audio.py:384-409), -1 = zeros."""
        T = self.shape[1]
        cols = np.arange(T)[self._seconds_to_frames(start):self._seconds_to_frames(start + duration)]
        rel = resize_source_frames(len(cols), target)
        return np.where(rel < 0, -1, cols[np.clip(rel, 0, max(len(cols) - 1, 0))] if len(cols) else -1).astype(np.int32)

    def resize(self, start, duration, target_frame_count, attribs=['F']):
        """util_audio.py:469-507: a new object holding `target_frame_count` frames of the requested
        attributes, cut from [start, start + duration) by the tile / crop rule of _resize."""
        short = audio_complete(None, self.N, hop_length=self.hl, center=self.center, sample_rate=self.sr)
        if self._ref_mag is not None:
            short._ref_mag = self._ref_mag
        index = None
        for attrib in attribs:
            if attrib not in ('F', 'mag', 'ph', 'D'):
                raise ValueError('Invalid attribute requested')
            getattr(self, attrib)                           # materialise it (STFT on first use)
            if index is None:
                index = self._resize_index(start, duration, target_frame_count)
            if attrib == 'F':
                short.F = self._take(index, names=())['F']
            else:
                got = self._take(index, names=(attrib,), with_F=False)[attrib]
                # what the reference's setter does on assignment (:149-157, :164-168, :181-190)
                if attrib == 'mag':
                    short._put('D'); short._ref_mag = None
                    if short._has('ph') and short._frames_of('ph') != target_frame_count:
                        short._put('ph')
                elif attrib == 'D':
                    if short._has('ph') and short._frames_of('ph') != target_frame_count:
                        short._put('ph')
                    short._put('mag')
                short._put(attrib, dev=got)
                short._F = None
                short._wf = None
        return short

    def spectral_flatness(self):                            # util_audio.py:330-332
        """np.mean(librosa.feature.spectral_flatness(y=wf, n_fft, hop)) (power = 2, amin = 1e-10): per frame the
        geometric over the arithmetic mean of max(amin, |STFT|^2).  training.py:266 skips a song whose render
        is white noise (> 0.3)."""
        lib = _lib.load()
        self.mag
        m = self._dev('mag')[None]
        out = empty((1, m.shape[1]))
        _lib.check(lib.amt_spectral_flatness(ptr(m), 1, m.shape[1], self._Fb, self._ldf, m.shape[1] * self._ldf,
                                             1e-10, ptr(out), stream_ptr()))
        return float(np.mean(out.cpu().numpy().astype(np.float64)))

    def save(self, filename, flac=True):
        """util_audio.py:520-527: the waveform as PCM-24 FLAC, or with flac=False as a float32 WAV normalised to its
        peak -- what librosa.output.write_wav(filename, self.wf, self.sr, norm=True) writes for a float waveform."""
        if not flac:
            return save_wav(to_dev(np.asarray(self.wf, dtype=np.float32).reshape(-1)), filename, self.sr,
                            fmt='float32', norm=True)
        _flac.save_float(np.asarray(self.wf), filename, sr=self.sr, bps=24)

    def plot_spec(self, width=12, height=5, filename=None):
        """util_audio.py:509-518 without the figure window: the dB spectrogram D (ref = ref_mag, 80 dB) on a log
        frequency axis as a PNG file of 100 pixels per inch -- width x height inches, the reference's arguments --
        rendered and encoded on the device (spectrogram_png).  Returns the file's bytes; filename: also written
        there."""
        self.mag
        size = (int(round(100 * width)), int(round(100 * height)))
        data = spectrogram_png([self._dev('mag')], [float(self.ref_mag)], size=size, axis='log', sr=self.sr,
                               n_fft=self.N)[0]
        if filename is not None:
            _write_files([data], filename)
        return data


# ======================================================================================
# Sample-rate conversion (the `sr=` of librosa.load, util_audio.py:962-964)
# ======================================================================================
MAX_SIGNALS = 65535                # signals (or files) one ragged call takes: the launchers' grid limit


def _check_rates(sr_in, sr_out):
    if int(sr_in) != sr_in or int(sr_out) != sr_out or int(sr_in) <= 0 or int(sr_out) <= 0:
        raise ValueError('resample: sample rates must be positive integers. Got: %r -> %r' % (sr_in, sr_out))
    return int(sr_in), int(sr_out)


def _check_signal(s):
    """(samples, channels) of a waveform [n] or [n, channels], from its shape alone."""
    shape = tuple(s.shape) if hasattr(s, 'shape') else np.asarray(s).shape
    if len(shape) not in (1, 2):
        raise ValueError('Invalid Input shape. Expected: a waveform [n] or [n, channels] . Got: %s' % (shape,))
    n, channels = shape[0], (shape[1] if len(shape) == 2 else 1)
    if n == 0:
        raise ValueError('Invalid Input shape. Expected: at least one sample . Got: an empty signal')
    if not 1 <= channels <= Resampler.MAX_CHANNELS:
        raise ValueError('Invalid Input shape. Expected: 1 to %d channels . Got: %d' % (Resampler.MAX_CHANNELS, channels))
    return int(n), int(channels)


class Resampler:
    """Signals at sr_in -> signals at sr_out on the device (amt_resample_ragged): rational polyphase resampling with a
    Kaiser-windowed sinc (32 zero crossings per side, beta 10, rolloff 0.88), zero phase -- output n sits at time
    n / sr_out.  L / M = sr_out / sr_in reduced; `taps` = the most input samples one output uses, 2 Z R / L + 1 with
    R = max(L, M).  Channels ([n, channels], interleaved) are averaged by the kernel, as librosa.load's mono=True does.
    Every argument error is a ValueError raised before the library or the GPU is touched; the coefficient table is
    built (amt_resampler_create) at the first call."""
    Z, R_MAX, MAX_CHANNELS, MAX_SIGNALS = 32, 2048, 8, MAX_SIGNALS

    def __init__(self, sr_in, sr_out):
        self.sr_in, self.sr_out = _check_rates(sr_in, sr_out)
        if self.sr_in == self.sr_out:
            raise ValueError('Resampler: equal rates (%d): pass the signal through (audio.resample does)' % self.sr_in)
        g = math.gcd(self.sr_in, self.sr_out)
        self.L, self.M = self.sr_out // g, self.sr_in // g
        R = max(self.L, self.M)
        if R > self.R_MAX:
            raise ValueError('Resampler: %d -> %d reduces to %d / %d; the larger side may be at most %d'
                             % (self.sr_in, self.sr_out, self.L, self.M, self.R_MAX))
        self.taps = 2 * self.Z * R // self.L + 1
        self._handles = {}                                          # (device index,) -> amt_resampler *

    def out_len(self, n_in):
        """ceil(n_in L / M) (amt_resample_length)."""
        return -((-int(n_in) * self.L) // self.M)

    def _handle(self):
        def build():
            h = C.c_void_p()
            _lib.check(_lib.load().amt_resampler_create(C.byref(h), self.sr_in, self.sr_out))
            return h
        return per_device(self._handles, (), build)

    def __del__(self):
        try:
            lib = _lib.load()
            for h in self._handles.values():
                lib.amt_resampler_destroy(h)
        except Exception:                                           # interpreter shutdown: the library may be gone
            pass
        self._handles = {}

    def __call__(self, signals, out=None):
        """signals: a waveform [n], an [n, channels] array, or a list of those (one channel count per call); numpy or
        torch, host or device.  Returns one float32 1-d device tensor per input (a list for a list), views of ONE
        packed buffer -- `out` when given (a contiguous float32 device tensor of at least the summed lengths)."""
        single = not isinstance(signals, (list, tuple))
        items = [signals] if single else list(signals)
        if not items:
            raise ValueError('Invalid Input shape. Expected: at least one signal . Got: an empty list')
        if len(items) > self.MAX_SIGNALS:
            raise ValueError('Invalid Input shape. Expected: at most %d signals a call . Got: %d'
                             % (self.MAX_SIGNALS, len(items)))
        shapes = [_check_signal(s) for s in items]
        channels = shapes[0][1]
        if any(c != channels for _, c in shapes):
            raise ValueError('Invalid Input shape. Expected: one channel count per call . Got: %s'
                             % sorted({c for _, c in shapes}))
        in_len = np.asarray([n for n, _ in shapes], np.int64)
        out_len = np.asarray([self.out_len(n) for n in in_len], np.int64)
        in_base = np.concatenate([[0], np.cumsum(in_len * channels)[:-1]]).astype(np.int64)
        out_base = np.concatenate([[0], np.cumsum(out_len)[:-1]]).astype(np.int64)
        total = int(out_len.sum())
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
                                    and out.dim() == 1 and out.is_contiguous() and out.numel() >= total):
            raise ValueError('Invalid Input shape. Expected: out = a contiguous float32 device tensor of >= %d . Got: %s'
                             % (total, tuple(out.shape) if hasattr(out, 'shape') else type(out).__name__))
        lib = _lib.load()
        flat = [to_dev(s).reshape(-1) for s in items]
        buf = flat[0] if len(flat) == 1 else torch.cat(flat)
        if out is None:
            out = empty((total,))
        meta = to_dev(np.stack([in_base, in_len, out_base]), torch.int64)
        _lib.check(lib.amt_resample_ragged(self._handle(), ptr(buf), ptr(meta[0]), ptr(meta[1]), len(items), channels,
                                           buf.numel(), int(out_len.max()), ptr(out), ptr(meta[2]), out.numel(),
                                           stream_ptr()))
        views = [out[b:b + n] for b, n in zip(out_base.tolist(), out_len.tolist())]
        return views[0] if single else views


_RESAMPLERS = {}


def resample(wf, sr_in, sr_out):
    """librosa.load's sr= and mono=True (util_audio.py:962-964) for a loaded waveform [n] or [n, channels]: the float32
    1-d device tensor of it at sr_out (Resampler, cached per rate pair).  Equal rates: to_dev(wf) itself, channels
    averaged if there are any -- no filter runs."""
    sr_in, sr_out = _check_rates(sr_in, sr_out)
    if sr_in == sr_out:
        _check_signal(wf)
        w = to_dev(wf)
        return w.mean(dim=1) if w.dim() == 2 else w
    rs = _RESAMPLERS.get((sr_in, sr_out))
    if rs is None:
        rs = _RESAMPLERS[(sr_in, sr_out)] = Resampler(sr_in, sr_out)
    return rs(wf)


# ======================================================================================
# File codecs: the steps the FLAC and the WAV paths share
# ======================================================================================
def _read_files(paths):
    """(single, datas): the files at `paths` (one path or a list) read whole, and whether it was one path."""
    single = isinstance(paths, (str, bytes, os.PathLike))
    datas = []
    for p in ([paths] if single else list(paths)):
        with open(p, 'rb') as f:
            datas.append(f.read())
    return single, datas


def _write_files(files, paths):
    """files[i] written to paths[i] (one path or a list), one write per file."""
    paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
    if len(paths) != len(files):
        raise ValueError('Invalid Input shape. Expected: one path per signal (%d) . Got: %d' % (len(files), len(paths)))
    for data, path in zip(files, paths):
        with open(path, 'wb') as f:
            f.write(data)


def _check_files(datas, limit=None):
    """The argument check of both decoders: `datas` is a non-empty list of bytes, of at most `limit` files."""
    if isinstance(datas, (bytes, bytearray, memoryview)) or not isinstance(datas, (list, tuple)):
        raise ValueError('Invalid Input shape. Expected: a list of bytes . Got: %s' % type(datas).__name__)
    if not datas:
        raise ValueError('Invalid Input shape. Expected: at least one file . Got: an empty list')
    if limit is not None and len(datas) > limit:
        raise ValueError('Invalid Input shape. Expected: at most %d files a call . Got: %d' % (limit, len(datas)))
    for d in datas:
        if not isinstance(d, (bytes, bytearray)):
            raise ValueError('Invalid Input shape. Expected: a list of bytes . Got: %s in it' % type(d).__name__)


def _upload_files(datas):
    """The files' bytes back to back in one uint8 tensor on the current device: one upload."""
    return torch.frombuffer(bytearray(b''.join(datas)), dtype=torch.uint8).to(
        torch.device('cuda', torch.cuda.current_device()))


def _file_view(buf, base, frames, channels):
    """One decoded file in the packed output `buf`: [frames] for mono, else [frames, channels]."""
    v = buf[base:base + frames * channels]
    return v if channels == 1 else v.view(frames, channels)


def _ragged_layout(sigs, spans=None):
    """The input layout of amt_flac_encode_ragged, amt_pcm_peak_ragged and amt_pcm_pack_ragged: 1-d float32 signals
    that lie anywhere in one address space, named by one pointer and two tables.  Returns (anchor, base, lens):
    anchor = the lowest data_ptr of the signals that have samples, base[i] = signal i's offset from it in floats (0 for
    an empty signal, whose pointer means nothing), lens[i] = its length.  No signal has samples: anchor is None.
    amt_spec_levels_ragged and amt_png_encode_ragged take their tensors the same way: spans[i] = the elements from
    tensor i's first to its last, taken for lens; base counts in the tensor's own element size, and the extent the
    call is told is the largest base + span."""
    lens = [int(s.numel()) for s in sigs] if spans is None else list(spans)
    live = [s.data_ptr() for s, l in zip(sigs, lens) if l]
    anchor = min(live) if live else None
    base = [(s.data_ptr() - anchor) // s.element_size() if l else 0 for s, l in zip(sigs, lens)]
    return anchor, base, lens


def _fetch_split(who, out, offsets, limit):
    """The tail of flac_encode and png_encode: the int64 device offsets [n + 1] to the host, a refusal in `who`'s words if
    the last lies behind the `limit` bytes of the device buffer `out`, ONE device-to-host copy, the n pieces between."""
    off = offsets.cpu().tolist()
    if off[-1] > limit:
        raise RuntimeError('%s: the %s need %d bytes, the buffer has %d' % (who + (off[-1], limit)))
    data = out[:off[-1]].cpu().numpy().tobytes()
    return [data[a:b] for a, b in zip(off, off[1:])]


def _device_signals(waves):
    """The signal check of both encoders: the 1-d float32 device signals of `waves`, a tensor [n] or [G, n] or a list of
    those.  Rows of a 2-d tensor are taken as views; only a signal whose samples are not adjacent in memory is copied."""
    items = [waves] if isinstance(waves, torch.Tensor) else list(waves)
    sigs = []
    for w in items:
        if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.dim() in (1, 2)):
            raise ValueError('Invalid Input shape. Expected: float32 device tensors [n] or [G, n] . Got: %s'
                             % (tuple(w.shape) if hasattr(w, 'shape') else type(w).__name__,))
        for r in ([w] if w.dim() == 1 else w.unbind(0)):
            sigs.append(r if r.numel() <= 1 or r.stride(0) == 1 else r.contiguous())
    if not sigs:
        raise ValueError('Invalid Input shape. Expected: at least one signal . Got: an empty list')
    if len({s.device for s in sigs}) != 1:
        raise ValueError('Invalid Input shape. Expected: signals of one device . Got: several')
    return sigs


# ======================================================================================
# FLAC encoding on the device (the soundfile.write of audio_to_flac, util_audio.py:966-968)
# ======================================================================================
FLAC_PREDICTORS = ('fixed', 'lpc')
FLAC_LPC_MAX_ORDER = 12


def _flac_predictor(predictor, lpc_order):
    """The check of predictor / lpc_order, before any device work: the order amt_flac_encode_lpc_ragged gets, 0 for
    'fixed' (amt_flac_encode_ragged; lpc_order is then only checked)."""
    if not isinstance(predictor, str) or predictor not in FLAC_PREDICTORS:
        raise ValueError('Requested attribute does not exist: predictor %r (one of %s)' % (predictor, FLAC_PREDICTORS))
    if isinstance(lpc_order, bool) or not isinstance(lpc_order, (int, np.integer)) \
            or not 1 <= lpc_order <= FLAC_LPC_MAX_ORDER:
        raise ValueError('Invalid Input shape. Expected: lpc_order in 1 .. %d . Got: %r' % (FLAC_LPC_MAX_ORDER, lpc_order))
    return int(lpc_order) if predictor == 'lpc' else 0


def flac_encode_streams(waves, bps=24, blocksize=4096, first_frame=0, predictor='fixed', lpc_order=12):
    """amt_flac_encode_ragged for the signals of `waves` (see _device_signals), one call on the current stream: returns
    (out, stream_off, frame_minmax, md5, frame_bytes) -- out a uint8 device buffer in which signal i's frames lie back
    to back at [stream_off[i], stream_off[i + 1]); stream_off int64 [n + 1], frame_minmax int32 [n, 2], md5 uint8
    [n, 16], frame_bytes int64 [n, frames of the longest]: all device tensors, nothing is synchronised.
    predictor='lpc': amt_flac_encode_lpc_ragged, LPC subframes of order 1 .. lpc_order beside the fixed predictors
    (DESIGN 20); the buffers are the same, no frame is larger."""
    order = _flac_predictor(predictor, lpc_order)
    lib = _lib.load()
    sigs = _device_signals(waves)
    bound = int(lib.amt_flac_frame_bound(int(blocksize), int(bps)))
    if bound < 0 or int(first_frame) < 0:
        _lib.check(_lib.AMT_E_INVALID)
    n = len(sigs)
    anchor, base, lens = _ragged_layout(sigs)
    max_len = max(lens)
    frames = [-(-l // int(blocksize)) for l in lens]
    dev = sigs[0].device
    meta = torch.tensor([base, lens], dtype=torch.int64).to(dev)
    scratch = torch.empty((max(int(lib.amt_flac_scratch_bytes(n, max_len, int(blocksize), int(bps))), 8),),
                          dtype=torch.uint8, device=dev)
    out = torch.empty((max(sum(frames) * bound, 8),), dtype=torch.uint8, device=dev)
    frame_bytes = torch.empty((n, max(frames)), dtype=torch.int64, device=dev)
    stream_off = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    minmax = torch.empty((n, 2), dtype=torch.int32, device=dev)
    md5 = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    # (a host-side 8 stands where a buffer would be empty, the scratch where no signal has samples: the ABI refuses NULL)
    fb = frame_bytes if frame_bytes.numel() else torch.empty((1,), dtype=torch.int64, device=dev)
    head = (C.c_void_p(scratch.data_ptr() if anchor is None else anchor), ptr(meta[0]), ptr(meta[1]), n, max_len,
            int(blocksize), int(bps), int(first_frame))
    tail = (ptr(scratch), scratch.numel(), ptr(out), out.numel(), ptr(fb), ptr(stream_off), ptr(minmax), ptr(md5),
            stream_ptr())
    _lib.check(lib.amt_flac_encode_lpc_ragged(*head, order, *tail) if order else lib.amt_flac_encode_ragged(*head, *tail))
    # the signals and the scratch stay referenced until the call is enqueued; torch's allocator keeps a freed block
    # for the stream that used it, so work enqueued later on this stream cannot overtake the encoder
    return out, stream_off, minmax, md5, frame_bytes


def flac_stream_header(n_samples, sr, bps, blocksize, min_frame, max_frame, md5):
    """fLaC + the STREAMINFO block (the last metadata block), 42 bytes, as flac.encode writes it for a mono stream."""
    si = int(blocksize).to_bytes(2, 'big') * 2 + int(min_frame).to_bytes(3, 'big') + int(max_frame).to_bytes(3, 'big')
    si += ((int(sr) << 44) | ((int(bps) - 1) << 36) | int(n_samples)).to_bytes(8, 'big') + bytes(md5)
    return b'fLaC' + bytes([0x80]) + len(si).to_bytes(3, 'big') + si


def flac_encode(waves, sr, bps=24, blocksize=4096, predictor='fixed', lpc_order=12):
    """audio_to_flac (util_audio.py:966-968) without the file: every signal of `waves` -- a list of 1-d float32 device
    tensors; a [G, n] tensor counts as G signals, its rows are not copied -- as the bytes of a complete mono FLAC file
    (fLaC, STREAMINFO, frames).  One encode call for the whole list, on the current stream, so it is ordered after
    whatever produced the tensors; the frames come back in one device-to-host copy.  predictor='fixed' (the default)
    or 'lpc' with lpc_order in 1 .. 12: see flac_encode_streams."""
    _flac_predictor(predictor, lpc_order)
    sigs = _device_signals(waves)
    out, stream_off, minmax, md5, _ = flac_encode_streams(sigs, bps=bps, blocksize=blocksize, predictor=predictor,
                                                          lpc_order=lpc_order)
    frames = _fetch_split(('flac_encode', 'streams'), out, stream_off, out.numel())
    minmax, md5 = minmax.cpu().tolist(), md5.cpu().numpy()
    return [flac_stream_header(s.numel(), sr, bps, blocksize, minmax[i][0], minmax[i][1], md5[i].tobytes()) + frames[i]
            for i, s in enumerate(sigs)]


def save_flac(waves, paths, sr, bps=24, predictor='fixed', lpc_order=12):
    """flac_encode(waves, sr, bps, predictor=..., lpc_order=...) written to `paths`, one file per signal, one write per
    file."""
    _write_files(flac_encode(waves, sr, bps=bps, predictor=predictor, lpc_order=lpc_order), paths)


# ======================================================================================
# FLAC decoding on the device (the librosa.load of audio_from_file, util_audio.py:962-964)
# ======================================================================================
FLAC_VERIFY = {True: 2, 'crc': 1, False: 0}
# scratch a file may ask for, in samples: the real frames hold `total` (plus less than one block); the recorded libFLAC
# files carry 0.6 false candidates per frame.  16 x leaves room for false ones that declare large blocks.
FLAC_SLOT_FACTOR, FLAC_SLOT_SLACK = 16, 1 << 20
_FLAC_FRAME_ERRORS = {1: 'the stream ends inside the frame', 2: 'a reserved or impossible code',
                      3: 'a sample outside its bit range', 4: 'bits per sample above 24 are not supported',
                      5: 'a table entry out of range'}


def _flac_tables(datas, verify):
    """The host's O(frames) share of flac_decode, no GPU involved: argument checks, STREAMINFO and the candidate
    headers of every file.  Returns (infos, stream_meta int64 [n, 9], cand_meta int64 [n_cand, 7], md5 uint8 [n, 16],
    slot_ints, out_values)."""
    if not isinstance(verify, (bool, str)) or verify not in FLAC_VERIFY:
        raise ValueError("Requested attribute does not exist: verify must be True, 'crc' or False")
    _check_files(datas)                                             # (amt_flac_decode_ragged has its own limit on files)
    infos, sm, cm, md5s = [], [], [], []
    off = slot = out = 0
    for i, d in enumerate(datas):
        sr, ch, bps, total, md5, first = _flac.read_streaminfo(d)
        if bps > 24:
            raise ValueError('FLAC file %d: %d bits per sample; above 24 is not supported (float32 is exact to 24)'
                             % (i, bps))
        pos, hdr, bs, ca, fb = _flac.frame_candidates(d, first)
        fb = np.where(fb == 0, bps, fb)
        lo = sum(len(c) for c in cm)
        slots = slot + np.concatenate([[0], np.cumsum(bs.astype(np.int64) * ch)])
        cm.append(np.stack([np.full(len(pos), i, np.int64), pos, hdr.astype(np.int64), bs.astype(np.int64),
                            ca.astype(np.int64), fb.astype(np.int64), slots[:-1]], axis=1).reshape(-1, 7))
        # every candidate, false ones included, gets a slot: a file of nothing but plausible headers that declare large
        # blocks is refused here, before it asks for scratch it could never fill
        if int(slots[-1]) - slot > FLAC_SLOT_FACTOR * total * ch + FLAC_SLOT_SLACK:
            raise ValueError('FLAC file %d: its %d candidate frame headers declare %d samples for the %d of the stream '
                             '(more than %d x + %d): refused' % (i, len(pos), int(bs.astype(np.int64).sum()), total,
                                                                 FLAC_SLOT_FACTOR, FLAC_SLOT_SLACK // ch))
        slot = int(slots[-1])
        sm.append([off, len(d), first, ch, bps, total, out, lo, lo + len(pos)])
        infos.append((sr, ch, bps, total))
        md5s.append(np.frombuffer(md5, np.uint8))
        off += len(d)
        out += total * ch
    return (infos, np.asarray(sm, np.int64).reshape(-1, 9), np.concatenate(cm).astype(np.int64).reshape(-1, 7),
            np.stack(md5s), slot, out)


def flac_decode_streams(datas, verify=True, pcm=False):
    """amt_flac_decode_ragged for the files `datas` (a list of bytes), one call on the current stream, nothing
    synchronised and nothing raised for a damaged stream: returns a dict of device tensors -- out float32 [values],
    pcm int32 [values] or None, status int64 [n, 4], cand_out int64 [n_cand, 3], md5 uint8 [n, 16] -- and the host
    tables infos [(sr, channels, bps, total)], stream_meta, cand_meta (see include/amt_saga.h)."""
    infos, sm, cm, md5, slot_ints, out_values = _flac_tables(datas, verify)
    lib = _lib.load()
    n, n_cand = len(infos), len(cm)
    data = _upload_files(datas)
    dev = data.device
    tab = torch.from_numpy(np.concatenate([sm.reshape(-1), cm.reshape(-1)])).to(dev)
    sm_d, cm_d = tab[:sm.size], tab[sm.size:]
    md5_in = torch.from_numpy(md5.copy()).to(dev)
    need = int(lib.amt_flac_decode_scratch_bytes(n_cand, slot_ints))
    if need < 0:
        _lib.check(_lib.AMT_E_INVALID)
    scratch = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev)
    out = torch.empty((max(out_values, 1),), dtype=torch.float32, device=dev)
    out_i = torch.empty((max(out_values, 1),), dtype=torch.int32, device=dev) if pcm else None
    status = torch.empty((n, 4), dtype=torch.int64, device=dev)
    cand_out = torch.empty((max(n_cand, 1), 3), dtype=torch.int64, device=dev)
    md5_out = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    # (a one-element buffer stands where a table would be empty: the ABI refuses NULL)
    cm_p = cm_d if n_cand else torch.zeros((7,), dtype=torch.int64, device=dev)
    _lib.check(lib.amt_flac_decode_ragged(
        ptr(data), data.numel(), ptr(sm_d), n, ptr(cm_p), n_cand, ptr(md5_in), FLAC_VERIFY[verify], ptr(scratch),
        scratch.numel(), slot_ints, ptr(out), ptr(out_i) if pcm else None, out_values, ptr(status), ptr(cand_out),
        ptr(md5_out), stream_ptr()))
    return dict(out=out, pcm=out_i, status=status, cand_out=cand_out[:n_cand], md5=md5_out, infos=infos,
                stream_meta=sm, cand_meta=cm)


def flac_status_error(row, cand_meta=None, cand_err=None):
    """The ValueError text of one stream's status row (host integers), or None: the reader's texts where the condition
    is the reader's."""
    code, at, crc_at, md5_bad = (int(v) for v in row)
    big = (1 << 63) - 1
    if code == 5:
        return 'FLAC decode: a table entry out of range'
    if crc_at != big and (code == 0 or crc_at < at):
        return 'FLAC frame CRC-16 mismatch at byte %d' % crc_at
    if code == 1:
        return 'lost sync at byte %d' % at
    if code == 2:
        return 'lost sync at byte %d: the frame there does not decode' % at
    if md5_bad:
        return 'FLAC STREAMINFO MD5 mismatch: decoded samples differ from the encoded audio'
    return None


def flac_decode(datas, verify=True, pcm=False):
    """audio_from_file (util_audio.py:962-964) without the host reader: the files `datas` (a list of bytes) decoded on
    the device in ONE call.  Returns a list of (wave, sr, bps) -- wave a float32 device tensor pcm 2^-(bps-1), [n] for
    mono and [n, channels] otherwise, views of one buffer -- or (wave, sr, bps, pcm int32) with pcm=True.
    verify: True = CRC-16 of every frame and the STREAMINFO MD5 when the file carries one, 'crc' = CRC-16 only (the MD5
    is one sequential chain per file), False = neither.  CRC-8 is checked in every case: a header that fails it is no
    candidate.  The status of all files comes back in one small copy; a damaged file raises ValueError."""
    r = flac_decode_streams(datas, verify=verify, pcm=pcm)
    status = r['status'].cpu().tolist()
    res = []
    for i, ((sr, ch, bps, total), row, m) in enumerate(zip(r['infos'], status, r['stream_meta'].tolist())):
        msg = flac_status_error(row)
        if msg is not None:
            if row[0] == 2:                                          # which refusal: one more small copy, errors only
                at = int(row[1])
                cmeta = r['cand_meta']
                hit = np.flatnonzero((cmeta[:, 0] == i) & (cmeta[:, 1] == at))
                if len(hit):
                    e = int(r['cand_out'][int(hit[0]), 1].item())
                    msg += ' (%s)' % _FLAC_FRAME_ERRORS.get(e, 'error %d' % e)
            raise ValueError(msg + (' (file %d of the call)' % i if len(status) > 1 else ''))
        res.append((_file_view(r['out'], m[6], total, ch), sr, bps)
                   + ((_file_view(r['pcm'], m[6], total, ch),) if pcm else ()))
    return res


def load_flac(paths, verify=True, pcm=False):
    """flac_decode of the files at `paths` (one path or a list), read whole and decoded in one call."""
    single, datas = _read_files(paths)
    res = flac_decode(datas, verify=verify, pcm=pcm)
    return res[0] if single else res


# ======================================================================================
# WAV files on the device (librosa.load for a WAV file, util_audio.py:962-964; write_wav, util_audio.py:526-527)
# ======================================================================================
PCM_TILE = 1024                    # values one workgroup of the unpack / pack kernels takes at a time (AMT_PCM_TILE)
PCM_KINDS = {'int': 0, 'float': 1}
PCM_FORMATS = {'pcm16': 0, 'pcm24': 1, 'float32': 2}


def _wav_tables(datas):
    """The host's O(chunks) share of wav_decode, no GPU involved: argument checks and the header of every file.
    Returns (infos [(sr, channels, kind, bits, frames)], stream_meta int64 [n, 8], out_values).  Every file's output
    begins on a 16-byte boundary."""
    _check_files(datas, MAX_SIGNALS)
    infos, sm = [], []
    off = out = 0
    for d in datas:
        sr, ch, kind, bits, c, first, frames = _wav.read_header(d)
        sm.append([off + first, frames, ch, PCM_KINDS[kind], c, bits, out, 0])
        infos.append((sr, ch, kind, bits, frames))
        off += len(d)
        out += -(-frames * ch // 4) * 4
    return infos, np.asarray(sm, np.int64).reshape(-1, 8), out


def wav_decode(datas, pcm=False):
    """audio_from_file (util_audio.py:962-964) for WAV files without the host reader: the files `datas` (a list of
    bytes) unpacked on the device -- one upload of the concatenated bytes, one small table, ONE launch
    (amt_pcm_unpack_ragged).  Returns a list of (wave, sr, bits) -- wave a float32 device tensor by amt_saga.wav's value
    rule, [n] for mono and [n, channels] otherwise, views of one buffer -- or (wave, sr, bits, pcm int32) with pcm=True
    (integer files only: ValueError for a float file in the call).  Every refusal is a ValueError raised by the header
    walk, before the GPU is touched."""
    infos, sm, out_values = _wav_tables(datas)
    if pcm and any(kind == 'float' for _, _, kind, _, _ in infos):
        _lib.check(_lib.AMT_E_INVALID)
    lib = _lib.load()
    data = _upload_files(datas)
    dev = data.device
    sm_d = torch.from_numpy(sm).to(dev)
    out = torch.empty((out_values,), dtype=torch.float32, device=dev)
    out_i = torch.empty((out_values,), dtype=torch.int32, device=dev) if pcm else None
    _lib.check(lib.amt_pcm_unpack_ragged(ptr(data), data.numel(), ptr(sm_d), len(infos),
                                         max(f for _, _, _, _, f in infos), ptr(out), ptr(out_i) if pcm else None,
                                         out_values, stream_ptr()))
    res = []
    for (sr, ch, kind, bits, frames), row in zip(infos, sm.tolist()):
        res.append((_file_view(out, row[6], frames, ch), sr, bits)
                   + ((_file_view(out_i, row[6], frames, ch),) if pcm else ()))
    return res


def load_wav(paths, pcm=False):
    """wav_decode of the files at `paths` (one path or a list), read whole and unpacked in one call."""
    single, datas = _read_files(paths)
    res = wav_decode(datas, pcm=pcm)
    return res[0] if single else res


def load_audio(paths, verify=True):
    """The files at `paths` (one path or a list), each taken by its first four bytes: the FLAC files of the call go
    through ONE flac_decode (with `verify`), the WAV files (RIFF) through ONE wav_decode.  Returns (wave, sr, bits) per
    file in input order; a file that is neither raises flac_decode's 'not a FLAC file'."""
    single, datas = _read_files(paths)
    is_wav = [bytes(d[:4]) == b'RIFF' for d in datas]
    res = [None] * len(datas)
    for want, decode in ((False, lambda ds: flac_decode(ds, verify=verify)), (True, wav_decode)):
        idx = [i for i, w in enumerate(is_wav) if w == want]
        if idx:
            for i, r in zip(idx, decode([datas[i] for i in idx])):
                res[i] = r
    return res[0] if single else res


def wav_encode(waves, sr, fmt='pcm24', norm=False):
    """librosa.output.write_wav (util_audio.py:526-527) without the file: every signal of `waves` (the conventions of
    flac_encode: 1-d float32 device tensors, a [G, n] tensor counts as G signals) as the bytes of a complete mono WAV
    file of `fmt` ('pcm16', 'pcm24' or 'float32'), identical to amt_saga.wav.encode on the same float32 samples.
    norm=True divides every signal by its own peak first (amt_pcm_peak_ragged; write_wav's norm=True).  One pack call
    for the whole list on the current stream, one device-to-host copy."""
    if fmt not in PCM_FORMATS:
        raise ValueError('Requested attribute does not exist: fmt must be one of %s' % (_wav.FORMATS,))
    sigs = _device_signals(waves)
    if len(sigs) > MAX_SIGNALS:
        raise ValueError('Invalid Input shape. Expected: at most %d signals a call . Got: %d' % (MAX_SIGNALS, len(sigs)))
    anchor, base, lens = _ragged_layout(sigs)
    heads = [_wav.header(l, sr, fmt) for l in lens]                  # (refuses a bad rate or an oversized signal)
    lib = _lib.load()
    c = _wav.FORMAT_BYTES[fmt]
    if anchor is None:                                               # nothing to pack: every file is its header
        return heads
    out_base, total = [], 0
    for l in lens:
        out_base.append(total)
        total += -(-l * c // 4) * 4                                  # every signal's bytes begin on a word
    dev = sigs[0].device
    meta = torch.tensor([base, lens, out_base], dtype=torch.int64).to(dev)
    out = torch.empty((total,), dtype=torch.uint8, device=dev)
    peaks = None
    if norm:
        peaks = torch.empty((len(sigs),), dtype=torch.float32, device=dev)
        _lib.check(lib.amt_pcm_peak_ragged(C.c_void_p(anchor), ptr(meta[0]), ptr(meta[1]), len(sigs), max(lens),
                                           ptr(peaks), stream_ptr()))
    _lib.check(lib.amt_pcm_pack_ragged(C.c_void_p(anchor), ptr(meta[0]), ptr(meta[1]), len(sigs), max(lens),
                                       PCM_FORMATS[fmt], ptr(peaks) if norm else None, ptr(out), ptr(meta[2]), total,
                                       stream_ptr()))
    data = out.cpu().numpy().tobytes()
    return [h + data[b:b + l * c] + (b'\0' if (l * c) & 1 else b'') for h, b, l in zip(heads, out_base, lens)]


def save_wav(waves, paths, sr, fmt='pcm24', norm=False):
    """wav_encode(waves, sr, fmt, norm) written to `paths`, one file per signal, one write per file."""
    _write_files(wav_encode(waves, sr, fmt=fmt, norm=norm), paths)


# ======================================================================================
# Spectrogram images on the device (plot_spec, util_audio.py:509-518; plot_specs, util_audio.py:938-960)
# ======================================================================================
def _image_sizes(size, n):
    """[(W, H)] * n from one (W, H) or a list of n of them."""
    sizes = [tuple(size)] * n if len(size) == 2 and not hasattr(size[0], '__len__') else [tuple(s) for s in size]
    if len(sizes) != n or any(len(s) != 2 for s in sizes):
        raise ValueError('Invalid Input shape. Expected: one (W, H) or one per spectrogram (%d) . Got: %r' % (n, size))
    return [(_png._dim(w, 'W'), _png._dim(h, 'H')) for w, h in sizes]


def spectrogram_levels(mags, refs, size=(1200, 500), axis='log', sr=44100, n_fft=2048, top_db=80.0, fmin=_png.FMIN):
    """The dB picture of audio_complete.D as plot_spec draws it (util_audio.py:509-518), without a logarithm: every
    magnitude spectrogram of `mags` -- float32 device tensors [T, >= F] frame-major, F = n_fft // 2 + 1, rows of any
    stride (a region of the song pool as SongState.region_spectra returns it is taken as a view) -- becomes a uint8
    device image [H, W] of levels 0 .. 255 over top_db below its reference level: refs[i], a number or a 0-d / 1-element
    device tensor (read on the device: nothing is synchronised).  size: (W, H) for all, or one per spectrogram; axis
    'log' (from fmin to sr / 2, the reference's y_axis='log') or 'linear'; row 0 is the highest frequency.  ONE
    amt_spec_levels_ragged launch on the current stream; the images are views of one buffer.  The rule: DESIGN 26."""
    if axis not in _png.AXES:
        raise ValueError('Requested attribute does not exist: axis must be one of %s' % (_png.AXES,))
    thr = _png.thresholds(top_db)
    mags = [mags] if isinstance(mags, torch.Tensor) and mags.dim() == 2 else list(mags)
    F = int(n_fft) // 2 + 1
    for m in mags:
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float32 and m.dim() == 2
                and m.shape[0] >= 1 and m.shape[1] >= F and (m.shape[1] == 1 or m.stride(1) == 1)):
            raise ValueError('Invalid Input shape. Expected: float32 device tensors [T, >= %d] . Got: %s'
                             % (F, tuple(m.shape) if hasattr(m, 'shape') else type(m).__name__))
    n = len(mags)
    if n == 0:
        raise ValueError('Invalid Input shape. Expected: at least one spectrogram . Got: an empty list')
    if n > MAX_SIGNALS:
        raise ValueError('Invalid Input shape. Expected: at most %d spectrograms a call . Got: %d' % (MAX_SIGNALS, n))
    refs = list(refs.reshape(-1).unbind(0)) if isinstance(refs, torch.Tensor) else list(refs)
    if len(refs) != n:
        raise ValueError('Invalid Input shape. Expected: one reference level per spectrogram (%d) . Got: %d' % (n, len(refs)))
    sizes = _image_sizes(size, n)
    if len({m.device for m in mags}) != 1:
        raise ValueError('Invalid Input shape. Expected: spectrograms of one device . Got: several')
    lib, dev = _lib.load(), mags[0].device
    anchor, bases, spans = _ragged_layout(mags, [(int(m.shape[0]) - 1) * int(_stride0(m)) + F for m in mags])
    extent = max(b + l for b, l in zip(bases, spans))
    tables, at, meta, out_at = [], {}, [], 0
    for m, base, (W, H) in zip(mags, bases, sizes):
        T, ldf = int(m.shape[0]), int(_stride0(m))
        for key, build in ((('r', H), lambda: _png.axis_rows(F, H, sr, n_fft, axis, fmin)),
                           (('c', T, W), lambda: _png.axis_cols(T, W))):
            if key not in at:
                at[key] = sum(t.size for t in tables)
                tables.append(build().reshape(-1))
        meta.append([base, T, ldf, F, W, H, at[('r', H)], at[('c', T, W)], out_at, 0])
        out_at += W * H
    host = np.concatenate(tables).astype(np.int32)
    d_tab, d_meta, d_thr = to_dev(host, torch.int32), to_dev(np.asarray(meta, np.int64), torch.int64), to_dev(thr)
    if all(isinstance(r, torch.Tensor) for r in refs):
        d_ref = torch.stack([r.reshape(()).to(torch.float32) for r in refs]).to(dev)
    else:
        d_ref = to_dev(np.asarray([float(r) for r in refs], np.float32))
    out = torch.empty((out_at,), dtype=torch.uint8, device=dev)
    _lib.check(lib.amt_spec_levels_ragged(C.c_void_p(anchor), extent, ptr(d_meta), n, max(w for w, _ in sizes),
                                          max(h for _, h in sizes), ptr(d_tab), host.size, ptr(d_thr), ptr(d_ref),
                                          ptr(out), out_at, stream_ptr()))
    return [out[row[8]:row[8] + W * H].view(H, W) for row, (W, H) in zip(meta, sizes)]


def png_encode_streams(images, palette='cubehelix'):
    """amt_png_encode_ragged for `images` (see png_encode), one call on the current stream: returns (out, file_off) --
    out a uint8 device buffer in which file i lies at [file_off[i], file_off[i + 1]), file_off int64 [n + 1] on the
    device.  The call waits for the upload of its two small tables (and so for the stream's earlier work); the kernels
    are only enqueued and nothing is copied back."""
    return _png_encode(images, palette)[:2]


def png_encode(images, palette='cubehelix'):
    """matplotlib's savefig of plot_spec (util_audio.py:509-518) without the figure: every image of `images` -- uint8
    device tensors [H, W], W and H in 1 .. 16384 -- as the bytes of a complete PNG file, indexed colour with the
    256-entry `palette` ('cubehelix') or greyscale ('gray').  Filters, deflate, Adler-32 and CRC-32 run on the device
    (amt_png_encode_ragged, ONE call for the whole list on the current stream); only the finished files are copied
    back, in one copy after the sizes.  The bytes are those of the rule in DESIGN 26, whatever the batch."""
    out, file_off, bound, _ = _png_encode(images, palette)
    return _fetch_split(('png_encode', 'files'), out, file_off, bound)


def _png_encode(images, palette):
    """The checks and the one call of png_encode / png_encode_streams: (out, file_off, bytes of out, images)."""
    pal = _png.palette(palette)
    items = [images] if isinstance(images, torch.Tensor) and images.dim() == 2 else list(images)
    for im in items:
        if not (isinstance(im, torch.Tensor) and im.is_cuda and im.dtype == torch.uint8 and im.dim() == 2):
            raise ValueError('Invalid Input shape. Expected: uint8 device tensors [H, W] . Got: %s'
                             % (tuple(im.shape) if hasattr(im, 'shape') else type(im).__name__,))
    if not items:
        raise ValueError('Invalid Input shape. Expected: at least one image . Got: an empty list')
    if len(items) > MAX_SIGNALS:
        raise ValueError('Invalid Input shape. Expected: at most %d images a call . Got: %d' % (MAX_SIGNALS, len(items)))
    for im in items:
        _png._dim(int(im.shape[1]), 'W'), _png._dim(int(im.shape[0]), 'H')
    if len({im.device for im in items}) != 1:
        raise ValueError('Invalid Input shape. Expected: images of one device . Got: several')
    items = [im if im.is_contiguous() else im.contiguous() for im in items]
    lib, dev, n = _lib.load(), items[0].device, len(items)
    anchor, bases, spans = _ragged_layout(items)
    extent = max(b + l for b, l in zip(bases, spans))
    meta = (C.c_longlong * (3 * n))()
    bound = 0
    for i, im in enumerate(items):
        H, W = int(im.shape[0]), int(im.shape[1])
        meta[3 * i], meta[3 * i + 1], meta[3 * i + 2] = bases[i], W, H
        bound += int(lib.amt_png_file_bound(W, H, int(pal is not None)))
    need = int(lib.amt_png_scratch_bytes(meta, n))
    if need < 0:
        _lib.check(_lib.AMT_E_INVALID)
    scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
    out = torch.empty((bound,), dtype=torch.uint8, device=dev)
    file_off = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    d_pal = to_dev(np.ascontiguousarray(pal).reshape(-1), torch.uint8) if pal is not None else None
    _lib.check(lib.amt_png_encode_ragged(C.c_void_p(anchor), extent, meta, n, ptr(d_pal) if pal is not None else None,
                                         ptr(scratch), need, ptr(out), bound, ptr(file_off), stream_ptr()))
    # the images and the scratch stay referenced until the call is enqueued; torch's allocator keeps a freed block for
    # the stream that used it, so work enqueued later on this stream cannot overtake the encoder
    return out, file_off, bound, n


def spectrogram_png(mags, refs, size=(1200, 500), axis='log', sr=44100, n_fft=2048, top_db=80.0, palette='cubehelix'):
    """spectrogram_levels and png_encode together: one levels launch and one encode call for the whole list; returns
    one PNG file (bytes) per spectrogram."""
    _png.palette(palette)                                              # (refused before any device work)
    return png_encode(spectrogram_levels(mags, refs, size=size, axis=axis, sr=sr, n_fft=n_fft, top_db=top_db),
                      palette=palette)


def save_spectrograms(mags, paths, refs, **kw):
    """spectrogram_png(mags, refs, ...) written to `paths`, one file per spectrogram, one write per file."""
    _write_files(spectrogram_png(mags, refs, **kw), paths)


# ======================================================================================
# Harmonic/percussive separation on the device, ahead of a transcription whose heads know pitched notes only
# (drum tracks are rendered into every training song, util_audio.py:843; the gold is pitched, util_train_test.py:83)
# ======================================================================================
class HpssArgs(C.Structure):
    """amt_hpss_args of amt_hpss_ragged (include/amt_saga.h)."""
    _fields_ = [('mag', C.c_void_p), ('out_h', C.c_void_p), ('out_p', C.c_void_p), ('out_r', C.c_void_p),
                ('med_t', C.c_void_p), ('med_f', C.c_void_p), ('frame_base', C.c_void_p), ('t_frames', C.c_void_p),
                ('n', C.c_int64), ('pool_frames', C.c_int64), ('max_frames', C.c_int32), ('ldf', C.c_int32),
                ('F', C.c_int32), ('kt', C.c_int32), ('kf', C.c_int32), ('power', C.c_float), ('margin_h', C.c_float),
                ('margin_p', C.c_float)]


def hpss_args(**fields):
    """HpssArgs filled by _lib.args: a tensor gives its device pointer, None a NULL."""
    return _lib.args(HpssArgs, **fields)


HPSS_MAX_KERNEL = 63
HPSS_POWERS = (1.0, 2.0, float('inf'))
HPSS_MAX_MARGIN = 100.0


def hpss_params(kernel=(31, 31), power=2.0, margin=(1.0, 1.0)):
    """(kt, kf, power, margin_h, margin_p) of hpss / hpss_spectra, checked: kernel a pair of odd integers in 1..63,
    power 1, 2 or inf, margin a pair of numbers in [1, 100].  ValueError otherwise; no device is touched."""
    try:
        kt, kf = kernel
        ok = all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 1 <= k <= HPSS_MAX_KERNEL and k % 2 == 1
                 for k in (kt, kf))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('hpss: kernel must be a pair of odd integers in 1..%d (frames, bins) . Got: %r'
                         % (HPSS_MAX_KERNEL, kernel))
    try:
        power = float(power)
    except (TypeError, ValueError):
        power = float('nan')
    if power not in HPSS_POWERS:
        raise ValueError('hpss: power must be 1, 2 or inf . Got: %r' % (power,))
    try:
        mh, mp = (float(m) for m in margin)
    except (TypeError, ValueError):
        mh = mp = float('nan')
    if not (1.0 <= mh <= HPSS_MAX_MARGIN and 1.0 <= mp <= HPSS_MAX_MARGIN):
        raise ValueError('hpss: margin must be a pair of numbers in [1, %g] (harmonic, percussive) . Got: %r'
                         % (HPSS_MAX_MARGIN, margin))
    return int(kt), int(kf), power, mh, mp


def _hpss_launch(pool, pool_frames, ldf, dev, fbase, frames, F, params, rest=False, medians=False):
    """ONE amt_hpss_ragged launch on the current stream over the signals frames [fbase[i], + frames[i]) of the pool
    [pool_frames, ldf] at `pool` (a tensor, or a device address the caller keeps alive): (harmonic, percussive, rest or
    None, Ht or None, Pf or None), pools of the same shape; frames of no signal are left as allocated."""
    kt, kf, power, mh, mp = params
    lib = _lib.load()
    outs = [torch.empty((pool_frames, ldf), dtype=torch.float32, device=dev) if on else None
            for on in (True, True, rest, medians, medians)]
    d_fb = to_dev(np.asarray(fbase, np.int64), torch.int64, dev)
    d_tf = to_dev(np.asarray(frames, np.int32), torch.int32, dev)
    a = hpss_args(mag=pool, out_h=outs[0], out_p=outs[1], out_r=outs[2], med_t=outs[3], med_f=outs[4],
                       frame_base=d_fb, t_frames=d_tf, n=len(frames), pool_frames=pool_frames,
                       max_frames=max(frames) if len(frames) else 0, ldf=ldf, F=F, kt=kt, kf=kf,
                       power=power, margin_h=mh, margin_p=mp)
    _lib.check(lib.amt_hpss_ragged(C.byref(a), stream_ptr()))
    return outs


def hpss_spectra(mags, n_fft, kernel=(31, 31), power=2.0, margin=(1.0, 1.0), medians=False):
    """Median-filter harmonic/percussive separation (Fitzgerald 2010) of every magnitude spectrogram of `mags` -- float32
    device tensors [T, >= F] frame-major, F = n_fft // 2 + 1, taken the way spectrogram_levels takes them (views of a
    song pool included).  Returns one (harmonic, percussive) per spectrogram -- (harmonic, percussive, Ht, Pf) with
    medians=True, the two median-filtered spectrograms -- each [T, row pitch] with the columns from F on zero.
    kernel = (frames, bins), odd, 1..63; power 1, 2 or inf; margin = (harmonic, percussive) in [1, 100].  The rule:
    DESIGN 30 -- scipy's 'reflect' ends on each spectrogram's own frames and bins, exact medians, librosa's softmask
    in float32; with power = inf a tie is harmonic, where librosa.decompose.hpss gives a tie to neither side.
    ONE amt_hpss_ragged launch for the whole list, on the current stream.  Spectrograms that are views of one allocation
    (equal row pitch, a multiple of 4 floats, whole rows apart, not overlapping, spanning at most twice their own frames)
    are read where they lie and the results are views of pools of that extent; any other list is first copied into one
    packed pool."""
    params = hpss_params(kernel, power, margin)
    mags = [mags] if isinstance(mags, torch.Tensor) and mags.dim() == 2 else list(mags)
    F = int(n_fft) // 2 + 1
    for m in mags:
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float32 and m.dim() == 2
                and m.shape[1] >= F and (m.shape[1] == 1 or m.stride(1) == 1)):
            raise ValueError('Invalid Input shape. Expected: float32 device tensors [T, >= %d] . Got: %s'
                             % (F, tuple(m.shape) if hasattr(m, 'shape') else type(m).__name__))
    if not mags:
        return []
    if len({m.device for m in mags}) != 1:
        raise ValueError('Invalid Input shape. Expected: spectrograms of one device . Got: several')
    frames = [int(m.shape[0]) for m in mags]
    live = [m for m, t in zip(mags, frames) if t]
    pitches = {int(m.stride(0)) for m in live if m.shape[0] > 1}
    ldf = pitches.pop() if len(pitches) == 1 else ldf_of(n_fft)
    # one pool = one allocation: tensors of different storages may lie whole rows apart by coincidence, any distance apart
    in_place = bool(live) and not pitches and ldf >= F and ldf % 4 == 0 and \
        len({m.untyped_storage().data_ptr() for m in live}) == 1
    if in_place:
        anchor = min(m.data_ptr() for m in live)
        offs = [(m.data_ptr() - anchor) // 4 if t else 0 for m, t in zip(mags, frames)]
        in_place = all(o % ldf == 0 for o in offs)
        spans = sorted((o // ldf, o // ldf + t) for o, t in zip(offs, frames) if t)
        in_place = in_place and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        # the outputs are pools of the extent: a few regions far apart in a large pool are cheaper to copy
        in_place = in_place and spans[-1][1] <= 2 * sum(frames)
    if in_place:
        fbase = [o // ldf for o in offs]
        extent = max(b + t for b, t in zip(fbase, frames))
        pool = anchor              # rows of `ldf` floats from the lowest spectrogram on; `mags` keeps them alive
    else:
        ldf = (F + 3) // 4 * 4
        fbase = [int(b) for b in np.concatenate([[0], np.cumsum(frames)])[:-1]]
        extent = max(1, sum(frames))
        pool = torch.zeros((extent, ldf), dtype=torch.float32, device=mags[0].device)
        for m, b, t in zip(mags, fbase, frames):
            pool[b:b + t, :F].copy_(m[:, :F])
    outs = _hpss_launch(pool, extent, ldf, mags[0].device, fbase, frames, F, params, medians=medians)
    keep = [o for o in outs if o is not None]
    return [tuple(o[b:b + t] for o in keep) for b, t in zip(fbase, frames)]


def _hpss_plan(n_fft, hop):
    """The plans amt_istft_ragged accepts; ValueError otherwise, before any device work."""
    if int(n_fft) not in (1024, 2048, 4096) or int(hop) * 4 != int(n_fft):
        raise ValueError('hpss: n_fft must be 1024, 2048 or 4096 and hop n_fft / 4 . Got: n_fft=%r, hop=%r' % (n_fft, hop))
    return int(n_fft), int(hop)


def hpss(waves, n_fft=2048, hop=512, kernel=(31, 31), power=2.0, margin=(1.0, 1.0), residual=False):
    """Harmonic/percussive separation of waveforms: `waves`, a list of 1-d float32 device signals (or one), each of
    more than n_fft / 2 samples.  ONE amt_stft_mag_ragged launch for all of them, ONE amt_hpss_ragged launch on the
    magnitudes (hpss_spectra's rule and parameters), then ONE amt_istft_ragged launch per component with each signal's
    own phases.  Returns one (harmonic, percussive) per signal -- (harmonic, percussive, rest) with residual=True, the
    rest being max(S - Sh - Sp, 0), more than rounding only where a margin exceeds 1 -- each a 1-d float32 device
    tensor of hop * (len // hop) samples, like the residual of a song walk.  n_fft in 1024 / 2048 / 4096 with
    hop == n_fft / 4 (the plans of amt_istft_ragged); anything else, and a signal of <= n_fft / 2 samples, is a
    ValueError before any device work.  Everything is enqueued on the current stream; nothing is waited for."""
    params = hpss_params(kernel, power, margin)
    n_fft, hop = _hpss_plan(n_fft, hop)
    sigs = _device_signals(waves)
    if len(sigs) > MAX_SIGNALS:
        raise ValueError('Invalid Input shape. Expected: at most %d signals a call . Got: %d' % (MAX_SIGNALS, len(sigs)))
    lens = [int(s.numel()) for s in sigs]
    for L in lens:
        if L <= n_fft // 2:
            raise ValueError('Invalid Input shape. Expected: signals of more than n_fft / 2 = %d samples '
                             '(reflect padding) . Got: %d' % (n_fft // 2, L))
    lib, dev, n = _lib.load(), sigs[0].device, len(sigs)
    plan, sp = _plan(n_fft, hop, True), stream_ptr()
    F, ldf = n_fft // 2 + 1, ldf_of(n_fft)
    frames = [1 + L // hop for L in lens]
    fbase = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    pool_frames = int(fbase[-1])
    samples = torch.empty((pool_frames * hop,), dtype=torch.float32, device=dev)
    for s, b, L in zip(sigs, fbase, lens):
        samples[int(b) * hop:int(b) * hop + L].copy_(s)
    mag = torch.empty((pool_frames, ldf), dtype=torch.float32, device=dev)
    ph = torch.empty((pool_frames, ldf, 2), dtype=torch.float32, device=dev)
    d_fb, d_sb = to_dev(fbase[:-1].copy(), torch.int64, dev), to_dev(fbase[:-1] * hop, torch.int64, dev)
    d_len, d_tf = to_dev(np.asarray(lens, np.int32), torch.int32, dev), to_dev(np.asarray(frames, np.int32), torch.int32, dev)
    _lib.check(lib.amt_stft_mag_ragged(plan, ptr(samples), ptr(d_sb), ptr(d_len), n, max(lens), samples.numel(), sum(lens),
                                       ptr(mag), ptr(ph), None, ptr(d_fb), pool_frames, ldf, sp))
    parts = [o for o in _hpss_launch(mag, pool_frames, ldf, dev, fbase[:-1].tolist(), frames, F, params, rest=residual)[:3] if o is not None]
    out_lens = [hop * (t - 1) for t in frames]
    obase = np.concatenate([[0], np.cumsum(out_lens)]).astype(np.int64)
    d_ob = to_dev(obase[:-1].copy(), torch.int64, dev)
    out = torch.empty((len(parts), int(obase[-1])), dtype=torch.float32, device=dev)
    for g, part in enumerate(parts):
        _lib.check(lib.amt_istft_ragged(plan, ptr(part), ptr(ph), ptr(d_fb), ptr(d_tf), n, max(frames), pool_frames, ldf,
                                        ptr(out[g]), ptr(d_ob), int(obase[-1]), sp))
    return [tuple(out[g, int(a):int(a) + m] for g in range(len(parts))) for a, m in zip(obase[:-1], out_lens)]


def save_hpss(waves, paths, sr, format='flac', **kw):
    """hpss(waves, **kw) written out: paths[i] = (harmonic path, percussive path) of signal i, 24-bit FLAC through
    save_flac or PCM-24 WAV through save_wav (format='wav'), all files in one encode call."""
    if format not in ('flac', 'wav'):
        raise ValueError('Requested attribute does not exist')
    paths = [tuple(p) for p in paths]
    n = 1 if isinstance(waves, torch.Tensor) and waves.dim() == 1 else len(waves)
    if len(paths) != n or any(len(p) != 2 for p in paths):
        raise ValueError('Invalid Input shape. Expected: one (harmonic, percussive) pair of paths per signal (%d) . Got: %d'
                         % (n, len(paths)))
    parts = hpss(waves, **kw)
    flat, names = [w for pair in parts for w in pair[:2]], [p for pair in paths for p in pair]
    (save_wav(flat, names, sr, fmt='pcm24') if format == 'wav' else save_flac(flat, names, sr))
