"""Beat tracking on the device: onset envelopes and dynamic-programming beat tracks (Ellis 2007, the form of
librosa.beat.beat_track) of any number of songs of unequal lengths, for the tempo map events.write_midi puts into the
MIDI it writes.  The reference stops at fixed-tempo note_sequence files (util_audio.py:594-639).  The rule lives in
csrc/amt_beat_core.h and is restated in tests/beat_reference.py: one float32 step per cell, integers from
there on, so a result is equal or wrong.  The two tables of the rule (the tempo prior and the transition penalties) are
built here, on the host, once per parameter set; the device never takes a logarithm.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .audio import MAX_SIGNALS, _device_signals, _plan, ldf_of
from .device import per_device, ptr, stream_ptr, to_dev

MAX_BINS = 2049
MAX_FRAMES = (1 << 20) - 1
MAX_LAG = 1024
MAX_TIGHTNESS = 10000.0        # pen <= tightness 1024 ln(2)^2 stays far inside int32
PRIOR_MAX = 32767


class EnvArgs(C.Structure):
    """amt_beat_env_args of amt_beat_envelope (include/amt_saga.h)."""
    _fields_ = [('mag', C.c_void_p), ('ref', C.c_void_p), ('frame_base', C.c_void_p), ('t_frames', C.c_void_p),
                ('env', C.c_void_p), ('flux', C.c_void_p), ('scratch', C.c_void_p), ('scratch_bytes', C.c_int64),
                ('n', C.c_int64), ('pool_frames', C.c_int64), ('max_frames', C.c_int32), ('ldf', C.c_int32),
                ('F', C.c_int32), ('w', C.c_int32)]


class TrackArgs(C.Structure):
    """amt_beat_track_args of amt_beat_track (include/amt_saga.h)."""
    _fields_ = [('env', C.c_void_p), ('frame_base', C.c_void_p), ('t_frames', C.c_void_p), ('prior', C.c_void_p),
                ('pen', C.c_void_p), ('beat_base', C.c_void_p), ('period', C.c_void_p), ('count', C.c_void_p),
                ('beats', C.c_void_p), ('C', C.c_void_p), ('back', C.c_void_p), ('scratch', C.c_void_p),
                ('scratch_bytes', C.c_int64), ('n', C.c_int64), ('pool_frames', C.c_int64), ('beats_total', C.c_int64),
                ('max_frames', C.c_int32), ('lag_lo', C.c_int32), ('lag_hi', C.c_int32)]


def env_args(**fields):
    """EnvArgs filled by _lib.args: a tensor gives its device pointer, None a NULL."""
    return _lib.args(EnvArgs, **fields)


def track_args(**fields):
    """TrackArgs filled by _lib.args."""
    return _lib.args(TrackArgs, **fields)


class Params(tuple):
    """(lag_lo, lag_hi, w, prior, pen) of a parameter set, with the frame rate it was made for as `.fps`: prior int32
    [lag_hi - lag_lo + 1], pen int32 [lag_hi - lag_lo + 1, 2 lag_hi + 1] (row P - lag_lo, entry tau), both numpy."""
    fps = None


_PARAMS = {}
_DEV_TABLES = {}


def _number(v):
    try:
        return float(v)
    except (TypeError, ValueError):
        return float('nan')


def lag_tables(lag_lo, lag_hi, fps, tightness=100, centre=120.0, octaves=1.0):
    """(prior, pen) over the lags lag_lo..lag_hi at `fps` frames a second: prior[L - lag_lo] = round(32767 exp(-z^2 / 2)),
    z = log2(tempo of L / centre) / octaves; pen[P - lag_lo][tau] = round(tightness 1024 ln(tau / P)^2) for
    ceil(P / 2) <= tau <= 2 P (256 for the envelope's unit of 1/256 rms, times 4 because the local score sums to 4 e)."""
    if not (isinstance(lag_lo, (int, np.integer)) and isinstance(lag_hi, (int, np.integer)) and 1 <= lag_lo <= lag_hi <= MAX_LAG):
        raise ValueError('beat: lags must be integers with 1 <= lag_lo <= lag_hi <= %d . Got: %r' % (MAX_LAG, (lag_lo, lag_hi)))
    tightness, centre, octaves, fps = _number(tightness), _number(centre), _number(octaves), _number(fps)
    if not 0.0 < tightness <= MAX_TIGHTNESS:
        raise ValueError('beat: tightness must be a number in (0, %g] . Got: %r' % (MAX_TIGHTNESS, tightness))
    if not (0.0 < centre < float('inf') and 0.0 < octaves < float('inf') and 0.0 < fps < float('inf')):
        raise ValueError('beat: centre, octaves and the frame rate must be positive numbers . Got: %r'
                         % ((centre, octaves, fps),))
    lags = np.arange(lag_lo, lag_hi + 1, dtype=np.float64)
    z = np.log2(60.0 * fps / lags / centre) / octaves
    prior = np.rint(PRIOR_MAX * np.exp(-0.5 * z * z)).astype(np.int32)
    pen = np.zeros((lag_hi - lag_lo + 1, 2 * lag_hi + 1), np.int32)
    for P in range(int(lag_lo), int(lag_hi) + 1):
        tau = np.arange((P + 1) // 2, 2 * P + 1, dtype=np.float64)
        pen[P - lag_lo, (P + 1) // 2:2 * P + 1] = np.rint(tightness * 1024.0 * np.log(tau / P) ** 2).astype(np.int32)
    return prior, pen


def params(sr, hop, bpm=(40, 240), tightness=100, mean_s=0.5, centre=120.0, octaves=1.0):
    """The checked parameter set of a track at sample rate sr and hop: Params (lag_lo, lag_hi, w, prior, pen) --
    lag_lo = floor(60 fps / bpm[1]) (at least 1), lag_hi = ceil(60 fps / bpm[0]), w = round(mean_s fps) frames, the half
    width of the envelope's local mean; the tables as lag_tables makes them.  Cached per argument set.  ValueError for
    anything else, before any device work."""
    try:
        lo, hi = (_number(b) for b in bpm)
    except (TypeError, ValueError):
        lo = hi = float('nan')
    key = (_number(sr), _number(hop), lo, hi, _number(tightness), _number(mean_s), _number(centre), _number(octaves))
    if key in _PARAMS:
        return _PARAMS[key]
    sr_, hop_, _, _, _, mean_, _, _ = key
    if not (0.0 < sr_ < float('inf') and 0.0 < hop_ < float('inf') and hop_ == int(hop_)):
        raise ValueError('beat: sr must be a positive number and hop a positive integer . Got: sr=%r, hop=%r' % (sr, hop))
    if not 0.0 < lo <= hi < float('inf'):
        raise ValueError('beat: bpm must be a pair of numbers with 0 < slowest <= fastest . Got: %r' % (bpm,))
    if not 0.0 <= mean_ < float('inf'):
        raise ValueError('beat: mean_s must be a number >= 0 . Got: %r' % (mean_s,))
    fps = sr_ / hop_
    lag_lo, lag_hi = max(1, int(math.floor(60.0 * fps / hi))), int(math.ceil(60.0 * fps / lo))
    if lag_hi > MAX_LAG:
        raise ValueError('beat: the slowest tempo must span at most %d frames . Got: bpm=%r at %g frames a second (%d)'
                         % (MAX_LAG, bpm, fps, lag_hi))
    w = int(round(mean_ * fps))
    if w > 2 ** 31 - 1:
        raise ValueError('beat: mean_s must be a number >= 0 . Got: %r' % (mean_s,))
    prior, pen = lag_tables(lag_lo, lag_hi, fps, tightness, centre, octaves)
    p = Params((lag_lo, lag_hi, w, prior, pen))
    p.fps = fps
    _PARAMS[key] = p
    return p


def params_for_lags(lag_lo, lag_hi, fps, w=0, tightness=100, centre=120.0, octaves=1.0):
    """A Params over an explicit lag range (frames) at `fps` frames a second, for callers that do not think in bpm."""
    if not (isinstance(w, (int, np.integer)) and not isinstance(w, bool) and 0 <= w <= 2 ** 31 - 1):
        raise ValueError('beat: w must be an integer >= 0 . Got: %r' % (w,))
    prior, pen = lag_tables(lag_lo, lag_hi, fps, tightness, centre, octaves)
    p = Params((int(lag_lo), int(lag_hi), int(w), prior, pen))
    p.fps = float(fps)
    return p


def _tables_on_device(p, dev):
    """prior and pen of a Params on the device, once per device and table pair."""
    with torch.cuda.device(dev):
        return per_device(_DEV_TABLES, (id(p[3]), id(p[4])),
                          lambda: (to_dev(p[3], torch.int32, dev), to_dev(np.ascontiguousarray(p[4]), torch.int32, dev), p))


def _scratch(n, pool_frames, lag_hi, beats_total, dev):
    need = _lib.load().amt_beat_scratch_bytes(n, pool_frames, lag_hi, beats_total)
    if need < 0:
        _lib.check(int(need))
    return torch.empty((max(int(need), 16),), dtype=torch.uint8, device=dev), int(need)


def _bases(frames):
    return [int(b) for b in np.concatenate([[0], np.cumsum(frames)])[:-1]]


def _check_frames(frames):
    if len(frames) > MAX_SIGNALS:
        raise ValueError('Invalid Input shape. Expected: at most %d songs a call . Got: %d' % (MAX_SIGNALS, len(frames)))
    if frames and max(frames) > MAX_FRAMES:
        raise ValueError('Invalid Input shape. Expected: songs of at most %d frames . Got: %d' % (MAX_FRAMES, max(frames)))


def _envelope_launch(pool, pool_frames, ldf, dev, fbase, frames, F, refs, w, flux=False):
    """ONE amt_beat_envelope call on the current stream over the songs frames [fbase[i], + frames[i]) of the pool
    [pool_frames, ldf] at `pool` (a tensor or a device address the caller keeps alive): (e uint16 [pool_frames], flux
    int32 [pool_frames] or None)."""
    lib = _lib.load()
    env = torch.zeros((pool_frames,), dtype=torch.int16, device=dev).view(torch.uint16)
    d_flux = torch.zeros((pool_frames,), dtype=torch.int32, device=dev) if flux else None
    scratch, need = _scratch(len(frames), pool_frames, 0, 0, dev)
    a = env_args(mag=pool, ref=refs, frame_base=to_dev(np.asarray(fbase, np.int64), torch.int64, dev),
                 t_frames=to_dev(np.asarray(frames, np.int32), torch.int32, dev), env=env, flux=d_flux, scratch=scratch,
                 scratch_bytes=need, n=len(frames), pool_frames=pool_frames, max_frames=max(frames) if frames else 0,
                 ldf=ldf, F=F, w=min(int(w), 2 ** 31 - 1))
    _lib.check(lib.amt_beat_envelope(C.byref(a), stream_ptr()))
    return env, d_flux


def onset_envelopes(mags, refs=None, w=43, n_bins=None, flux=False):
    """The onset envelope of every magnitude spectrogram of `mags` -- float32 device tensors [T, >= F] frame-major, taken
    the way audio.hpss_spectra takes them (views of a song pool included); F = n_bins, or the narrowest tensor's width.
    refs: each song's maximum magnitude, a float32 device tensor [n] or a sequence of numbers; None takes the maxima of
    the live bins on the device.  w: half-width of the local mean in frames (params(...)[2]).  Returns one uint16 device
    tensor [T] per spectrogram, in 1/256 of the rms of the flux's excess over its local mean -- (e, flux int32 [T]) pairs
    with flux=True.  ONE amt_beat_envelope call for the whole list, on the current stream; spectrograms that are views of
    one allocation are read where they lie, any other list is first copied into one packed pool."""
    mags = [mags] if isinstance(mags, torch.Tensor) and mags.dim() == 2 else list(mags)
    if not (isinstance(w, (int, np.integer)) and not isinstance(w, bool) and w >= 0):
        raise ValueError('beat: w must be an integer >= 0 . Got: %r' % (w,))
    for m in mags:
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float32 and m.dim() == 2
                and m.shape[1] >= 1 and (m.shape[1] == 1 or m.stride(1) == 1)):
            raise ValueError('Invalid Input shape. Expected: float32 device tensors [T, >= F] . Got: %s'
                             % (tuple(m.shape) if hasattr(m, 'shape') else type(m).__name__,))
    if not mags:
        return []
    F = int(n_bins) if n_bins is not None else min(int(m.shape[1]) for m in mags)
    if not (1 <= F <= MAX_BINS and all(m.shape[1] >= F for m in mags)):
        raise ValueError('Invalid Input shape. Expected: 1 <= F <= %d bins in every spectrogram . Got: %d' % (MAX_BINS, F))
    if len({m.device for m in mags}) != 1:
        raise ValueError('Invalid Input shape. Expected: spectrograms of one device . Got: several')
    frames = [int(m.shape[0]) for m in mags]
    _check_frames(frames)
    dev, n = mags[0].device, len(mags)
    if refs is not None and not isinstance(refs, torch.Tensor):
        refs = np.asarray(refs, np.float32).reshape(-1)
    if refs is not None and (refs.numel() if isinstance(refs, torch.Tensor) else refs.size) != n:
        raise ValueError('Invalid Input shape. Expected: one ref per spectrogram (%d) . Got: %d'
                         % (n, refs.numel() if isinstance(refs, torch.Tensor) else refs.size))
    if isinstance(refs, torch.Tensor) and not (refs.is_cuda and refs.dtype == torch.float32):
        raise ValueError('Invalid Input shape. Expected: refs as a float32 device tensor . Got: %s on %s' % (refs.dtype, refs.device))
    live = [m for m, t in zip(mags, frames) if t]
    pitches = {int(m.stride(0)) for m in live if m.shape[0] > 1}
    ldf = pitches.pop() if len(pitches) == 1 else 0
    in_place = bool(live) and not pitches and ldf >= F and \
        len({m.untyped_storage().data_ptr() for m in live}) == 1
    if in_place:
        anchor = min(m.data_ptr() for m in live)
        offs = [(m.data_ptr() - anchor) // 4 if t else 0 for m, t in zip(mags, frames)]
        spans = sorted((o // ldf, o // ldf + t) for o, t in zip(offs, frames) if t)
        in_place = all(o % ldf == 0 for o in offs) and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    if in_place:
        fbase = [o // ldf for o in offs]
        extent = max(b + t for b, t in zip(fbase, frames))
        pool = anchor                  # rows of `ldf` floats from the lowest spectrogram on; `mags` keeps them alive
    if not in_place:
        ldf = (F + 3) // 4 * 4
        fbase = _bases(frames)
        extent = max(1, sum(frames))
        pool = torch.zeros((extent, ldf), dtype=torch.float32, device=dev)
        for m, b, t in zip(mags, fbase, frames):
            pool[b:b + t, :F].copy_(m[:, :F])
    if refs is None:
        refs = torch.stack([m[:, :F].amax() if t else m.new_zeros(()) for m, t in zip(mags, frames)])
    elif not isinstance(refs, torch.Tensor):
        refs = to_dev(refs, torch.float32, dev)
    env, d_flux = _envelope_launch(pool, extent, ldf, dev, fbase, frames, F, refs.contiguous(), w, flux=flux)
    if flux:
        return [(env[b:b + t], d_flux[b:b + t]) for b, t in zip(fbase, frames)]
    return [env[b:b + t] for b, t in zip(fbase, frames)]


def _track_launch(env, pool_frames, dev, fbase, frames, p, debug=False):
    """ONE amt_beat_track call on the current stream: (out int32 [2 n + beats_total] = periods, counts, beats; the beat
    bases; C int64 and back int32 [pool_frames] or None)."""
    lib = _lib.load()
    lag_lo, lag_hi = int(p[0]), int(p[1])
    step = (lag_lo + 1) // 2
    bounds = [t // step + 1 for t in frames]
    bbase = _bases(bounds)
    total, n = sum(bounds), len(frames)
    prior, pen, _ = _tables_on_device(p, dev)
    out = torch.zeros((2 * n + total,), dtype=torch.int32, device=dev)
    d_C = torch.zeros((pool_frames,), dtype=torch.int64, device=dev) if debug else None
    d_back = torch.full((pool_frames,), -1, dtype=torch.int32, device=dev) if debug else None
    scratch, need = _scratch(n, pool_frames, lag_hi, total, dev)
    a = track_args(env=env, frame_base=to_dev(np.asarray(fbase, np.int64), torch.int64, dev),
                   t_frames=to_dev(np.asarray(frames, np.int32), torch.int32, dev), prior=prior, pen=pen,
                   beat_base=to_dev(np.asarray(bbase, np.int64), torch.int64, dev), period=out[:n], count=out[n:2 * n],
                   beats=out[2 * n:] if total else out, C=d_C, back=d_back, scratch=scratch, scratch_bytes=need, n=n,
                   pool_frames=pool_frames, beats_total=total, max_frames=max(frames) if frames else 0, lag_lo=lag_lo,
                   lag_hi=lag_hi)
    _lib.check(lib.amt_beat_track(C.byref(a), stream_ptr()))
    return out, bbase, d_C, d_back


def _results(out, bbase, n, hop, sr):
    """The one copy back: per song dict(period, frames, beats, tempo), a beat at frame * hop / sr seconds."""
    host = out.cpu().numpy()
    res = []
    for i in range(n):
        period, count = int(host[i]), int(host[n + i])
        frames = [int(b) for b in host[2 * n + bbase[i]:2 * n + bbase[i] + count]]
        beats = [f * hop / sr for f in frames]
        gaps = np.diff(beats)
        res.append(dict(period=period, frames=frames, beats=beats,
                        tempo=float(60.0 / np.median(gaps)) if len(beats) >= 2 else None))
    return res


def _as_params(p, sr, hop, kw):
    if isinstance(p, Params):
        if kw:
            raise ValueError('beat: params given together with %s' % ', '.join(sorted(kw)))
        return p
    if p is not None:
        raise ValueError('beat: params must come from beat.params(...) . Got: %s' % type(p).__name__)
    try:
        return params(sr, hop, **kw)
    except TypeError:
        raise ValueError('Requested attribute does not exist')


def track(envelopes, sr=44100, hop=512, params=None, debug=False, **kw):
    """Period and beats of every envelope of `envelopes` -- uint16 device tensors [T] (onset_envelopes' results, views of
    one tensor included), or one.  Parameters: a Params from beat.params(...), or its keyword arguments with sr and hop.
    Returns per song dict(period (frames, 0: no beats), frames (beat frames, ascending), beats (seconds, frame hop / sr),
    tempo (60 / median inter-beat interval, None below two beats)); with debug=True also C (int64 [T]) and back (int32
    [T]), device tensors.  ONE amt_beat_track call and ONE copy back for the whole list."""
    p = _as_params(params, sr, hop, kw)
    envs = [envelopes] if isinstance(envelopes, torch.Tensor) and envelopes.dim() == 1 else list(envelopes)
    for e in envs:
        if not (isinstance(e, torch.Tensor) and e.is_cuda and e.dtype == torch.uint16 and e.dim() == 1):
            raise ValueError('Invalid Input shape. Expected: uint16 device tensors [T] . Got: %s'
                             % ('%s %s' % (e.dtype, tuple(e.shape)) if hasattr(e, 'shape') else type(e).__name__,))
    if not envs:
        return []
    if len({e.device for e in envs}) != 1:
        raise ValueError('Invalid Input shape. Expected: envelopes of one device . Got: several')
    frames = [int(e.numel()) for e in envs]
    _check_frames(frames)
    dev = envs[0].device
    fbase = _bases(frames)
    pool = torch.zeros((max(1, sum(frames)),), dtype=torch.int16, device=dev).view(torch.uint16)
    for e, b, t in zip(envs, fbase, frames):
        pool[b:b + t].copy_(e)
    out, bbase, d_C, d_back = _track_launch(pool, pool.numel(), dev, fbase, frames, p, debug=debug)
    res = _results(out, bbase, len(envs), hop, sr)
    if debug:
        for r, b, t in zip(res, fbase, frames):
            r['C'], r['back'] = d_C[b:b + t], d_back[b:b + t]
    return res


def beat_track(waves, sr, n_fft=2048, hop=512, params=None, keep=None, **kw):
    """Beats of waveforms: `waves`, a list of 1-d float32 device signals (or one), each of more than n_fft / 2 samples.
    ONE amt_stft_mag_ragged launch for all of them (magnitudes and maxima only, no phases), ONE amt_beat_envelope and ONE
    amt_beat_track call on the pool, one copy back.  Returns per song dict(period, tempo, beats, frames): beats in
    seconds as frame hop / sr, tempo = 60 / median inter-beat interval or None below two beats.  Parameters as track's.
    keep: a dict that is filled with the call's device arrays -- 'mag' [pool_frames, row pitch], 'refs' [n], 'env'
    [pool_frames], and the host lists 'frame_base' and 'frames' -- for a caller that wants to look at them.
    Bad arguments are a ValueError before any device work."""
    p = _as_params(params, sr, hop, kw)
    n_fft, hop = int(n_fft), int(hop)
    if n_fft // 2 + 1 > MAX_BINS or n_fft < 2:
        raise ValueError('beat: n_fft must be at most %d . Got: %r' % (2 * (MAX_BINS - 1), n_fft))
    sigs = _device_signals(waves)
    lens = [int(s.numel()) for s in sigs]
    for L in lens:
        if L <= n_fft // 2:
            raise ValueError('Invalid Input shape. Expected: signals of more than n_fft / 2 = %d samples '
                             '(reflect padding) . Got: %d' % (n_fft // 2, L))
    frames = [1 + L // hop for L in lens]
    _check_frames(frames)
    lib, dev, n = _lib.load(), sigs[0].device, len(sigs)
    plan, sp = _plan(n_fft, hop, True), stream_ptr()
    F, ldf = n_fft // 2 + 1, ldf_of(n_fft)
    fbase = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    pool_frames = int(fbase[-1])
    samples = torch.empty((pool_frames * hop,), dtype=torch.float32, device=dev)
    for s, b, L in zip(sigs, fbase, lens):
        samples[int(b) * hop:int(b) * hop + L].copy_(s)
    mag = torch.empty((pool_frames, ldf), dtype=torch.float32, device=dev)
    refs = torch.empty((n,), dtype=torch.float32, device=dev)
    d_fb, d_sb = to_dev(fbase[:-1].copy(), torch.int64, dev), to_dev(fbase[:-1] * hop, torch.int64, dev)
    d_len = to_dev(np.asarray(lens, np.int32), torch.int32, dev)
    _lib.check(lib.amt_stft_mag_ragged(plan, ptr(samples), ptr(d_sb), ptr(d_len), n, max(lens), samples.numel(), sum(lens),
                                       ptr(mag), None, ptr(refs), ptr(d_fb), pool_frames, ldf, sp))
    bases = [int(b) for b in fbase[:-1]]
    env, _ = _envelope_launch(mag, pool_frames, ldf, dev, bases, frames, F, refs, p[2])
    out, bbase, _, _ = _track_launch(env, pool_frames, dev, bases, frames, p)
    if keep is not None:
        keep.update(mag=mag, refs=refs, env=env, frame_base=bases, frames=frames)
    return _results(out, bbase, n, hop, sr)
