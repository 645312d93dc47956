"""Song-level driver over the batched loop: waveform (or FLAC) -> windows -> note events -> MIDI.

The reference only has this in its *training* form (training.py:296-449: 6-s windows advanced
by half a window, one note detected and subtracted per step, the gold note sequence standing
where predictions would).  This module composes the pieces the hot path and the widened rows
provide for the inference direction:

    flac.load_float / audio_from_file      util_audio.py:650-700 (file I/O)
    windows of p.timing_frames frames, hop = half a window        training.py:317-328
    TranscriptionLoop.run (all windows of the song in one batch)  the hot path
    TranscriptionLoop.run_songs (traversal='song': ONE window sliding over the song's spectrogram)   training.py:284-328
    events.events_to_notes -> merge_overlap_duplicates -> write_midi   util_audio.py:594-639, 790-792

    python -m amt_saga.transcribe in.flac out.mid [--weights DIR] [--iters 5]
    python -m amt_saga.transcribe --songs a.flac b.flac ... --out-dir DIR [--slots N]     (song queue, one .mid per input)
    --sr RATE (both modes): the model runs at RATE and every file is resampled to it from its own rate on the device
    (audio.resample, the `sr=` of librosa.load, util_audio.py:962-964); without it the model is built at the file's rate.
    --residual OUT.flac (with --traversal song) / --residual-dir DIR (with --songs): what the walk left of the song after
    every subtraction, as 24-bit FLAC at the model's rate (the reference's _after_subtr.flac, training.py:438-447).
    --stems-dir DIR (with --traversal song, or with --songs): what the walk took out of the song, one file per instrument
    group, <input stem>.group<g>.flac (the reference's _guessed.flac, training.py:426-447, at song length).
    --flac {host,device}: the writer of those files -- host (default): amt_saga.flac's VERBATIM writer; device: the HIP
    encoder (audio.save_flac), a song's residual and stems in one call, compressed.
    --flac-predictor {fixed,lpc}: the predictors of --flac device -- fixed (default): orders 0..4; lpc: linear prediction
    of order 1..12 beside them.  Refused with --flac host.
    --decode {host,device}: the reader of the input files -- host (default): amt_saga.flac's reader; device: the HIP
    decoder (audio.load_audio), --slots files per decode call with --songs, the samples never on the host.
    A file that begins with RIFF is read as WAV, by amt_saga.wav's reader (host) or by audio.load_audio (device: the FLAC
    and the WAV files of a group in one decode call each); every other file is read as FLAC.
    --format {flac,wav} (both modes): the container of --residual / --residual-dir / --stems-dir -- flac (default), or
    wav: PCM-24 WAV through audio.save_wav, a song's residual and stems in one call, named .residual.wav / .group<g>.wav.
    --spectrogram-dir DIR (with --traversal song, or with --songs) [--spectrogram-size WxH, default 1200x500]: the dB
    spectrograms of the input, of what the walk left and of what it took out per group, as <input stem>.song.png,
    .residual.png and .group<g>.png (plot_specs, util_audio.py:938-960), levels and PNG files made on the device
    (audio.save_spectrograms), all against the song's own maximum.

    --gold GOLD.mid (one file) / --gold-dir DIR (with --songs): score what was written against gold MIDI (amt_saga.score,
    DESIGN 27).  One file: <outfile stem>.score.json beside the .mid.  --songs: when the last song has been written, every
    song with a <stem>.mid in DIR is scored in ONE device call -- <stem>.score.json beside each .mid and scores.json for
    the collection; a song without a gold file is named on stderr and left out.  The .mid files as written are what is
    scored, so `python -m amt_saga.score` on the same files gives the same counts.

    --roll-dir DIR [--roll-width W, default 1200] [--roll-row-px N, default 5] (both modes): the piano roll of what was
    written, <stem>.roll.png -- pitches 21..108, from 0 to the song's duration, a tick every second, coloured by
    instrument group, so that it lines up with <stem>.song.png at the same width -- and, for a song with a gold file
    (--gold / --gold-dir), <stem>.roll.gold.png: estimate only, gold only, both.  Drawn and encoded on the device
    (amt_saga.roll); with --songs all rolls of the collection come from ONE rasteriser call after the last song.

    --hpss [--hpss-kernel TxF, default 31x31] [--hpss-power {1,2,inf}, default 2] [--hpss-margin H,P, default 1,1] (both
    modes): a median-filter harmonic/percussive split of the song on the device (audio.hpss) after resampling,
    at the model's rate; the harmonic part is what is transcribed -- the heads were trained on pitched notes only, with
    drum tracks in the audio (util_audio.py:843, util_train_test.py:83).  --percussive OUT.flac (one file) /
    --percussive-dir DIR (with --songs, <stem>.percussive.flac) writes the percussive part through the writer --format,
    --flac and --flac-predictor choose; with --spectrogram-dir also <stem>.percussive.png against the song's own maximum.
    With --traversal song, residual + stems + percussive is the song.  Without --hpss nothing changes.

    --tempo-map [--quantize DIV] (both modes): the beats of every song, tracked on the device (amt_saga.beat)
    on the signal as given -- after resampling, before any --hpss split -- go into the .mid as a tempo map, every beat on a
    multiple of 480 ticks and every note where it was in seconds to within half a tick; --quantize snaps onsets to 1/DIV
    of a beat and is refused without --tempo-map.  --beats-out FILE (one file) / --beats-dir DIR (with --songs,
    <stem>.beats.txt) writes the beat times, one per line.  Without these the .mid is byte for byte what it was.

    --instrument-model NAME (both modes): the instrument head is the reference's model NAME (training.py:466-477; one of
    loop.INSTRUMENT_MODELS), fed the recipe arrays that model was trained on; the default is the plain CQT model.

Weights: a directory with {timing_start,timing_end,pitch,instrument,velocity}.npz in the
naming of amt_saga/rdcnn.py (the instrument net's file is <its model's name>.npz: instrument.npz by default); without it the heads carry their seeded synthetic weights (the
reference ships no checkpoint), which exercises the whole path but transcribes nothing.
"""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

from . import audio, beat as beat_mod, events as ev, flac as host_flac, png as host_png, roll as host_roll, score as host_score, wav as host_wav
from .hyperparams import Hyperparams
from .loop import INSTRUMENT_MODELS, TranscriptionLoop


def window_starts(n_samples, win_len, hop_len):
    """Start samples of the 50 %-overlapped windows covering the song (the last one is
    zero-padded)."""
    if n_samples <= win_len:
        return [0]
    n = 1 + int(np.ceil((n_samples - win_len) / hop_len))
    return [i * hop_len for i in range(n)]


def cut_windows(wf, win_len, hop_len):
    starts = window_starts(len(wf), win_len, hop_len)
    out = np.zeros((len(starts), win_len), dtype=np.float32)
    for i, s in enumerate(starts):
        seg = wf[s:s + win_len]
        out[i, :len(seg)] = seg
    return out, starts


def _model_option(instrument_model):
    """The keyword that names a non-default instrument model to _make_loop; none for the default, whose call stays the
    six-argument one that callers wrap (a cache of loops keyed by those six)."""
    return {} if instrument_model == 'instrument' else {'instrument_model': instrument_model}


def _hpss_option(hpss, percussive=False):
    """The `hpss` argument of transcribe / iter_transcribe_songs as audio.hpss's keywords: None (off) for None / False,
    {} for True, a dict of kernel / power / margin checked by audio.hpss_params.  ValueError before any device work."""
    if hpss is None or hpss is False:
        if percussive:
            raise ValueError('percussive=True needs hpss')
        return None
    opts = {} if hpss is True else hpss
    if not isinstance(opts, dict) or set(opts) - {'kernel', 'power', 'margin'}:
        raise ValueError("hpss: True, or a dict of 'kernel', 'power', 'margin' . Got: %r" % (hpss,))
    audio.hpss_params(**opts)
    return dict(opts)


def _beats_option(beats, p):
    """The `beats` argument of transcribe / iter_transcribe_songs as beat.beat_track's keywords: None (off) for None /
    False, {} for True, a dict of beat.params's bpm / tightness / mean_s / centre / octaves, checked at the model's rate
    and hop.  ValueError before any device work."""
    if beats is None or beats is False:
        return None
    opts = {} if beats is True else beats
    if not isinstance(opts, dict) or set(opts) - {'bpm', 'tightness', 'mean_s', 'centre', 'octaves'}:
        raise ValueError("beats: True, or a dict of 'bpm', 'tightness', 'mean_s', 'centre', 'octaves' . Got: %r" % (beats,))
    beat_mod.params(p.sr, p.H, **opts)
    return dict(opts)


class Song:
    """What one transcribed song carries from waveform to files -- THE list of outputs; every docstring below means these.
    index: the song's place in the queue (0 for transcribe()).  samples: its length at the model's rate, as walked.
    notes: list of dicts (pitch, program, velocity, start, end; from a song walk also `song`, the index).  events: the raw
    int32 records.
    residual: what the walk left, a 1-d float32 device tensor of hop * (frames - 1) samples.  stems: what it took out,
    [len(groups), hop * (frames - 1)], row g of groups[g].  percussive: the percussive waveform of an hpss split, 1-d
    float32 on the device.  beats: beat.beat_track's dict(period, tempo, beats, frames).
    A field nobody asked for is None; so are residual and stems of a song whose walk stopped before its end."""
    __slots__ = ('index', 'samples', 'notes', 'events', 'residual', 'stems', 'percussive', 'beats')

    def __init__(self, index, samples, notes=None, events=None, residual=None, stems=None, percussive=None, beats=None):
        self.index, self.samples, self.notes, self.events = index, samples, notes, events
        self.residual, self.stems, self.percussive, self.beats = residual, stems, percussive, beats


def _result(song, residual, stems, percussive, beats, indexed=False):
    """A Song as the tuple the public functions document: (notes, events[, residual][, stems][, percussive][, beats]),
    an optional item present when its want is true; indexed=True puts the song's index in front (the queue's form).
    The only place that builds or orders that tuple."""
    fields = ((indexed, song.index), (True, song.notes), (True, song.events), (residual, song.residual),
              (stems, song.stems), (percussive, song.percussive), (beats, song.beats))
    return tuple(value for want, value in fields if want)


def _on_device(wf):
    return isinstance(wf, torch.Tensor) and wf.is_cuda


def _device_mono(wf):
    """One mono waveform, array or tensor, as the 1-d float32 device tensor beat.beat_track and audio.hpss take."""
    w = wf if _on_device(wf) else torch.from_numpy(np.ascontiguousarray(wf, dtype=np.float32).reshape(-1)).cuda()
    return w.to(torch.float32).reshape(-1)


def _prepare(wf, sr, p, tracked, split):
    """What happens to a song's waveform ahead of either traversal, in this order: resampled from `sr` to p.sr on the
    device (sr given: audio.resample, a downmix at equal rates); beat-tracked on the signal as given (tracked: the
    keywords of beat.beat_track at the model's p.N / p.H -- a signal too short for the STFT's padding has no beats);
    split by audio.hpss at p.N / p.H, the harmonic part going on (split: its keywords).
    -> (waveform at p.sr, percussive waveform or None, beat dict or None)."""
    if sr is not None:
        wf = audio.resample(wf, sr, p.sr)                              # 1-d float32, on the device
    found = drums = None
    if tracked is not None:
        w = _device_mono(wf)
        found = dict(period=0, tempo=None, beats=[], frames=[]) if w.numel() <= p.N // 2 else \
            beat_mod.beat_track([w], p.sr, n_fft=p.N, hop=p.H, **tracked)[0]
    if split is not None:
        wf, drums = audio.hpss([_device_mono(wf)], n_fft=p.N, hop=p.H, **split)[0][:2]
    return wf, drums, found


def _make_loop(p, iters, heads, groups, weights_dir, guess, instrument_model='instrument'):
    loop = TranscriptionLoop(p, heads=heads, iters=iters, groups=groups, guess=guess, instrument_model=instrument_model)
    if weights_dir:
        for name, net in loop.nets.items():
            # the instrument net's file carries its model's name, as the reference's checkpoints do (training.py:76-98)
            f = os.path.join(weights_dir, (instrument_model if name == 'instrument' else name) + '.npz')
            if os.path.exists(f):
                net.load_weights(f)
    return loop.setup_device()


def _song_records(pairs, p, loop, slots=None, iters=5, silence=1e-3, poll=16, pool_frames=None, residual=False,
                  stems=False, on_finish=None, split=None, tracked=None, percussive=False, in_flight=None):
    """The Songs of `pairs` -- (waveform, its rate or None for p.sr) each, pulled lazily and through _prepare -- by the
    song walk, as they finish.  slots=None: the first song alone through run_songs (events [steps, 1, 9]); else all of
    them through iter_song_queue's `slots` windows (events [k, 9], notes with `song`).  on_finish(song, slot, state):
    the walk's hook with the Song of the song in flight in place of its index -- song.percussive is there for it.
    percussive: keep the percussive parts; in_flight: a caller's dict that holds {index: percussive waveform} meanwhile."""
    flight = {}

    def feed():
        for i, (wf, sr) in enumerate(pairs):
            w, drums, found = _prepare(wf, sr, p, tracked, split)
            if not _on_device(w):
                w = np.ascontiguousarray(w, dtype=np.float32)
            flight[i] = Song(i, len(w), percussive=drums if percussive else None, beats=found)   # (kept only if asked)
            if in_flight is not None:
                in_flight[i] = drums
            yield w
    hook = None if on_finish is None else lambda i, slot, st: on_finish(flight[i], slot, st)

    def alone():
        events, st = loop.run_songs([next(feed())], max_notes=iters, silence=silence, residual=residual, stems=stems)
        evs = events.cpu().numpy()
        if hook is not None:
            hook(0, 0, st)
        yield 0, evs, dict(residual=st.residual[0] if residual else None, stems=st.stem_audio[0] if stems else None)

    def queued():
        kinds = [k for k, want in (('residual', residual), ('stems', stems)) if want]     # iter_song_queue's own order
        for i, evs, *kept in loop.iter_song_queue(feed(), slots, max_notes=iters, silence=silence, poll=poll,
                                                  pool_frames=pool_frames, on_finish=hook, residual=residual,
                                                  stems=stems):
            yield i, evs, dict(zip(kinds, kept))
    for i, evs, kept in (alone() if slots is None else queued()):
        song = flight.pop(i)
        if in_flight is not None:
            in_flight.pop(i, None)
        one = evs
        if slots is not None:
            one = evs.copy()
            one[:, 0] = 0                                              # song_events_to_notes indexes scalars by song 0
        song.notes = ev.song_events_to_notes(one, 1 + song.samples // p.H, song.samples, sr=p.sr)
        if slots is not None:
            for note in song.notes:
                note['song'] = i
        song.events, song.residual, song.stems = evs, kept.get('residual'), kept.get('stems')
        yield song


def _record(wf, sr, p, loop, traversal, batch=1024, split=None, tracked=None, percussive=False, **walk):
    """The Song of one waveform by either traversal: 'song' is the one-song case of _song_records (`walk`: its iters,
    silence, residual, stems, on_finish); 'windows' cuts independent 50 %-overlapped windows, merges duplicates, keeps
    nothing and calls nothing back, so `walk` is not looked at."""
    if traversal == 'song':
        return next(_song_records([(wf, sr)], p, loop, split=split, tracked=tracked, percussive=percussive, **walk))
    wf, drums, found = _prepare(wf, sr, p, tracked, split)
    on_dev = _on_device(wf)
    L = p.H * (p.timing_frames - 1)
    wf_dev = wf if on_dev else torch.from_numpy(np.ascontiguousarray(wf, dtype=np.float32)).cuda()
    wins, starts = cut_windows(wf.cpu().numpy() if on_dev else np.asarray(wf, dtype=np.float32), L, L // 2)
    # song-level normalisers, as training.py:269-282 computes them: once per song, the maxima of the WHOLE song's
    # STFT and CQTs (one pass of the block-sum kernel over the song as a single signal), shared by every window
    song_refs = loop.song_levels(wf_dev)
    # the loop proper: host batches streamed through run_stream (copy of batch i+1 under the compute of batch i)
    chunks = [wins[b0:b0 + batch] for b0 in range(0, len(wins), batch)]

    def refs_for(i):
        return {k: v.expand(len(chunks[i])).contiguous() for k, v in song_refs.items()}
    evs = np.concatenate([e.cpu().numpy() for e, _ in loop.run_stream(chunks, refs=refs_for)], axis=1)
    notes = ev.events_to_notes(evs, p.timing_frames, L, sr=p.sr, window_start_s=[s / p.sr for s in starts])
    return Song(0, len(wf), ev.merge_overlap_duplicates(notes), evs, percussive=drums if percussive else None, beats=found)


def _by_index(on_finish):
    """The public on_finish(index, slot, state) as _song_records' hook, which is handed the Song."""
    return None if on_finish is None else lambda song, slot, st: on_finish(song.index, slot, st)


def transcribe(wf, params=None, iters=5, heads=('timing', 'pitch', 'instrument', 'velocity'),
               groups=(0, 1, 2), weights_dir=None, guess='bank', loop=None, batch=1024, traversal='windows',
               silence=1e-3, sr=None, residual=False, stems=False, instrument_model='instrument', on_finish=None,
               hpss=None, percussive=False, beats=False):
    """wf: float32 mono waveform at params.sr -- or, with `sr` given, a waveform [n] or [n, channels] at `sr`, resampled
    to params.sr (and downmixed) on the device first (audio.resample): everything below, the length the note times are
    computed from included, then sees the resampled signal.  Returns (notes, events) where notes is the
    merged list of dicts (pitch, program, velocity, start, end) and events the raw int32
    [iters, n_windows, 7] records -- the fields of a Song, put in order by _result.
    traversal='windows' (default): independent 50 %-overlapped windows, `iters` notes each, duplicates merged.
    traversal='song': the reference's own walk (training.py:296-328, TranscriptionLoop.run_songs) -- one window that
    lives on the song's spectrogram and slides by half, at most `iters` notes per position (max_notes), windows below
    `silence` x the song's maximum skipped; events are then the [steps, 1, 9] song records and nothing needs merging.
    residual=True (traversal='song' only; the independent windows have no song-level residual: ValueError): returns
    (notes, events, residual) with the song's residual waveform at params.sr, a 1-d float32 device tensor of
    hop * (frames - 1) samples (run_songs(residual=True)); None if the walk stopped before the song's end.
    stems=True (traversal='song' only: ValueError): the song's instrument stems, a [len(groups), hop * (frames - 1)]
    float32 device tensor (run_songs(stems=True); row g belongs to groups[g]), are appended to what is returned --
    (notes, events[, residual][, stems]).
    instrument_model: which of the reference's ten instrument models the instrument head is (loop.INSTRUMENT_MODELS);
    no effect on a `loop` handed in.
    on_finish(0, 0, state) (traversal='song' only): called after the walk with the song's SongState, its pool still in
    place -- iter_song_queue's hook; state.region_spectra([0]) is what write_song_spectrograms draws.
    hpss=True, or a dict of audio.hpss's kernel / power / margin: the waveform, once resampled, is split by audio.hpss
    at params.N / params.H and the HARMONIC part (hop * (len // hop) samples) is what either traversal sees.
    percussive=True (needs hpss: ValueError) appends the percussive waveform, a 1-d float32 device tensor, to what is
    returned.  hpss=None: nothing changes.
    beats=True, or a dict of beat.params's keywords: the waveform as given -- once resampled, before any hpss split -- is
    beat-tracked on the device (beat.beat_track at params.N / params.H) and the song's dict(period, tempo, beats,
    frames) is appended last to what is returned; events.write_midi(notes, path, beats=that['beats']) writes the tempo
    map.  Notes and events are those of the run without it."""
    if traversal not in ('windows', 'song'):
        raise ValueError('Requested attribute does not exist')
    split = _hpss_option(hpss, percussive)
    if residual and traversal != 'song':
        raise ValueError("transcribe: residual=True needs traversal='song'")
    if stems and traversal != 'song':
        raise ValueError("transcribe: stems=True needs traversal='song'")
    p = params or Hyperparams(N=2048)
    tracked = _beats_option(beats, p)
    if loop is None:
        loop = _make_loop(p, iters, heads, groups, weights_dir, guess, **_model_option(instrument_model))
    song = _record(wf, sr, p, loop, traversal, batch, split, tracked, percussive, iters=iters, silence=silence,
                   residual=residual, stems=stems, on_finish=_by_index(on_finish))
    return _result(song, residual, stems, percussive, tracked is not None)


def iter_transcribe_songs(wfs, params=None, iters=5, heads=('timing', 'pitch', 'instrument', 'velocity'),
                          groups=(0, 1, 2), weights_dir=None, guess='bank', loop=None, slots=8, silence=1e-3, poll=16,
                          pool_frames=None, residual=False, stems=False, instrument_model='instrument', on_finish=None,
                          hpss=None, percussive=False, beats=False):
    """The song queue behind transcribe_songs (TranscriptionLoop.iter_song_queue): yields (index, notes, events) as
    each song finishes, in finishing order -- (index, notes, events[, residual waveform][, stems [G, samples]]) with
    residual=True / stems=True: the fields of a Song, put in order by _result.  wfs: a sequence or an iterator of mono
    float32 waveforms at params.sr; an
    item may also be a (waveform [n] or [n, channels], sr) pair, which is resampled to params.sr on the device as it is
    pulled (audio.resample).  on_finish(index, slot, state): iter_song_queue's hook, called when a song is found
    finished, before its slot and its pool region are given away.
    hpss (True or a dict, see transcribe): every song is split by audio.hpss as it is pulled, after resampling, and its
    harmonic part is what the queue walks.  percussive (needs hpss: ValueError): the song's percussive waveform is
    appended to what is yielded; a dict in place of True is also filled with {index: percussive waveform} while the
    song is in flight, which is where an on_finish hook finds it.
    beats (True or a dict, see transcribe): every song is beat-tracked as it is pulled, after resampling and before any
    split -- three device calls and one copy back per song -- and its beat dict is appended last to what is yielded."""
    want = percussive is True or isinstance(percussive, dict)
    split = _hpss_option(hpss, want)
    p = params or Hyperparams(N=2048)
    tracked = _beats_option(beats, p)
    if loop is None:
        loop = _make_loop(p, iters, heads, groups, weights_dir, guess, **_model_option(instrument_model))
    for song in _song_records(_pairs(wfs), p, loop, slots, iters, silence, poll, pool_frames, residual, stems,
                              _by_index(on_finish), split, tracked, want,
                              percussive if isinstance(percussive, dict) else None):
        yield _result(song, residual, stems, want, tracked is not None, indexed=True)


def _pairs(wfs):
    """The queue's input as (waveform, rate) pairs: a bare item is a host waveform at the model's rate (None)."""
    for wf in wfs:
        yield wf if isinstance(wf, tuple) else (np.ascontiguousarray(wf, dtype=np.float32).reshape(-1), None)


def transcribe_songs(wfs, params=None, slots=8, **kw):
    """A collection of songs through the song queue: `slots` live windows, a finished slot refilled with the next
    song.  Returns [(notes, events [k, 9]), ...] in input order; a song's notes are those of
    transcribe(wf, traversal='song') for it alone (with `song` = its index).  residual=True / stems=True:
    (notes, events[, residual][, stems]); beats=True appends each song's beat dict."""
    out = {i: tuple(rest) for i, *rest in iter_transcribe_songs(wfs, params, slots=slots, **kw)}
    return [out[i] for i in range(len(out))]


CLI_GROUPS = (0, 1, 2)                                             # the command line's instrument groups (reference ids)


FLAC_WRITERS = ('host', 'device')
_FLAC_HELP = ("writer of --residual / --residual-dir / --stems-dir: 'host' = the VERBATIM writer (uncompressed FLAC, the "
              "default), 'device' = the HIP encoder (fixed predictors + Rice coding, one call per song); no effect with "
              "--format wav")


FLAC_PREDICTORS = audio.FLAC_PREDICTORS
_FLAC_PREDICTOR_HELP = ("predictors of --flac device: 'fixed' (the default) = the fixed orders 0..4, 'lpc' = linear "
                        "prediction of order 1..12 beside them (smaller files for tonal audio, more encoding time); the "
                        "host writer has no predictors, so 'lpc' with --flac host is refused; no effect with --format wav")


FORMATS = ('flac', 'wav')
_FORMAT_HELP = ("container of --residual / --residual-dir / --stems-dir: 'flac' (the default) or 'wav' = PCM-24 WAV packed "
                "on the device (audio.save_wav), a song's residual and stems in one call, the generated names ending in "
                ".residual.wav and .group<g>.wav; with 'wav', --flac has no effect")


_SPECTROGRAM_HELP = ('with --traversal song, or with --songs: write <stem>.song.png (the STFT of the input), '
                     '<stem>.residual.png (what the walk left) and <stem>.group<g>.png (what it took out, per '
                     'instrument group) per song as it finishes: dB spectrograms over 80 dB on a log frequency axis, '
                     'all drawn against the song\'s own maximum, so that a colour is a level across them; levels and '
                     'PNG files are made on the device, one levels call and one encode call per song')


_ROLL_HELP = ('write <stem>.roll.png per song: the piano roll of the notes written, pitches 21..108 from 0 to the '
              'song\'s duration with a tick every second, coloured by instrument group; with --gold / --gold-dir also '
              '<stem>.roll.gold.png for a song that has a gold file: estimate only, gold only, both; rasteriser and PNG '
              'encoder run on the device')
ROLL_PITCH = (21, 108)


DECODERS = ('host', 'device')
_DECODE_HELP = ("reader of the input files: 'host' = the pure-Python reader (the default), 'device' = the HIP decoder "
                "(--songs: --slots files per decode call, as the queue pulls them; CRC-8, CRC-16 and MD5 verified as the "
                "host reader does).  A mono "
                "file gives the same samples and the same .mid either way; a file with channels and no --sr is mixed "
                "down in float32 on the device and in float64 on the host, so its samples may differ in the last bit")


def _shared_options(ap, sr_help, **stems_dir):
    """The options both command-line modes have; the help of --sr and --stems-dir is the mode's own."""
    ap.add_argument('--weights', default=None)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--guess', default='bank', choices=('bank', 'render'))
    ap.add_argument('--instrument-model', default='instrument', choices=tuple(INSTRUMENT_MODELS), metavar='NAME',
                    help='which of the ten instrument models the instrument head is: ' + ', '.join(INSTRUMENT_MODELS) +
                         '; --weights then looks for NAME.npz')
    ap.add_argument('--sr', type=int, default=None, help=sr_help)
    ap.add_argument('--stems-dir', default=None, **stems_dir)
    ap.add_argument('--flac', default='host', choices=FLAC_WRITERS, help=_FLAC_HELP)
    ap.add_argument('--flac-predictor', default='fixed', choices=FLAC_PREDICTORS, help=_FLAC_PREDICTOR_HELP)
    ap.add_argument('--decode', default='host', choices=DECODERS, help=_DECODE_HELP)
    ap.add_argument('--format', default='flac', choices=FORMATS, help=_FORMAT_HELP)
    ap.add_argument('--spectrogram-dir', default=None, metavar='DIR', help=_SPECTROGRAM_HELP)
    ap.add_argument('--spectrogram-size', default='1200x500', metavar='WxH',
                    help='pixels of every --spectrogram-dir image, each side 1 .. 16384 (default 1200x500)')
    ap.add_argument('--hpss', action='store_true', help=_HPSS_HELP)
    ap.add_argument('--hpss-kernel', default='31x31', metavar='TxF',
                    help='median lengths of --hpss in frames x bins, each odd and in 1 .. 63 (default 31x31)')
    ap.add_argument('--hpss-power', default='2', choices=('1', '2', 'inf'),
                    help='exponent of the soft masks of --hpss; inf: hard masks, a tie is harmonic (default 2)')
    ap.add_argument('--hpss-margin', default='1,1', metavar='H,P',
                    help='margins of --hpss for the harmonic and the percussive mask, each in 1 .. 100 (default 1,1); '
                         'above 1 a third part belongs to neither and is dropped')
    ap.add_argument('--tempo-map', action='store_true', help=_TEMPO_MAP_HELP)
    ap.add_argument('--quantize', type=int, default=None, metavar='DIV', choices=ev.QUANTIZE_DIVISIONS,
                    help='with --tempo-map: snap every onset to 1/DIV of a beat (480 / DIV ticks), durations kept; one of '
                         + ', '.join(map(str, ev.QUANTIZE_DIVISIONS)))
    ap.add_argument('--roll-dir', default=None, metavar='DIR', help=_ROLL_HELP)
    ap.add_argument('--roll-width', type=int, default=1200, metavar='W',
                    help='pixel columns of every --roll-dir image, 1 .. 16384 (default 1200)')
    ap.add_argument('--roll-row-px', type=int, default=5, metavar='N',
                    help='pixel rows per pitch of every --roll-dir image, 1 .. 186 (default 5: 440 rows)')


_TEMPO_MAP_HELP = ('track the beats of every song on the device (amt_saga.beat: the signal as given, after resampling and '
                   'before any --hpss split) and write them into the .mid as a tempo map: every beat on a multiple of 480 '
                   'ticks, time 0 on tick 0, every note where it was in seconds to within half a tick.  A song with fewer '
                   'than two beats keeps the fixed 120 bpm.  Without it the .mid is what it was')


def _beats_cli(a, beats_out):
    """True when the beats are wanted (--tempo-map, or `beats_out`, the value of --beats-out / --beats-dir); --quantize
    without --tempo-map is refused, before any file is read."""
    if a.quantize is not None and not a.tempo_map:
        raise SystemExit('--quantize needs --tempo-map (there is no beat grid to snap to without it)')
    return bool(a.tempo_map or beats_out is not None)


def write_beats(path, found):
    """One beat time per line, seconds with microseconds."""
    with open(path, 'w') as f:
        f.write(''.join('%.6f\n' % t for t in found['beats']))
    print('%d beats -> %s' % (len(found['beats']), path))


_HPSS_HELP = ('split every song into a harmonic and a percussive part on the device before it is transcribed (median '
              'filtering, after resampling, at the model\'s rate) and transcribe the harmonic part: the heads know pitched '
              'notes only, and a drum hit is energy none of them can explain.  With --traversal song, residual + stems + '
              'percussive is the song.  Without --hpss nothing changes')


def _hpss_cli(a, percussive):
    """audio.hpss's keywords from --hpss-kernel / --hpss-power / --hpss-margin, or None without --hpss; `percussive` (the
    value of --percussive / --percussive-dir) without --hpss and malformed strings are refused, before any file is read."""
    if not a.hpss:
        if percussive is not None:
            raise SystemExit('--percussive / --percussive-dir needs --hpss (there is no percussive part without the split)')
        return None
    try:
        kernel = tuple(int(k) for k in a.hpss_kernel.lower().split('x'))
        if len(kernel) != 2:
            raise ValueError
    except ValueError:
        raise SystemExit('--hpss-kernel: expected TxF, two odd integers in 1 .. 63 . Got: %s' % a.hpss_kernel)
    try:
        margin = tuple(float(m) for m in a.hpss_margin.split(','))
        if len(margin) != 2:
            raise ValueError
    except ValueError:
        raise SystemExit('--hpss-margin: expected H,P, two numbers in 1 .. 100 . Got: %s' % a.hpss_margin)
    for option, given in (('--hpss-kernel', dict(kernel=kernel)), ('--hpss-margin', dict(margin=margin))):
        try:
            audio.hpss_params(**given)
        except ValueError as e:
            raise SystemExit('%s: %s' % (option, e))
    return dict(kernel=kernel, power=float(a.hpss_power), margin=margin)


def _check_writer(a):
    """--flac-predictor lpc asks for the device encoder: refused with the host writer, before any work."""
    if a.flac_predictor == 'lpc' and a.flac == 'host' and a.format == 'flac':
        raise SystemExit('--flac-predictor lpc needs --flac device (the host writer has no predictors)')


def _is_wav(path):
    """True for a file that begins with RIFF; every other file, and a missing one, is left to the FLAC path."""
    try:
        return host_wav.is_wav(path)
    except OSError:
        return False


def _load_float(path):
    """(float64 waveform, rate) of one file on the host: amt_saga.wav's reader for a RIFF file, else the FLAC reader."""
    return (host_wav if _is_wav(path) else host_flac).load_float(path)


def _read_inputs(paths, decode, group=1):
    """(waveform, rate) of every file of `paths` in order, lazily.  decode='host': read one by one, float64 arrays.
    decode='device': audio.load_audio calls of `group` files each, made as the consumer pulls them, the waveforms device
    tensors -- the bytes, the scratch and the samples on the device are those of one such group and of the songs in
    flight, not of the collection."""
    if decode == 'device':
        step = max(1, group)
        for k in range(0, len(paths), step):
            for wf, sr, _ in audio.load_audio(list(paths[k:k + step])):
                yield wf, sr
    else:
        for f in paths:
            yield _load_float(f)


def _mono(wf, sr, decode):
    """A file's waveform [n] or [n, channels] as one channel at its own rate `sr`: the float64 mean of the channels on
    the host, audio.resample at equal rates (a float32 mean) on the device; a mono waveform passes through."""
    if decode == 'device':
        return audio.resample(wf, sr, sr)
    return wf.mean(axis=1) if wf.ndim > 1 else wf


def write_song_audio(rate, residual=None, residual_path=None, stems=None, stems_dir=None, name=None, flac='host',
                     format='flac', predictor='fixed', percussive=None, percussive_path=None):
    """What a song walk kept, as 24-bit FLAC at `rate`: `residual` (1-d device tensor) to residual_path, and / or the rows
    of `stems` [G, samples] to <stems_dir>/<name>.group<g>.flac, g the reference group id of the row (CLI_GROUPS).
    flac='host': the VERBATIM writer of amt_saga.flac, file by file (the default: the bytes every earlier call wrote);
    flac='device': audio.save_flac -- the residual and all stems of the song in ONE encode call on the device,
    compressed, and no sample crosses to the host before it is coded.
    format='wav': PCM-24 WAV instead, <name>.group<g>.wav, through audio.save_wav -- one pack call and one copy for the
    residual and all stems of the song; `flac` then has no effect.
    predictor='lpc' (with flac='device'): save_flac's LPC subframes beside the fixed predictors; the host writer has no
    predictors and refuses it.
    percussive (1-d device tensor, the percussive part of an --hpss split) goes to percussive_path the same way, in the
    same call."""
    if flac not in FLAC_WRITERS or format not in FORMATS or predictor not in FLAC_PREDICTORS:
        raise ValueError('Requested attribute does not exist')
    if predictor == 'lpc' and flac == 'host' and format == 'flac':
        raise ValueError("predictor='lpc' needs flac='device': the host writer has no predictors")
    waves, paths, notes = [], [], []
    if residual is not None:
        waves.append(residual)
        paths.append(residual_path)
        notes.append('residual -> %s' % residual_path)
    if stems is not None:
        for row, g in zip(stems, CLI_GROUPS):
            waves.append(row)
            paths.append(os.path.join(stems_dir, '%s.group%d.%s' % (name, g, format)))
            notes.append('stem of group %d -> %s' % (g, paths[-1]))
    if percussive is not None:
        waves.append(percussive)
        paths.append(percussive_path)
        notes.append('percussive -> %s' % percussive_path)
    if not waves:
        return
    if format == 'wav':
        audio.save_wav(waves, paths, rate, fmt='pcm24')
    elif flac == 'device':
        audio.save_flac(waves, paths, rate, predictor=predictor)
    else:
        for w, path in zip(waves, paths):
            host_flac.save_float(np.ascontiguousarray(w.cpu().numpy()), path, sr=rate)
    for line in notes:
        print(line)


def _spectrogram_size(a):
    """(W, H) of --spectrogram-size, checked before any work; None without --spectrogram-dir."""
    if a.spectrogram_dir is None:
        return None
    try:
        return host_png.parse_size(a.spectrogram_size)
    except ValueError as e:
        raise SystemExit('--spectrogram-size: ' + str(e))


def write_song_spectrograms(st, slot, directory, name, size=(1200, 500), percussive=None):
    """The pictures of a finished song (plot_specs, util_audio.py:938-960: the reference's before / after comparison):
    <directory>/<name>.song.png from an STFT of the song's samples in the pool, <name>.residual.png from the region of
    the pool the slides wrote back, <name>.group<g>.png from its stem regions (g the reference group id of the row,
    CLI_GROUPS) -- SongState.region_spectra(slot), so the state keeps residual and stems and the song is finished
    (ValueError otherwise).  Every image: dB over 80 dB below the SONG's maximum (the slot's ref_mag, read on the
    device), log frequency axis, `size` = (W, H) pixels.  ONE audio.spectrogram_levels launch and ONE audio.png_encode
    call for all of them, on the walk's stream and ahead of the slot's release.  percussive (the percussive waveform of
    an --hpss split): also <name>.percussive.png, from its STFT, against the same maximum, in the same two calls."""
    residual, stems = st.region_spectra([slot])[0]
    p, f0 = st.lp.p, st.region[slot]
    song = audio.AudioBatch(st.samples[f0 * p.H:f0 * p.H + st.lens[slot]][None, :], p.N, p.H, sample_rate=p.sr).stft(False)
    mags, kinds = [song.mag[0]], ['song']
    if residual is not None:
        mags.append(residual)
        kinds.append('residual')
    if stems is not None:
        for row, g in zip(stems.unbind(0), CLI_GROUPS):
            mags.append(row)
            kinds.append('group%d' % g)
    if percussive is not None:
        mags.append(audio.AudioBatch(percussive[None, :], p.N, p.H, sample_rate=p.sr).stft(False).mag[0])
        kinds.append('percussive')
    paths = [os.path.join(directory, '%s.%s.png' % (name, k)) for k in kinds]
    audio.save_spectrograms(mags, paths, [st.refs['ref_mag'][slot]] * len(mags), size=size, sr=p.sr, n_fft=p.N)
    for path in paths:
        print('spectrogram -> %s' % path)


def _roll_size(a):
    """(width, row_px) of --roll-width / --roll-row-px and the directory of --roll-dir, checked before any work; None
    without --roll-dir."""
    if a.roll_dir is None:
        return None
    if os.path.exists(a.roll_dir) and not os.path.isdir(a.roll_dir):
        raise SystemExit('--roll-dir: %s is not a directory' % a.roll_dir)
    try:
        return host_roll.geometry(0, a.roll_width, a.roll_row_px, ROLL_PITCH)[:2]
    except ValueError as e:
        raise SystemExit('--roll-width / --roll-row-px: ' + str(e))


def write_rolls(names, mid_paths, durations, directory, size, gold_paths=None):
    """The piano rolls of written .mid files (amt_saga.roll): <directory>/<name>.roll.png for every song, and
    <name>.roll.gold.png for every song whose entry of gold_paths is not None, read by score.read_gold.  Pitches 21..108,
    from 0 to the song's duration in seconds (at least one microsecond a column), a tick every second, the loop's
    instrument groups; size = (width, row_px).  ONE rasteriser call for all of them."""
    notes = [ev.read_midi(p, full=True) for p in mid_paths]
    gold_paths = [None] * len(names) if gold_paths is None else list(gold_paths)
    pairs = [i for i, g in enumerate(gold_paths) if g is not None]
    spans = [(0.0, max(float(d), size[0] * 1e-6)) for d in durations]
    paths = [os.path.join(directory, nm + '.roll.png') for nm in names] + \
        [os.path.join(directory, names[i] + '.roll.gold.png') for i in pairs]
    host_roll.save_piano_rolls(notes + [notes[i] for i in pairs], paths,
                               [None] * len(names) + [host_score.read_gold(gold_paths[i]) for i in pairs],
                               width=size[0], row_px=size[1], pitch=ROLL_PITCH, span=spans + [spans[i] for i in pairs],
                               tick=1.0, group=host_score.loop_groups())
    for path in paths:
        print('roll -> %s' % path)


def _note_durations(wfs, rate, out):
    """`wfs` passed through, the seconds of every item appended to `out` as it is pulled: an item is a waveform at `rate`
    or a (waveform, rate) pair."""
    for item in wfs:
        wf, sr = item if isinstance(item, tuple) else (item, rate)
        out.append(int(wf.shape[0]) / float(sr))
        yield item


def write_scores(names, mid_paths, gold_paths, collection_path=None):
    """Score the written .mid files against their gold files in one device call (score.score_files with the loop's
    instrument groups): <mid path minus its extension>.score.json per song, and collection_path (scores.json) for the
    collection when it is given.  Returns the collection's record."""
    import json
    counts, summ = host_score.score_files(mid_paths, gold_paths, group=host_score.loop_groups())
    pairs, whole = host_score.report(names, mid_paths, gold_paths, counts, summ)
    for mid, rec in zip(mid_paths, pairs):
        out = os.path.splitext(mid)[0] + '.score.json'
        with open(out, 'w') as f:
            json.dump(rec, f, sort_keys=True)
        print('score -> %s' % out)
    if collection_path is not None:
        with open(collection_path, 'w') as f:
            json.dump(dict(whole, songs=pairs), f, sort_keys=True)
        print('scores -> %s' % collection_path)
    return whole


def _same_rate(paths, pairs, rate, decode):
    """The queue's input without --sr: every (waveform, rate) of `pairs` as one channel, a file of another rate than
    `rate` refused."""
    for f, (wf, sr) in zip(paths, pairs):
        if sr != rate:
            raise SystemExit('%s: sample rate %d differs from the first file\'s %d; one queue runs at one rate'
                             % (f, sr, rate))
        wf = _mono(wf, sr, decode)
        yield (wf, sr) if decode == 'device' else wf        # (the queue takes a device tensor as a pair; equal rates pass)


def _preflight(a, percussive, beats_out, own, own_first):
    """The checks both command-line modes make before a file is read, in the order each always made them: writer, split
    and beat options, then the image sizes -- the mode's `own` checks ahead of the sizes (own_first: the one-file mode)
    or after them.  -> (audio.hpss's keywords or None, beats wanted, spectrogram size or None, roll size or None)."""
    _check_writer(a)
    split, want_beats = _hpss_cli(a, percussive), _beats_cli(a, beats_out)
    if own_first:
        own()
    size, roll_size = _spectrogram_size(a), _roll_size(a)
    if not own_first:
        own()
    return split, want_beats, size, roll_size


def _make_dirs(*dirs):
    """Every output directory a command line was given, made before its first song is walked."""
    for d in dirs:
        if d is not None:
            os.makedirs(d, exist_ok=True)


def _cli_walk(a, rate, split, want_beats, keep_residual, draw, on_finish):
    """The model of a command line at `rate` and what it asks of the walk: (hyperparameters, loop, the keywords of
    _record / _song_records).  The pictures of --spectrogram-dir (draw) need the residual and the stems kept."""
    p = Hyperparams(N=2048, sr=rate)
    loop = _make_loop(p, a.iters, ('timing', 'pitch', 'instrument', 'velocity'), CLI_GROUPS, a.weights, a.guess,
                      **_model_option(a.instrument_model))
    return p, loop, dict(iters=a.iters, residual=keep_residual or draw, stems=a.stems_dir is not None or draw,
                         on_finish=on_finish if draw else None, split=split, tracked=_beats_option(want_beats, p),
                         percussive=split is not None)


def _write_song(a, song, rate, name, out, residual_option):
    """The files of one Song, in both modes: out['mid'] (with the tempo map under --tempo-map) and its line, then
    out['beats'], then the residual to out['residual'], the stems into --stems-dir as <name>.group<g>.<format> and the
    percussive part to out['percussive'] in ONE write_song_audio call; a path that is None is not written.  A walk that
    stopped before the song's end has no residual and no stems: refused under the mode's name of the option."""
    if a.tempo_map:
        ev.write_midi(song.notes, out['mid'], beats=song.beats['beats'], quantize=a.quantize)
    else:
        ev.write_midi(song.notes, out['mid'])
    print('%d notes -> %s' % (len(song.notes), out['mid']))
    if out['beats'] is not None:
        write_beats(out['beats'], song.beats)
    for option, asked, kept in ((residual_option, out['residual'], song.residual), ('--stems-dir', a.stems_dir, song.stems)):
        if asked is not None and kept is None:
            raise SystemExit('%s: the walk stopped before the end of the song' % option)
    write_song_audio(rate, residual=song.residual if out['residual'] is not None else None, residual_path=out['residual'],
                     stems=song.stems if a.stems_dir is not None else None, stems_dir=a.stems_dir, name=name,
                     flac=a.flac, format=a.format, predictor=a.flac_predictor,
                     percussive=song.percussive if out['percussive'] is not None else None,
                     percussive_path=out['percussive'])


def main_songs(argv):
    """The many-files mode: --songs a.flac b.flac ... --out-dir DIR [--slots N]; one .mid per input, written as its song
    finishes."""
    ap = argparse.ArgumentParser(description='song queue: one MIDI file per input file')
    ap.add_argument('--songs', nargs='+', required=True)
    ap.add_argument('--out-dir', required=True)
    ap.add_argument('--slots', type=int, default=8)
    ap.add_argument('--residual-dir', default=None,
                    help='write <stem>.residual.flac per song as it finishes: what the walk left after every subtraction, '
                         '24-bit FLAC at the rate the model runs at (with --sr, the resampled rate)')
    ap.add_argument('--percussive-dir', default=None, metavar='DIR',
                    help='with --hpss: write <stem>.percussive.flac per song as it finishes, the percussive part of the '
                         'split, through the writer --format, --flac and --flac-predictor choose')
    _shared_options(ap, 'rate the model runs at; every file is resampled to it from its own rate (mixed rates allowed)',
                    help='write <stem>.group<g>.flac per song and instrument group as it finishes: what the subtractions '
                         'took out of the song, 24-bit FLAC at the rate the model runs at')
    ap.add_argument('--gold-dir', default=None, metavar='DIR',
                    help='when the last song has been written, score every song that has a <stem>.mid in DIR against it, '
                         'all in one device call: <stem>.score.json beside each .mid and scores.json in --out-dir; a song '
                         'without a gold file is named on stderr and left out')
    ap.add_argument('--beats-dir', default=None, metavar='DIR',
                    help='write <stem>.beats.txt per song as it finishes: its beat times in seconds, one per line')
    a = ap.parse_args(argv)

    def own():
        if a.gold_dir is not None and not os.path.isdir(a.gold_dir):
            raise SystemExit('--gold-dir: %s is not a directory' % a.gold_dir)
    split, want_beats, size, roll_size = _preflight(a, a.percussive_dir, a.beats_dir, own, False)
    _make_dirs(a.out_dir, a.residual_dir, a.stems_dir, a.spectrogram_dir, a.roll_dir, a.percussive_dir, a.beats_dir)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in a.songs]
    if len(set(stems)) != len(stems):
        raise SystemExit('--songs: two inputs would write the same .mid (equal file names)')
    wfs = _read_inputs(a.songs, a.decode, a.slots)
    if a.sr is not None:                         # every file resampled to the model's rate as the queue pulls it
        if a.sr <= 0:
            raise SystemExit('--sr: the rate must be positive')
        rate = a.sr
    else:                                        # the model at the first file's rate, every other file held to it
        if a.decode == 'device':                 # the first file's header, on the host
            with open(a.songs[0], 'rb') as f0:
                head = f0.read()
            rate = (host_wav.read_header(head) if head[:4] == b'RIFF' else host_flac.read_streaminfo(head))[0]
        else:                                    # the first file itself, loaded once
            first = next(wfs)
            rate, wfs = first[1], itertools.chain([first], wfs)
        wfs = _same_rate(a.songs, wfs, rate, a.decode)
    durations = []
    if roll_size is not None:
        wfs = _note_durations(wfs, rate, durations)

    def on_finish(song, slot, st):
        write_song_spectrograms(st, slot, a.spectrogram_dir, stems[song.index], size, percussive=song.percussive)
    p, loop, walk = _cli_walk(a, rate, split, want_beats, a.residual_dir is not None, size is not None, on_finish)

    def path(directory, stem, kind):                                   # <dir>/<stem>.<kind>, None without the directory
        return None if directory is None else os.path.join(directory, '%s.%s' % (stem, kind))
    for song in _song_records(_pairs(wfs), p, loop, a.slots, **walk):
        stem = stems[song.index]
        _write_song(a, song, rate, stem, dict(mid=path(a.out_dir, stem, 'mid'), beats=path(a.beats_dir, stem, 'beats.txt'),
                                              residual=path(a.residual_dir, stem, 'residual.' + a.format),
                                              percussive=path(a.percussive_dir, stem, 'percussive.' + a.format)),
                    '--residual-dir')
    golds = [None] * len(stems)
    if a.gold_dir is not None:
        scored = []
        for i, stem in enumerate(stems):
            gold = os.path.join(a.gold_dir, stem + '.mid')
            if os.path.isfile(gold):
                scored.append((stem, os.path.join(a.out_dir, stem + '.mid'), gold))
                golds[i] = gold
            else:
                print('%s: no gold file in %s, left out of the scores' % (stem, a.gold_dir), file=sys.stderr)
        if scored:
            write_scores(*zip(*scored), collection_path=os.path.join(a.out_dir, 'scores.json'))
    if roll_size is not None:
        write_rolls(stems, [os.path.join(a.out_dir, s + '.mid') for s in stems], durations, a.roll_dir, roll_size, golds)


# what the one-file mode writes only with --traversal song: (option, what the independent windows do not have)
_SONG_ONLY = (('--residual', 'residual'), ('--stems-dir', 'stems'), ('--spectrogram-dir', 'spectra'))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if '--songs' in argv:
        return main_songs(argv)
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('infile')
    ap.add_argument('outfile')
    ap.add_argument('--traversal', default='windows', choices=('windows', 'song'),
                    help="'song': one sliding window per song with the residual kept (run_songs)")
    ap.add_argument('--residual', default=None, metavar='OUT.flac',
                    help='with --traversal song: write what the walk left of the song after every subtraction, 24-bit FLAC '
                         'at the rate the model runs at (with --sr, the resampled rate)')
    _shared_options(ap, 'rate the model runs at; the file is resampled to it from its own rate', metavar='DIR',
                    help='with --traversal song: write <input stem>.group<g>.flac per instrument group, what the '
                         'subtractions took out of the song, 24-bit FLAC at the rate the model runs at')
    ap.add_argument('--gold', default=None, metavar='GOLD.mid',
                    help='score the written file against this gold MIDI file: <outfile stem>.score.json beside it')
    ap.add_argument('--percussive', default=None, metavar='OUT.flac',
                    help='with --hpss: write the percussive part of the split, through the writer --format, --flac and '
                         '--flac-predictor choose')
    ap.add_argument('--beats-out', default=None, metavar='FILE',
                    help='write the beat times of the song in seconds, one per line')
    a = ap.parse_args(argv)

    def own():
        if a.gold is not None and not os.path.isfile(a.gold):
            raise SystemExit('--gold: %s: no such file' % a.gold)
        for option, noun in _SONG_ONLY:
            if getattr(a, option[2:].replace('-', '_')) is not None and a.traversal != 'song':
                raise SystemExit('%s needs --traversal song (independent windows have no song-level %s)' % (option, noun))
    split, want_beats, size, roll_size = _preflight(a, a.percussive, a.beats_out, own, True)
    wf, sr = next(_read_inputs([a.infile], a.decode))
    duration = int(wf.shape[0]) / float(sr)
    if a.sr is None:                             # the model at the file's rate
        wf, model_sr, file_sr = _mono(wf, sr, a.decode), sr, None
    elif a.sr <= 0:
        raise SystemExit('--sr: the rate must be positive')
    else:                                        # the file at the model's rate: resampled and downmixed on the device
        model_sr, file_sr = a.sr, sr
    name = os.path.splitext(os.path.basename(a.infile))[0]
    _make_dirs(a.stems_dir, a.spectrogram_dir, a.roll_dir)

    def on_finish(song, slot, st):
        if not int(st.finished[slot]):
            raise SystemExit('--spectrogram-dir: the walk stopped before the end of the song')
        write_song_spectrograms(st, slot, a.spectrogram_dir, name, size, percussive=song.percussive)
    p, loop, walk = _cli_walk(a, model_sr, split, want_beats, a.residual is not None, size is not None, on_finish)
    song = _record(wf, file_sr, p, loop, a.traversal, **walk)
    _write_song(a, song, model_sr, name, dict(mid=a.outfile, beats=a.beats_out, residual=a.residual,
                                              percussive=a.percussive), '--residual')
    if a.gold is not None:
        write_scores([name], [a.outfile], [a.gold])
    if roll_size is not None:
        write_rolls([name], [a.outfile], [duration], a.roll_dir, roll_size, [a.gold])


if __name__ == '__main__':
    main(sys.argv[1:])
