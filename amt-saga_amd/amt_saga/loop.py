"""The detect -> subtract loop for B windows at once, device resident.

The reference has no inference loop (main.py only trains); what it
has is the per-note generator loop of training.py:296-449 that builds the head
inputs from the residual window and subtracts the *gold* note.  This driver
composes the same steps with the *predicted* note, for B independent windows
per launch:

  per iteration (one note per window):
    C_timing  = compress_bands(mag, 20) / ref_mag_song        training.py:333-336
    onset,end = rint(timing_start(C_timing)), rint(timing_end(C_timing))
    wf        = istft(mag * ph)                               util_audio.py:94-97 (what slice_C reads)
    C_sw_pitch = slice_C(onset, dur, 8, bpt=2) / ref_C_1      training.py:340-342
    pitch     = rint(pitch_classifier(C_sw_pitch))
    C_sw_inst = slice_C(onset, dur, 8, bpt=4) / ref_C_inst    training.py:343-346
    program   = argmax(InstrumentClassifier(C_sw_inst))
    C_velocity = slice_C(..., bpt=2, nbins=36, lowest=pitch-10) / ref_C_foc   training.py:382-388
    velocity  = rint(VelocityClassifier(C_velocity))
    guess     = template bank[(program group, pitch)]         stand-in for render(), synth.py
                (guess='render': one note of the decided duration synthesised per window and
                 iteration by amt_synth_windows and STFT'd -- what the reference does per note,
                 training.py:421-431 -- instead of the fixed-duration bank row)
    mag       = relu(mag - guess * ref_mag/ref_mag(guess)) at frame `onset`   training.py:449

Everything numeric is a HIP kernel behind the C ABI; torch only holds the
buffers.  Song-level constants (ref_mag_song, ref_C_*) are computed once in
prepare(), as the reference computes them once per song (training.py:269-282).
"""
import ctypes as C

import os

import numpy as np
import torch

from . import _lib, synth
from .audio import AudioBatch, cqt_slices, cqt_table, cqt_window_max, ldf_of, midi_to_hz
from .device import empty, ptr, require_gpu, stream_ptr, to_dev, zeros
from .heads import (InstrumentClassifier, VelocityClassifier, pitch_classifier,
                    timming_classifier)

EVENT_FIELDS = ('window', 'iter', 'pitch', 'program', 'velocity', 'onset_frame', 'end_frame')
# run_songs(): one record per step and song; onset / end / offset are song frames
SONG_EVENT_FIELDS = ('song', 'step', 'kind', 'pitch', 'program', 'velocity', 'onset_frame', 'end_frame', 'offset_frame')
SONG_DETECT, SONG_SLIDE, SONG_FORCED_SLIDE, SONG_FINISHED = 0, 1, 2, 3


def song_wave_segments(lens, t_song, timing_frames, sr, positions, min_len=0):
    """Which song samples audio_complete.wf of the live window holds while nothing has been subtracted from the song,
    for every window position k = offset / half: the index arithmetic of section (util_audio.py:322-327: samples
    floor(_frames_to_seconds(frame) * sr), zero-padded by wav_end - len), slice (:355-357: int(_frames_to_seconds(
    frame) * sr) of the WINDOW's own length) and concat (:378), carried out on (source, length) pieces instead of
    samples -- Python float arithmetic on lengths, as the reference does it, so it stays on the host.
    Returns (int32 [B, positions, S, 3] pieces (first row sample, first song sample, length), row length)."""
    half = timing_frames // 2
    per_song, l_row, n_seg = [], int(min_len), 1
    for n_samples, T in zip(lens, t_song):
        def sample_of(frame):
            return int(np.floor(frame / T / sr * n_samples * sr))

        def section(first, last):
            a, e = sample_of(first), sample_of(last)
            got = max(min(e, n_samples) - min(a, n_samples), 0)
            pieces = [(a, got)] if got else []
            if got < e - a:
                pieces.append((-1, e - got))                        # the reference pads by (wav_end - len)
            return pieces

        def cut(pieces, a, e):
            out, at = [], 0
            for src, n in pieces:
                lo, hi = max(a, at), min(e, at + n)
                if hi > lo:
                    out.append((src + (lo - at) if src >= 0 else -1, hi - lo))
                at += n
            return out
        w = section(0, timing_frames)
        offset, rows = 0, []
        for _ in range(positions):
            row, at = [], 0
            for src, n in w:
                if src >= 0:
                    if row and row[-1][1] + row[-1][2] == src and row[-1][0] + row[-1][2] == at:
                        row[-1] = (row[-1][0], row[-1][1], row[-1][2] + n)
                    else:
                        row.append((at, src, n))
                at += n
            rows.append(row)
            n_seg = max(n_seg, len(row))
            l_row = max([l_row] + [d + n for d, _, n in row])
            total = sum(n for _, n in w)
            a = int(half / timing_frames / sr * total * sr)
            e = int(2 * half / timing_frames / sr * total * sr)
            offset += half
            w = cut(w, a, e) + section(offset + half, offset + 2 * half)
        per_song.append(rows)
    seg = np.zeros((len(per_song), positions, n_seg, 3), dtype=np.int32)
    for i, rows in enumerate(per_song):
        for k, row in enumerate(rows):
            for j, piece in enumerate(row):
                seg[i, k, j] = piece
    return seg, (l_row + 3) // 4 * 4


def admission_plan(finished, next_song, songs_left):
    """The admission policy of the song queue, as data: `finished` = one flag per slot (true: the slot is free),
    next_song = queue index of the next song, songs_left = how many songs the queue still holds.  Free slots in
    ascending slot order take the next songs in queue order.  Returns [(slot, song), ...]."""
    free = [b for b, f in enumerate(finished) if f]
    n = min(len(free), max(int(songs_left), 0))
    return [(free[i], int(next_song) + i) for i in range(n)]


class FramePool:
    """Host-side first-fit free list over the `frames` frames of the packed spectrogram pool: alloc(n) returns the
    first frame of the lowest free region of at least n frames (None: nothing fits now), release(first) takes a region
    back and merges it with free neighbours.  A request larger than the pool can never fit: ValueError."""

    def __init__(self, frames):
        self.frames = int(frames)
        if self.frames < 1:
            raise ValueError('run_song_queue: pool_frames must be at least 1')
        self.free = [(0, self.frames)]                             # (first, length), ascending, never adjacent
        self.used = {}

    def alloc(self, n):
        n = int(n)
        if n > self.frames:
            raise ValueError('run_song_queue: a song of %d frames is longer than the pool (%d frames)' % (n, self.frames))
        for i, (a, m) in enumerate(self.free):
            if m >= n:
                if m == n:
                    del self.free[i]
                else:
                    self.free[i] = (a + n, m - n)
                self.used[a] = n
                return a
        return None

    def release(self, first):
        n = self.used.pop(first)
        self.free.append((first, n))
        self.free.sort()
        merged = []
        for a, m in self.free:
            if merged and merged[-1][0] + merged[-1][1] == a:
                merged[-1] = (merged[-1][0], merged[-1][1] + m)
            else:
                merged.append((a, m))
        self.free = merged


class SongState:
    """What prepare_songs() builds and walk_songs() advances: the packed song spectrograms and samples, the live
    windows (`batch`), the per-song integers offset / count / finished / clean [B] and the song-level constants."""


class TranscriptionLoop:
    def __init__(self, params, heads=('timing', 'pitch', 'velocity'), iters=1, subtract=True,
                 groups=(0,), seeds=None, guess='bank', timbres=None, soundfont=None):
        self.p = params
        self.heads = tuple(heads)
        self.iters = int(iters)
        self.do_subtract = bool(subtract)
        self.groups = tuple(groups)
        if guess not in ('bank', 'render'):
            raise ValueError('Requested attribute does not exist')
        self.guess = guess
        # timbres = 'gm' (guess='render' only): every decided MIDI program is synthesised with its own timbre
        # (synth.gm_timbre_table) instead of one of the three groups
        if timbres not in (None, 'gm'):
            raise ValueError("timbres: None or 'gm'")
        if timbres == 'gm' and guess != 'render':
            raise ValueError("per-program timbres need guess='render' (the template bank holds the three groups)")
        self.timbres = timbres
        # soundfont (guess='render' only): an sf2.SoundFont or a path -- the guess is played from its samples
        # (main.py:25-29 -soundfont_path; util_audio.py:758-786), every decided MIDI program through its own preset
        if soundfont is not None and guess != 'render':
            raise ValueError("a soundfont needs guess='render'")
        if soundfont is not None and not hasattr(soundfont, 'programs'):
            from . import sf2 as _sf2
            soundfont = _sf2.SoundFont(soundfont)
        self.soundfont = soundfont
        # AMT_TIMING_STREAMS=2: timing_end on a second HIP stream under timing_start (-1 ... +3 % on a C3 step, run to run).
        # Opt-in.  Until round 4's fix two timing networks that really overlapped in time returned wrong floats at the
        # metric size: packed-FP32 vector instructions (v_pk_mul / add / fma_f32) of the transform kernels compute wrong
        # values in lanes 48-63 while a wave of ANOTHER dispatch issues v_mfma_f32_16x16x32_f16 on the same SIMD
        # (DESIGN 10.1); the network kernels are built without those instructions now (build.py NO_PK) and the full-size
        # fixtures pass on two streams (tests/test_gpu_fullsize_fixtures.py)
        self.timing_streams = int(os.environ.get('AMT_TIMING_STREAMS', '1'))
        # the subtraction on the guess's frames only (amt_subtract_span): the residual is a magnitude spectrogram (>= 0) and
        # the timing features' compress_bands pass leaves the per-frame maxima on the way; AMT_SUBTRACT_SPAN=0: whole windows
        self.span_subtract = os.environ.get('AMT_SUBTRACT_SPAN', '1') != '0'
        # diagnostic hook: when set to a list, iterate() appends one dict per iteration with copies of the heads'
        # pre-rounding outputs (what res_net.predict returns, RDCNN.py:591-597) -- the parity tests compare them
        # with the oracle's floats so that no window near a rounding tie leaves a test uncompared
        self.trace = None
        self.lib = _lib.load()
        # default seeds: synthetic timing_start / timing_end nets whose (nearly input-independent)
        # outputs satisfy onset < end, so the short-window features are not empty
        seeds = seeds or {}
        self.nets = {}
        if 'timing' in self.heads:
            self.nets['timing_start'] = timming_classifier(params, weight_seed=seeds.get('timing_start', 107))
            self.nets['timing_end'] = timming_classifier(params, weight_seed=seeds.get('timing_end', 105))
        if 'pitch' in self.heads:
            self.nets['pitch'] = pitch_classifier(params, weight_seed=seeds.get('pitch', 101))
        if 'instrument' in self.heads:
            self.nets['instrument'] = InstrumentClassifier(params, 'instrument',
                                                           weight_seed=seeds.get('instrument', 102))
        if 'velocity' in self.heads:
            self.nets['velocity'] = VelocityClassifier(params, weight_seed=seeds.get('velocity', 103))
        self._dev_ready = False

    # ---- one-time device setup (not timed: weights / tables / bank upload) ---------
    def setup_device(self, bank_waves=None):
        p = self.p
        dev = require_gpu()
        sr, lo = p.sr, p.pitch_low
        f_lo = float(midi_to_hz(lo))
        self.tab_pitch = cqt_table(sr, f_lo, p.pitch_bands, 12 * p.pitch_bins_per_tone, dev)
        self.tab_inst = cqt_table(sr, f_lo, p.instrument_bands, 12 * p.instrument_bins_per_tone, dev)
        # velocity: 36 bins at 2 bins/semitone from (pitch-10) -> one global grid from midi lo-10
        self.vel_bpt = 2
        n_vel = self.vel_bpt * (p.pitch_high - lo) + p.bins_velocity
        self.tab_vel = cqt_table(sr, float(midi_to_hz(lo - 10)), n_vel, 12 * self.vel_bpt, dev)
        # song-level normaliser grids (training.py:271-282): bpt 1, inst_bpt, 4*inst_bpt over A0..C8
        span = p.pitch_high - lo
        self.tab_ref1 = cqt_table(sr, f_lo, span * 1, 12, dev)
        self.tab_refi = cqt_table(sr, f_lo, span * p.instrument_bins_per_tone,
                                  12 * p.instrument_bins_per_tone, dev)
        self.tab_reff = cqt_table(sr, f_lo, span * p.instrument_bins_per_tone * 4,
                                  12 * p.instrument_bins_per_tone * 4, dev)
        # index of a program group inside this loop's bank
        remap = np.zeros(3, dtype=np.int32)
        for i, g in enumerate(self.groups):
            remap[g] = i
        self.prog_group = to_dev(remap[synth.prog_group_table(p.instrument_classes)], torch.int32)
        self.prog_preset = to_dev(np.arange(p.instrument_classes, dtype=np.int32)
                                  if (self.timbres == 'gm' or self.soundfont is not None)
                                  else synth.prog_group_table(p.instrument_classes), torch.int32)
        self.bank_dur = 1.0
        self.bank_len = int(round((self.bank_dur + synth.TAIL_SECONDS) * sr))
        if bank_waves is None:
            bank_waves = synth.guess_bank_waves(self.groups, p.pitch_low, p.pitch_high, sr=sr, device=dev)
        bank = AudioBatch(bank_waves, p.N, p.H).stft(with_phase=False)
        self.bank_mag, self.bank_max, self.bank_frames = bank.mag, bank.ref_max, bank.T
        self.tail_frames = int(synth.TAIL_SECONDS * sr / p.H)
        for n in self.nets.values():
            n._ensure()
        self._dev_ready = True
        return self

    # ---- small wrappers over the glue kernels -----------------------------------------
    def _round(self, y, lo, hi):
        out = empty((y.shape[0],), torch.int32)
        _lib.check(self.lib.amt_round_clamp(ptr(y), y.shape[0], y.stride(0) if y.dim() > 1 else 1,
                                            int(lo), int(hi), ptr(out), stream_ptr()))
        return out

    def _argmax(self, pr):
        out = empty((pr.shape[0],), torch.int32)
        _lib.check(self.lib.amt_argmax_rows(ptr(pr), pr.shape[0], pr.shape[1], ptr(out), stream_ptr()))
        return out

    def _resize_table(self, s, e, T, frames):
        out = empty((s.shape[0], frames), torch.int32)
        _lib.check(self.lib.amt_resize_table(ptr(s), ptr(e), s.shape[0], int(T), int(frames), ptr(out),
                                             stream_ptr()))
        return out

    # ---- per batch ------------------------------------------------------------------------
    def prepare(self, wave, refs=None):
        """STFT of the windows + the song-level constants (training.py:269-282; each window stands for its
        song): ref_mag = max |STFT|, ref_C_* = max over every bin and every frame of the normaliser's CQT
        grid.  `refs` may supply dict(ref_mag, ref_C_1, ref_C_inst, ref_C_foc) tensors [B]."""
        if not self._dev_ready:
            self.setup_device()
        p = self.p
        # the unit phase is read only by the iSTFT that feeds the CQT heads from iteration 1 on (iteration 0
        # reads the original samples): with one iteration, or without those heads, it is never stored
        # (8 F T bytes per window, 57 % of the STFT's traffic)
        odd_length = wave.shape[-1] % p.H != 0              # then even iteration 0 resynthesises (iterate())
        b = AudioBatch(wave, p.N, p.H).stft(with_phase=self.needs_phase or (self.needs_wave and odd_length))
        refs = dict(refs or {})
        if 'ref_mag' not in refs:
            refs['ref_mag'] = b.ref_max.clone()
        need_cqt = any(h in self.heads for h in ('pitch', 'instrument', 'velocity'))
        if need_cqt:
            if 'pitch' in self.heads and 'ref_C_1' not in refs:
                refs['ref_C_1'] = cqt_window_max(b.wave, self.tab_ref1, p.H)
            if 'instrument' in self.heads and 'ref_C_inst' not in refs:
                refs['ref_C_inst'] = cqt_window_max(b.wave, self.tab_refi, p.H)
            if 'velocity' in self.heads and 'ref_C_foc' not in refs:
                refs['ref_C_foc'] = cqt_window_max(b.wave, self.tab_reff, p.H)
        self.refs = refs
        return b

    def song_levels(self, song):
        """The song-level constants exactly as the reference computes them (training.py:269-282): ref_mag = the
        maximum of the whole song's |STFT|, ref_C_* = the maximum of the whole song's CQT on the respective grid.
        song: [n_samples] float32 device tensor.  Returns a dict of 0-d device tensors for the heads of this loop."""
        if not self._dev_ready:
            self.setup_device()
        p = self.p
        s = song.reshape(1, -1).to(torch.float32).contiguous()
        out = {'ref_mag': AudioBatch(s, p.N, p.H).stft(with_phase=False).ref_max[0].clone()}
        if 'pitch' in self.heads:
            out['ref_C_1'] = cqt_window_max(s, self.tab_ref1, p.H)[0]
        if 'instrument' in self.heads:
            out['ref_C_inst'] = cqt_window_max(s, self.tab_refi, p.H)[0]
        if 'velocity' in self.heads:
            out['ref_C_foc'] = cqt_window_max(s, self.tab_reff, p.H)[0]
        return out

    @property
    def needs_wave(self):
        return any(h in self.heads for h in ('pitch', 'instrument', 'velocity'))

    @property
    def needs_phase(self):
        return self.iters > 1 and self.needs_wave

    def _step(self, b, wave_fn, fmax, before_subtract=None):
        """One detect -> subtract step on the windows of `b` -- the head sequence both traversals share (iterate() for
        independent windows, run_songs() for the song walk).  wave_fn() returns what the CQT heads read as the windows'
        waveform; before_subtract(onset, end, guess_frames) runs after the guess has been selected and before it is
        subtracted (run_songs decides there which songs detect).  Returns (onset, end, pitch, program, velocity)."""
        p = self.p
        B, T = b.mag.shape[0], b.mag.shape[1]
        st = stream_ptr()
        onset = end = pitch = program = velocity = None
        tr = {}
        if 'timing' in self.heads:
            ct = b.compress_bands(p.timing_bands, self.refs['ref_mag'], p.timing_frames, fmax=fmax)
            if self.timing_streams == 2:
                # the two timing networks read the same features and are independent: timing_end on a second stream
                # fills the tails of timing_start's small-image launches (5 x 8 and 10 x 64 layers)
                cur = torch.cuda.current_stream()
                if getattr(self, '_side_stream', None) is None:
                    self._side_stream = torch.cuda.Stream()
                side = self._side_stream
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    te = self.nets['timing_end'].classify(ct)
                ts = self.nets['timing_start'].classify(ct)
                cur.wait_stream(side)
                te.record_stream(cur)
            else:
                ts = self.nets['timing_start'].classify(ct)
                te = self.nets['timing_end'].classify(ct)
            onset = self._round(ts, 0, T - 1)
            end = self._round(te, 0, T)
            tr['timing_start'], tr['timing_end'] = ts, te
        else:
            onset = zeros((B,), torch.int32)
            end = torch.full((B,), p.pitch_frames, dtype=torch.int32, device=onset.device)
        src = self._resize_table(onset, end, T, p.pitch_frames)
        wave_r = wave_fn() if self.needs_wave else None
        if 'pitch' in self.heads:
            cp = cqt_slices(wave_r, src, self.tab_pitch, p.pitch_bands, p.H, ref=self.refs['ref_C_1'])
            tr['pitch'] = self.nets['pitch'].classify(cp)
            pitch = self._round(tr['pitch'], p.pitch_low, p.pitch_high)
        else:
            pitch = torch.full((B,), 60, dtype=torch.int32, device=onset.device)
        if 'instrument' in self.heads:
            ci = cqt_slices(wave_r, src, self.tab_inst, p.instrument_bands, p.H, ref=self.refs['ref_C_inst'])
            tr['instrument'] = self.nets['instrument'].classify(ci)
            program = self._argmax(tr['instrument'])
        if 'velocity' in self.heads:
            bin0 = empty((B,), torch.int32)
            _lib.check(self.lib.amt_affine_i32(ptr(pitch), B, self.vel_bpt, -self.vel_bpt * p.pitch_low,
                                               ptr(bin0), st))
            cv = cqt_slices(wave_r, src, self.tab_vel, p.bins_velocity, p.H, bin0=bin0,
                            ref=self.refs['ref_C_foc'])
            tr['velocity'] = self.nets['velocity'].classify(cv)
            velocity = self._round(tr['velocity'], 1, 127)
        gidx = gfr = None
        if self.do_subtract:
            gidx = empty((B,), torch.int32)
            gfr = empty((B,), torch.int32)
            _lib.check(self.lib.amt_note_select(
                ptr(program), ptr(pitch), ptr(onset), ptr(end), ptr(self.prog_group),
                self.prog_group.shape[0], B, p.pitch_low, p.pitch_high - p.pitch_low + 1,
                self.tail_frames, self.bank_frames, ptr(gidx), ptr(gfr), st))
        if before_subtract is not None:
            before_subtract(onset, end, gfr)
        if self.do_subtract:
            if self.guess == 'bank':
                b.subtract(self.bank_mag, self.bank_max, gidx, gfr, onset, normalize=True, relu=True,
                           span=self.span_subtract)
            else:
                notes = empty((B, 1, 5))
                _lib.check(self.lib.amt_guess_notes(
                    ptr(program), ptr(pitch), ptr(velocity), ptr(onset), ptr(end), ptr(self.prog_preset),
                    self.prog_preset.shape[0], B, p.H / p.sr, self.bank_dur, 100.0, ptr(notes), st))
                if self.soundfont is not None:
                    from . import sf2 as _sf2
                    gw = _sf2.render_windows_device(notes, self.bank_len, self.soundfont, p.sr)
                else:
                    gw = synth.render_windows_device(notes, self.bank_len, p.sr, timbres=self.timbres)
                g = AudioBatch(gw, p.N, p.H).stft(with_phase=False)
                b.subtract(g.mag, g.ref_max, None, gfr, onset, normalize=True, relu=True, span=self.span_subtract)
        if self.trace is not None:
            self.trace.append({k: v.clone() for k, v in tr.items()})
        return onset, end, pitch, program, velocity

    def iterate(self, b, it, events, window0=0):
        p = self.p
        T = b.mag.shape[1]

        def wave_fn():
            # iteration 0 reads the original samples, later ones the iSTFT of the residual (util_audio.py:94-97)
            if it == 0 and b.wave is not None and b.wave.shape[1] == p.H * (T - 1):
                return b.wave
            return b.istft()
        onset, end, pitch, program, velocity = self._step(b, wave_fn, fmax=self.span_subtract)
        _lib.check(self.lib.amt_pack_events(b.mag.shape[0], int(window0), int(it), ptr(pitch), ptr(program),
                                            ptr(velocity), ptr(onset), ptr(end), ptr(events[it]), stream_ptr()))

    def run(self, wave, window0=0, refs=None):
        """All iterations for one batch.  Returns (events [iters, B, 7] int32 device,
        the AudioBatch holding the residual)."""
        b = self.prepare(wave, refs)
        events = empty((self.iters, b.mag.shape[0], len(EVENT_FIELDS)), torch.int32)
        for it in range(self.iters):
            self.iterate(b, it, events, window0)
        return events, b

    def prepare_songs(self, songs, refs=None, spectra=None):
        """Set-up of the song walk, once per batch of songs: one STFT per song (training.py:265-269) packed frame-major
        into one buffer, the song-level constants (:269-282), the first window of every song (section(0, None,
        timing_frames), :284), the raw-sample table of amt_song_wave and the per-song integers.
        songs: sequence of 1-d float32 waveforms of at least one hop.  refs: optional dict(ref_mag, ref_C_1, ref_C_inst,
        ref_C_foc) of [B] tensors instead of the constants computed here.  spectra: optional AudioBatch that already
        holds the songs' STFT (mag, ph, ref_max; songs of equal length, one per row) -- it is read, not changed.
        Returns the state walk_songs() advances."""
        if not self._dev_ready:
            self.setup_device()
        p = self.p
        songs = list(songs)
        if not songs:
            raise ValueError('run_songs: no songs given')
        if 'timing' not in self.heads or not self.do_subtract:
            raise ValueError('run_songs: the walk needs the timing heads and the subtraction')
        tf = p.timing_frames
        if tf % 2:
            raise ValueError('Invalid Input shape. run_songs needs an even timing_frames. Got: %d' % tf)
        half, B = tf // 2, len(songs)
        waves = [to_dev(s).reshape(-1) for s in songs]
        for w in waves:
            if w.numel() < p.H:
                raise ValueError('Invalid Input shape. Expected: a song of at least one hop (%d samples) . Got: %d'
                                 % (p.H, w.numel()))
        lens = [int(w.numel()) for w in waves]
        t_song = [1 + n // p.H for n in lens]
        fbase = np.concatenate(([0], np.cumsum(t_song)))
        sbase = np.concatenate(([0], np.cumsum(lens)))
        ldf = ldf_of(p.N)
        s_mag, s_ph = empty((int(fbase[-1]), ldf)), empty((int(fbase[-1]), ldf, 2))
        b = AudioBatch(None, p.N, p.H)
        b.mag, b.ph, b.ref_max = zeros((B, tf, ldf)), zeros((B, tf, ldf, 2)), empty((B,))
        own = {}
        normalisers = (('pitch', 'ref_C_1', self.tab_ref1), ('instrument', 'ref_C_inst', self.tab_refi),
                       ('velocity', 'ref_C_foc', self.tab_reff))
        for i, w in enumerate(waves):
            if spectra is not None:
                mag, ph, ref_max = spectra.mag[i], spectra.ph[i], spectra.ref_max[i]
                if mag.shape[0] != t_song[i]:
                    raise ValueError('Invalid Input shape. Expected: %d frames . Got: %d' % (t_song[i], mag.shape[0]))
            else:
                a = AudioBatch(w[None, :], p.N, p.H).stft(with_phase=True)
                mag, ph, ref_max = a.mag[0], a.ph[0], a.ref_max[0]
            f0, n0 = int(fbase[i]), min(tf, t_song[i])
            s_mag[f0:f0 + t_song[i]], s_ph[f0:f0 + t_song[i]] = mag, ph
            b.mag[i, :n0], b.ph[i, :n0] = mag[:n0], ph[:n0]
            if refs is None:
                own.setdefault('ref_mag', []).append(ref_max.clone())
                for head, key, tab in normalisers:
                    if head in self.heads:
                        own.setdefault(key, []).append(cqt_window_max(w[None, :], tab, p.H)[0])
        st = SongState()
        st.refs = {k: torch.stack(v).contiguous() for k, v in own.items()} if refs is None else \
            {k: to_dev(v).reshape(B).contiguous() for k, v in refs.items()}
        st.batch, st.s_mag, st.s_ph, st.samples = b, s_mag, s_ph, torch.cat(waves)
        st.positions = max(-(-t // half) for t in t_song)            # window positions of the longest song
        seg, st.l_row = song_wave_segments(lens, t_song, tf, p.sr, st.positions, min_len=tf * p.H)
        st.seg = to_dev(seg, torch.int32)
        st.t_song = to_dev(np.asarray(t_song, dtype=np.int32), torch.int32)
        st.frame_base = to_dev(fbase[:-1].astype(np.int64), torch.int64)
        st.sample_base = to_dev(sbase[:-1].astype(np.int64), torch.int64)
        st.offset, st.count, st.finished = (zeros((B,), torch.int32) for _ in range(3))
        st.clean = torch.ones((B,), dtype=torch.int32, device=st.offset.device)
        st.slide, st.detect, st.kind = (empty((B,), torch.int32) for _ in range(3))
        st.wave = empty((B, st.l_row))
        st.steps = 0
        return st

    def _song_step_fns(self, st, max_notes, silence):
        """What _step() needs from the song walk (walk_songs and the song queue share it): wave_fn() = the windows'
        waveform for the CQT heads, decide(onset, end, guess_frames) = the step's slide / detect masks."""
        p, b, sp = self.p, st.batch, stream_ptr()
        tf = p.timing_frames
        half, B, ldf = tf // 2, b.mag.shape[0], b.mag.shape[2]
        self.refs = st.refs
        l_istft = p.H * (tf - 1)

        def wave_fn():
            # util_audio.py:94-97 for windows that had a subtraction (their _wf is None: the mag setter cleared it, slice
            # and concat keep None); the raw samples section / slice / concat carry along for the others
            _lib.check(self.lib.amt_istft(b.plan, ptr(b.mag), ptr(b.ph), B, tf, ldf, tf * ldf, ptr(st.wave), st.l_row,
                                          sp))
            _lib.check(self.lib.amt_song_wave(ptr(st.samples), ptr(st.sample_base), ptr(st.seg), B, int(st.seg.shape[1]),
                                              int(st.seg.shape[2]), ptr(st.offset), half, ptr(st.clean),
                                              ptr(st.finished), ptr(st.wave), st.l_row, st.l_row, l_istft, sp))
            return st.wave

        def decide(onset, end, gfr):
            wmax = empty((B,))
            _lib.check(self.lib.amt_song_decide(ptr(onset), ptr(b._fmax[0]), B, tf, ptr(st.refs['ref_mag']),
                                                float(silence), half, int(max_notes), ptr(st.finished), ptr(st.count),
                                                ptr(st.clean), ptr(st.slide), ptr(st.detect), ptr(st.kind), ptr(gfr),
                                                ptr(wmax), sp))
            b.ref_max = wmax                                         # np.max(audio_w.mag) at the subtraction (:170-174)

        return wave_fn, decide

    def walk_songs(self, st, max_notes=8, silence=1e-3, poll=16, song0=0, max_steps=None):
        """The steps of the song walk on a state from prepare_songs(); see run_songs().  max_steps: stop after that many
        steps even if songs are unfinished (the state can be inspected, not resumed).  Returns events [steps, B, 9] int32
        (device)."""
        if int(max_notes) < 1:
            raise ValueError('run_songs: max_notes must be at least 1')
        if not float(silence) >= 0.0:
            raise ValueError('run_songs: silence must be >= 0')
        p, b, sp = self.p, st.batch, stream_ptr()
        tf = p.timing_frames
        half, B, ldf = tf // 2, b.mag.shape[0], b.mag.shape[2]
        wave_fn, decide = self._song_step_fns(st, max_notes, silence)
        st.bound = st.positions * (int(max_notes) + 1)
        if max_steps is not None:
            st.bound = min(st.bound, int(max_steps))
        events = empty((st.bound, B, len(SONG_EVENT_FIELDS)), torch.int32)
        steps = 0
        while steps < st.bound:
            onset, end, pitch, program, velocity = self._step(b, wave_fn, fmax=True, before_subtract=decide)
            _lib.check(self.lib.amt_song_pack_events(B, int(song0), steps, ptr(st.kind), ptr(pitch), ptr(program),
                                                     ptr(velocity), ptr(onset), ptr(end), ptr(st.offset),
                                                     ptr(events[steps]), sp))
            _lib.check(self.lib.amt_song_slide(ptr(b.mag), ptr(b.ph), B, tf, ldf, tf * ldf, ptr(st.s_mag), ptr(st.s_ph),
                                               ptr(st.frame_base), ptr(st.t_song), ptr(st.slide), ptr(st.offset),
                                               ptr(st.count), ptr(st.finished), sp))
            b._fmax = None                                           # the slid windows' per-frame maxima are stale
            steps += 1
            if steps % max(int(poll), 1) == 0 and int(st.finished.sum()) == B:
                break
        st.steps = steps
        return events[:steps]

    def run_songs(self, songs, max_notes=8, silence=1e-3, poll=16, song0=0, refs=None):
        """The reference's own traversal (training.py:284, :296-328) with the predicted note where it has the gold
        note, for B songs at once: ONE live window of timing_frames frames per song, cut from the song's spectrogram
        (one STFT per song) and, whenever the predicted onset lies in its second half, slid by half a window with
        the residual of every subtraction kept.  prepare_songs() + walk_songs().

        songs: sequence of 1-d float32 waveforms (device tensors or arrays) of any lengths >= one hop.
        Per step and unfinished song (amt_song_decide): onset >= half -> slide; else count == max_notes or
        max(window) <= silence * ref_mag(song) -> forced slide; else detect (remaining heads, guess, subtraction as in
        run(); count += 1).  A slide moves the second half of the window to the first, appends the next half window
        of song frames (zeros past the end), offset += half, count = 0; the song is finished once offset >= its frames.
        max_notes and silence are BUILD-DEFINED: they stand for the reference's "no gold note left in this window"
        (training.py:313-314), which a transcriber cannot know.

        Nothing is read back per step: decisions are device masks; the host polls the finished songs every `poll`
        steps and stops at the bound positions * (max_notes + 1) steps at the latest.  Finished and sliding songs
        keep their slot (their heads are computed and discarded; the batch is NOT compacted): batch songs of similar
        length, or hand a collection to run_song_queue(), which refills finished slots.  Requires the timing heads and an even timing_frames.

        Returns (events [steps, B, 9] int32 device, SONG_EVENT_FIELDS; state): state.batch is the AudioBatch holding
        every song's last window (residual magnitudes, unit phases, maxima), state.offset / count / finished /
        t_song the per-song integers, state.refs the song-level constants."""
        if int(max_notes) < 1:
            raise ValueError('run_songs: max_notes must be at least 1')
        st = self.prepare_songs(songs, refs=refs)
        return self.walk_songs(st, max_notes=max_notes, silence=silence, poll=poll, song0=song0), st

    def iter_song_queue(self, songs, slots, max_notes=8, silence=1e-3, poll=16, pool_frames=None, on_finish=None):
        """Continuous batching of the song walk: any number of songs of any lengths walked through `slots` live windows,
        a finished slot handed to the next song of the queue (the reference's unit of work is a dataset of songs, one
        song after the other per worker, training.py:623-634).  The step is run_songs' step, unchanged; a song's records
        are those run_songs([song]) gives for it alone, whatever shares the batch with it.

        songs: a sequence or an iterator of 1-d float32 waveforms (arrays or tensors), consumed lazily -- only the
        songs in a slot, and up to `slots` waiting ones, are held.  Yields (song_index, events [k, 9] int32 host array)
        as each song finishes: the song's own records in step order (kinds DETECT / SLIDE / FORCED_SLIDE), `step`
        counted from 0 within the song, `song` = its index in the queue.

        Admission happens where the walk polls anyway (before the first step, then every `poll` steps): the host reads
        `finished` and the last `poll` steps' records in one pinned copy, yields the finished songs, and the free slots,
        in ascending slot order, take the next songs in queue order (admission_plan).  For the admitted songs: ONE
        ragged STFT launch (amt_stft_mag_ragged) into their regions of the spectrogram pool, the song-level CQT
        normalisers per song (cqt_window_max), their raw-sample tables, ONE amt_song_admit.
        Pool: `pool_frames` frames of magnitudes + phases with pool_frames x hop samples beside them; a first-fit free
        list (FramePool) hands a song 1 + samples // hop frames at admission and takes them back when the song has
        been yielded.  A song longer than the pool is a ValueError when it is met; a song that does not fit NOW waits,
        and the songs behind it wait with it (queue order is kept) while its slot idles -- with no song active the pool
        is empty and the next song fits, so the walk cannot stall.  Default pool_frames: slots x the frames of the
        longest of the first `slots` songs of the queue.
        The per-slot tables that run_songs sizes from its whole batch (window positions and pieces of the raw-sample
        table, the row length of the CQT heads' waveform) grow at an admission that needs more; no record depends on them.
        ONE compute stream: the admission's STFT and normaliser kernels run on the stream of the networks, between two
        steps.  They are built with packed-FP32 instructions and must not overlap the networks' MFMA kernels on a side
        stream.
        The walk ends when the queue is empty and every slot is finished; it raises RuntimeError past the sum over the
        admitted songs of positions x (max_notes + 1) steps, each rounded up to `poll` (a song is admitted and found
        finished at poll points only, and at every step at least one admitted song is live).
        on_finish(song_index, slot, state): called when a song is found finished, before its slot and region are given
        away -- state.batch.mag[slot] is then the residual of the song's last window.
        Counters of the walk, updated at every poll point: state.stats, also left in self.queue_stats (the LAST queue
        started on this loop; a second queue replaces it) -- dict(steps, songs, admissions, waits = admissions that
        stopped at a song without a free region, bound = the step cap so far, slot_steps = step slots per kind
        [detect, slide, forced slide, idle])."""
        if int(slots) < 1:
            raise ValueError('run_song_queue: slots must be at least 1')
        if int(max_notes) < 1:
            raise ValueError('run_songs: max_notes must be at least 1')
        if not float(silence) >= 0.0:
            raise ValueError('run_songs: silence must be >= 0')
        if 'timing' not in self.heads or not self.do_subtract:
            raise ValueError('run_songs: the walk needs the timing heads and the subtraction')
        tf = self.p.timing_frames
        if tf % 2:
            raise ValueError('Invalid Input shape. run_songs needs an even timing_frames. Got: %d' % tf)
        if pool_frames is not None and int(pool_frames) < 1:
            raise ValueError('run_song_queue: pool_frames must be at least 1')
        if not self._dev_ready:
            self.setup_device()
        p, B, poll = self.p, int(slots), max(int(poll), 1)
        it, ahead, pulled = iter(songs), [], [0]

        def pull(n):
            """Songs waiting for a slot: up to n, validated as run_songs validates them."""
            while len(ahead) < n:
                w = next(it, None)
                if w is None:
                    break
                w = to_dev(w).reshape(-1)
                if w.numel() < p.H:
                    raise ValueError('Invalid Input shape. Expected: a song of at least one hop (%d samples) . Got: %d'
                                     % (p.H, w.numel()))
                if w.numel() <= p.N // 2:                          # what amt_stft_mag answers for it in run_songs
                    raise ValueError('Invalid Input shape. Expected: a song of more than n_fft / 2 = %d samples '
                                     '(reflect padding) . Got: %d' % (p.N // 2, w.numel()))
                ahead.append((pulled[0], w))
                pulled[0] += 1

        pull(B)
        if not ahead:
            raise ValueError('run_songs: no songs given')
        if pool_frames is None:
            pool_frames = B * max(1 + w.numel() // p.H for _, w in ahead)
        return self._walk_song_queue(pull, ahead, pulled, B, int(max_notes), float(silence), poll, int(pool_frames),
                                     on_finish)

    def _walk_song_queue(self, pull, ahead, pulled, B, max_notes, silence, poll, pool_frames, on_finish):
        p, sp = self.p, stream_ptr()
        tf, ldf, dev = p.timing_frames, ldf_of(p.N), require_gpu()
        half = tf // 2
        st = SongState()
        st.pool = FramePool(pool_frames)
        st.s_mag, st.s_ph = empty((pool_frames, ldf)), empty((pool_frames, ldf, 2))
        st.samples = empty((pool_frames * p.H,))                   # a song of T frames has fewer than T hops of samples
        b = AudioBatch(None, p.N, p.H)
        b.mag, b.ph, b.ref_max = zeros((B, tf, ldf)), zeros((B, tf, ldf, 2)), zeros((B,))
        ref_keys = ['ref_mag'] + [k for h, k in (('pitch', 'ref_C_1'), ('instrument', 'ref_C_inst'),
                                                 ('velocity', 'ref_C_foc')) if h in self.heads]
        tabs = {'ref_C_1': self.tab_ref1, 'ref_C_inst': self.tab_refi, 'ref_C_foc': self.tab_reff}
        st.refs = {k: torch.ones((B,), dtype=torch.float32, device=dev) for k in ref_keys}   # idle slots divide by 1
        st.batch = b
        st.t_song, st.offset, st.count = (zeros((B,), torch.int32) for _ in range(3))
        st.frame_base, st.sample_base = zeros((B,), torch.int64), zeros((B,), torch.int64)
        st.finished, st.clean = (torch.ones((B,), dtype=torch.int32, device=dev) for _ in range(2))
        st.slot_song = torch.full((B,), -1, dtype=torch.int32, device=dev)
        st.slide, st.detect, st.kind = (empty((B,), torch.int32) for _ in range(3))
        st.seg = zeros((B, 1, 1, 3), torch.int32)
        st.l_row = (tf * p.H + 3) // 4 * 4
        st.wave = empty((B, st.l_row))
        st.steps = 0
        wave_fn, decide = self._song_step_fns(st, max_notes, silence)
        chunk = empty((poll, B, len(SONG_EVENT_FIELDS)), torch.int32)
        host_chunk = torch.empty(tuple(chunk.shape), dtype=torch.int32, pin_memory=True)
        host_fin = torch.empty((B,), dtype=torch.int32, pin_memory=True)
        slot_song, region, records = [-1] * B, [None] * B, {}
        stats = self.queue_stats = st.stats = dict(steps=0, songs=0, admissions=0, waits=0, bound=0,
                                        slot_steps=[0, 0, 0, 0])   # per kind: detect, slide, forced slide, idle

        def admit():
            pull(sum(s < 0 for s in slot_song))
            plan = admission_plan([s < 0 for s in slot_song], ahead[0][0] if ahead else pulled[0], len(ahead))
            new = []
            for slot, idx in plan:
                w = ahead[0][1]
                f0 = st.pool.alloc(1 + w.numel() // p.H)
                if f0 is None:                                     # waits for a region; the songs behind it wait too
                    stats['waits'] += 1
                    break
                ahead.pop(0)
                new.append((slot, idx, w, f0))
            if not new:
                return
            n = len(new)
            lens = [int(w.numel()) for _, _, w, _ in new]
            t_song = [1 + L // p.H for L in lens]
            fbase = np.asarray([f0 for _, _, _, f0 in new], np.int64)
            for (_, _, w, f0), L in zip(new, lens):
                st.samples[f0 * p.H:f0 * p.H + L].copy_(w)
            d_fb, d_sb = to_dev(fbase, torch.int64), to_dev(fbase * p.H, torch.int64)
            d_len = to_dev(np.asarray(lens, np.int32), torch.int32)
            new_refs = {'ref_mag': empty((n,))}
            _lib.check(self.lib.amt_stft_mag_ragged(b.plan, ptr(st.samples), ptr(d_sb), ptr(d_len), n, max(lens),
                                                    st.samples.numel(), sum(lens), ptr(st.s_mag), ptr(st.s_ph),
                                                    ptr(new_refs['ref_mag']), ptr(d_fb), pool_frames, ldf, sp))
            for k in ref_keys[1:]:
                new_refs[k] = torch.cat([cqt_window_max(st.samples[f0 * p.H:f0 * p.H + L][None, :], tabs[k], p.H)
                                         for (_, _, _, f0), L in zip(new, lens)]).contiguous()
            seg, l_row = song_wave_segments(lens, t_song, tf, p.sr, max(-(-t // half) for t in t_song),
                                            min_len=tf * p.H)
            K, S = max(seg.shape[1], st.seg.shape[1]), max(seg.shape[2], st.seg.shape[2])
            if (K, S) != tuple(st.seg.shape[1:3]):                 # the per-slot piece table grows, its rows are kept
                grown = zeros((B, K, S, 3), torch.int32)
                grown[:, :st.seg.shape[1], :st.seg.shape[2]] = st.seg
                st.seg = grown
            if l_row > st.l_row:
                st.l_row, st.wave = l_row, empty((B, l_row))
            seg_new = np.zeros((n, K, S, 3), np.int32)
            seg_new[:, :seg.shape[1], :seg.shape[2]] = seg
            mask = np.zeros(B, np.int32)
            for j, (slot, idx, _, f0) in enumerate(new):
                mask[slot] = 1 + j
                slot_song[slot], region[slot], records[idx] = idx, f0, []
                stats['bound'] += -(-(-(-t_song[j] // half) * (max_notes + 1)) // poll) * poll
            d_mask, d_seg = to_dev(mask, torch.int32), to_dev(seg_new, torch.int32)
            d_ts, d_song = to_dev(np.asarray(t_song, np.int32), torch.int32), \
                to_dev(np.asarray([idx for _, idx, _, _ in new], np.int32), torch.int32)
            a = _lib.song_admit_args(
                w_mag=b.mag, w_ph=b.ph, s_mag=st.s_mag, s_ph=st.s_ph, admit=d_mask, new_frame_base=d_fb, new_t_song=d_ts,
                new_sample_base=d_sb, new_song=d_song, new_seg=d_seg, new_ref=[new_refs[k] for k in ref_keys],
                frame_base=st.frame_base, t_song=st.t_song, sample_base=st.sample_base, slot_song=st.slot_song,
                seg=st.seg, ref=[st.refs[k] for k in ref_keys], offset=st.offset, count=st.count,
                finished=st.finished, clean=st.clean, w_stride=tf * ldf, B=B, n_new=n, T=tf, ldf=ldf, K=K, S=S)
            _lib.check(self.lib.amt_song_admit(C.byref(a), sp))
            b._fmax = None                                         # the admitted windows' per-frame maxima are stale
            stats['admissions'] += 1
            stats['songs'] += n

        admit()
        while any(s >= 0 for s in slot_song):
            for r in range(poll):
                onset, end, pitch, program, velocity = self._step(b, wave_fn, fmax=True, before_subtract=decide)
                _lib.check(self.lib.amt_song_pack_events_slots(B, ptr(st.slot_song), st.steps, ptr(st.kind), ptr(pitch),
                                                               ptr(program), ptr(velocity), ptr(onset), ptr(end),
                                                               ptr(st.offset), ptr(chunk[r]), sp))
                _lib.check(self.lib.amt_song_slide(ptr(b.mag), ptr(b.ph), B, tf, ldf, tf * ldf, ptr(st.s_mag),
                                                   ptr(st.s_ph), ptr(st.frame_base), ptr(st.t_song), ptr(st.slide),
                                                   ptr(st.offset), ptr(st.count), ptr(st.finished), sp))
                b._fmax = None
                st.steps += 1
            host_chunk.copy_(chunk, non_blocking=True)
            host_fin.copy_(st.finished, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            ev = host_chunk.numpy()
            stats['steps'] = st.steps
            kinds = np.bincount(ev[:, :, 2].ravel(), minlength=4)
            for k in range(4):
                stats['slot_steps'][k] += int(kinds[k])
            done = []
            for slot, idx in enumerate(slot_song):
                if idx < 0:
                    continue
                rows = ev[:, slot, :]
                records[idx].append(rows[rows[:, 2] != SONG_FINISHED].copy())
                if host_fin[slot]:
                    done.append((slot, idx))
            for slot, idx in done:
                if on_finish is not None:
                    on_finish(idx, slot, st)
                out = np.concatenate(records.pop(idx))
                out[:, 1] = np.arange(len(out))
                st.pool.release(region[slot])
                slot_song[slot], region[slot] = -1, None
                yield idx, out
            admit()
            if st.steps > stats['bound']:
                raise RuntimeError('run_song_queue: %d steps, past the bound of the admitted songs (%d)'
                                   % (st.steps, stats['bound']))

    def run_song_queue(self, songs, slots, max_notes=8, silence=1e-3, poll=16, pool_frames=None, on_finish=None):
        """iter_song_queue() run to its end.  Returns the list of the songs' records, events [k, 9] int32 host arrays,
        in queue order."""
        out = {}
        for idx, ev in self.iter_song_queue(songs, slots, max_notes=max_notes, silence=silence, poll=poll,
                                            pool_frames=pool_frames, on_finish=on_finish):
            out[idx] = ev
        return [out[i] for i in range(len(out))]

    def run_stream(self, host_batches, refs=None, window0=0):
        """run() over a sequence of HOST batches with the host -> HBM copy of batch i+1 overlapped with the
        compute of batch i: two device staging buffers, a copy stream, and events in both directions (the
        compute waits for its batch's copy; a copy waits until the compute that last read its buffer is done).
        host_batches: iterable of float32 [B, L] CPU tensors or arrays (pinned memory makes the copy
        asynchronous; pageable memory still works, serialised by the driver).  `refs`: dict of [B] device
        tensors shared by all batches, or a callable batch_index -> dict, or None (prepare() computes them).
        Yields (events, AudioBatch) per batch, in order; the AudioBatch's `wave` is the staging buffer and is
        overwritten two batches later."""
        if not self._dev_ready:
            self.setup_device()
        cur = torch.cuda.current_stream()
        if getattr(self, '_copy_stream', None) is None:
            self._copy_stream = torch.cuda.Stream()
        cs = self._copy_stream
        bufs = [None, None]
        ready = [torch.cuda.Event(), torch.cuda.Event()]
        free = [torch.cuda.Event(), torch.cuda.Event()]

        def issue(i, host):
            h = host if torch.is_tensor(host) else torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32))
            s = i & 1
            if bufs[s] is None or bufs[s].shape != h.shape:
                bufs[s] = empty(tuple(h.shape))
                cs.wait_stream(cur)                  # the allocation (and whatever freed that memory) is ordered
            with torch.cuda.stream(cs):
                cs.wait_event(free[s])               # no-op until the event has been recorded once
                bufs[s].copy_(h, non_blocking=True)
                ready[s].record(cs)

        it = iter(host_batches)
        nxt = next(it, None)
        if nxt is None:
            return
        issue(0, nxt)
        i = 0
        while nxt is not None:
            nxt = next(it, None)
            if nxt is not None:
                issue(i + 1, nxt)                    # in flight while batch i computes
            s = i & 1
            cur.wait_event(ready[s])
            r = refs(i) if callable(refs) else refs
            events, b = self.run(bufs[s], window0=window0, refs=r)
            free[s].record(cur)
            window0 += bufs[s].shape[0]
            yield events, b
            events = b = None                        # let the allocator reuse the batch's blocks
            i += 1

    def flops_per_window_iter(self):
        return sum(n.flops_per_window for n in self.nets.values())
