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
                (instrument_model=: any of the reference's ten instrument models, INSTRUMENT_MODELS below -- its towers
                 read the focused FFT bands, their log10 and phase, training.py:347-363, from one amt_note_features
                 launch, or the focused CQT slices, :365-380; note_features() composes them)
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
import os

import numpy as np
import torch

from . import _lib, song_walk, synth
from .audio import AudioBatch, cqt_slices, cqt_table, cqt_window_max, midi_to_hz, tone_bin_table
from .device import empty, ptr, require_gpu, stream_ptr, to_dev, zeros
from .heads import (InstrumentClassifier, VelocityClassifier, pitch_classifier,
                    timming_classifier)
# the song walk (run_songs, run_song_queue) lives in song_walk.py; its names stay importable from here
from .song_walk import (SONG_DETECT, SONG_EVENT_FIELDS, SONG_FINISHED, SONG_FORCED_SLIDE, SONG_SLIDE,  # noqa: F401
                        FramePool, SongState, admission_plan, song_wave_segments)  # noqa: F401

EVENT_FIELDS = ('window', 'iter', 'pitch', 'program', 'velocity', 'onset_frame', 'end_frame')

# The reference's ten instrument models (training.py:466-477): name -> (InstrumentClassifier variant, as gen_model
# builds it, training.py:76-98; the recipe arrays its towers read, in tower order, as thread_training feeds them).
# The arrays are those of the feature recipe, training.py:343-380:
#   C_sw_inst                  slice_C at instrument_bins_per_tone from A0                     / ref_C_inst
#   C_sw_inst_foc(_const)      slice_C at 4 x that from the decided pitch (from C4)            / ref_C_foc
#   F_sw_inst_foc(_const)      the FFT band from midi_tone_to_FFT(pitch) (of C4), mag          / ref_mag
#   F_sw_inst_foc(_const)_log10    the same band, log10(1000 mag + 1)                          / its maximum
#   ph                         the phase angle of the pitch's band, (angle + 3.15) / 6.3
INSTRUMENT_MODELS = {
    'instrument': (InstrumentClassifier.INSTRUMENT, ('C_sw_inst',)),
    'instrument_focused_lin': (InstrumentClassifier.INSTRUMENT_FOCUSED, ('F_sw_inst_foc',)),
    'instrument_focused_lin_log10': (InstrumentClassifier.INSTRUMENT_FOCUSED, ('F_sw_inst_foc_log10',)),
    'instrument_focused_const_lin': (InstrumentClassifier.INSTRUMENT_FOCUSED_CONST, ('F_sw_inst_foc_const',)),
    'instrument_focused_const_lin_log10': (InstrumentClassifier.INSTRUMENT_FOCUSED_CONST,
                                           ('F_sw_inst_foc_const_log10',)),
    'instrument_dual_lin': (InstrumentClassifier.INSTRUMENT_DUAL, ('C_sw_inst', 'F_sw_inst_foc')),
    'instrument_dual_lin_phase': (InstrumentClassifier.INSTRUMENT_DUAL, ('F_sw_inst_foc', 'ph')),
    'instrument_focused': (InstrumentClassifier.INSTRUMENT_FOCUSED, ('C_sw_inst_foc',)),
    'instrument_focused_const': (InstrumentClassifier.INSTRUMENT_FOCUSED_CONST, ('C_sw_inst_foc_const',)),
    'instrument_dual': (InstrumentClassifier.INSTRUMENT_DUAL, ('C_sw_inst', 'C_sw_inst_foc')),
}
CONST_TONE = 60        # the _const models' fixed window position: C4 (training.py:289-290, :378)
# recipe array -> the output of amt_note_features it is, for the decided pitch and for the constant tone
_FFT_FEATURES = {'F_sw_inst_foc': 'lin', 'F_sw_inst_foc_log10': 'log10', 'ph': 'phase'}
_FFT_FEATURES_CONST = {'F_sw_inst_foc_const': 'lin', 'F_sw_inst_foc_const_log10': 'log10'}
FEATURE_NAMES = ('C_sw_inst', 'C_sw_inst_foc', 'C_sw_inst_foc_const') + tuple(_FFT_FEATURES) + tuple(_FFT_FEATURES_CONST)


class TranscriptionLoop:
    def __init__(self, params, heads=('timing', 'pitch', 'velocity'), iters=1, subtract=True,
                 groups=(0,), seeds=None, guess='bank', timbres=None, soundfont=None, instrument_model='instrument'):
        if instrument_model not in INSTRUMENT_MODELS:
            raise ValueError('Invalid Variant Selected')
        self.instrument_model = instrument_model
        # the recipe arrays the instrument towers read; none without the instrument head
        self.instrument_inputs = INSTRUMENT_MODELS[instrument_model][1] if 'instrument' in heads else ()
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
            self.nets['instrument'] = InstrumentClassifier(params, INSTRUMENT_MODELS[instrument_model][0],
                                                           prefix=instrument_model,
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
        # the focused instrument towers: instrument_bands bins at 4 x instrument_bins_per_tone from the decided pitch
        # (training.py:365-380) -> one global grid from pitch_low, as the velocity grid above; built for the models
        # that read it
        self.foc_bpt = 4 * p.instrument_bins_per_tone
        self.tab_foc = None
        if any(k.startswith('C_sw_inst_foc') for k in self.instrument_inputs):
            self.tab_foc = cqt_table(sr, f_lo, self.foc_bpt * span + p.instrument_bands, 12 * self.foc_bpt, dev)
        # midi_tone_to_FFT (util_audio.py:278-284) of every tone the pitch head can decide: what amt_note_features
        # indexes with the step's pitches
        self.tone_bin = to_dev(tone_bin_table(sr, p.N, lo, p.pitch_high), torch.int32)
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
        for key, tab in self.normalisers:
            if key not in refs:
                refs[key] = cqt_window_max(b.wave, getattr(self, tab), p.H)
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
        for key, tab in self.normalisers:
            out[key] = cqt_window_max(s, getattr(self, tab), p.H)[0]
        return out

    @property
    def normalisers(self):
        """(song-level CQT normaliser, the table of its grid) of every normaliser this loop's heads divide by
        (training.py:271-282), in a fixed order: ref_C_1 for the pitch head, ref_C_inst where an instrument tower reads
        C_sw_inst, ref_C_foc for the velocity head and for the focused CQT towers.  ref_mag comes with the STFT."""
        inputs = self.instrument_inputs
        out = []
        if 'pitch' in self.heads:
            out.append(('ref_C_1', 'tab_ref1'))
        if 'C_sw_inst' in inputs:
            out.append(('ref_C_inst', 'tab_refi'))
        if 'velocity' in self.heads or any(k.startswith('C_sw_inst_foc') for k in inputs):
            out.append(('ref_C_foc', 'tab_reff'))
        return tuple(out)

    @property
    def needs_wave(self):
        return 'pitch' in self.heads or 'velocity' in self.heads or any(k.startswith('C_') for k in self.instrument_inputs)

    @property
    def needs_phase(self):
        # the unit phase: read by the iSTFT behind the CQT heads from iteration 1 on, and by a `ph` tower at once
        return (self.iters > 1 and self.needs_wave) or 'ph' in self.instrument_inputs

    def note_features(self, b, src, wave_r, pitch, names):
        """The instrument towers' part of the feature recipe (training.py:343-380) for the windows of the AudioBatch
        `b`: the arrays `names` (of FEATURE_NAMES), each a [B, instrument_bands, instrument_frames] device tensor, in
        the order asked for.  src [B, frames] int32: the step's resize table; wave_r [B, L]: what the CQT towers read
        as the windows' waveform (may be None when no C_* array is asked for); pitch [B] int32: the decided pitches
        (the loop's constant 60 without the pitch head).  Needs self.refs (prepare() / the song walk).
        The FFT-side arrays of the decided pitch come from one amt_note_features launch, those of the constant tone
        from another; every CQT array is one amt_cqt_slices launch."""
        p, refs = self.p, self.refs
        B = b.mag.shape[0]
        names = tuple(names)
        if any(k not in FEATURE_NAMES for k in names):
            raise ValueError('Requested attribute does not exist')
        got = {}
        for table, tone in ((_FFT_FEATURES, pitch), (_FFT_FEATURES_CONST, None)):
            want = tuple(dict.fromkeys(table[k] for k in names if k in table))
            if want:
                out = b.note_features(src, tone, self.tone_bin, p.pitch_low, p.instrument_bands, ref=refs['ref_mag'],
                                      want=want, const_tone=CONST_TONE)
                got.update({k: out[table[k]] for k in names if k in table})
        for k in names:
            if k in got:
                continue
            if k == 'C_sw_inst':
                got[k] = cqt_slices(wave_r, src, self.tab_inst, p.instrument_bands, p.H, ref=refs['ref_C_inst'])
                continue
            if self.tab_foc is None:
                raise ValueError('Requested attribute does not exist')       # the loop's model has no focused CQT tower
            bin0 = empty((B,), torch.int32)
            if k == 'C_sw_inst_foc':
                _lib.check(self.lib.amt_affine_i32(ptr(pitch), B, self.foc_bpt, -self.foc_bpt * p.pitch_low, ptr(bin0),
                                                   stream_ptr()))
            else:
                bin0.fill_(self.foc_bpt * (CONST_TONE - p.pitch_low))
            got[k] = cqt_slices(wave_r, src, self.tab_foc, p.instrument_bands, p.H, bin0=bin0, ref=refs['ref_C_foc'])
        return [got[k] for k in names]

    def _step(self, b, wave_fn, fmax, before_subtract=None, stems=None):
        """One detect -> subtract step on the windows of `b` -- the head sequence both traversals share (iterate() for
        independent windows, run_songs() for the song walk).  wave_fn() returns what the CQT heads read as the windows'
        waveform; before_subtract(onset, end, guess_frames) runs after the guess has been selected and before it is
        subtracted (run_songs decides there which songs detect).  stems: None, or the _lib.StemArgs of the song
        walk (SongState.step) -- its `program` is set here to the step's decided programs (NULL without the instrument
        head: stem 0) and it goes to the subtraction (AudioBatch.subtract(stems=)).
        Returns (onset, end, pitch, program, velocity)."""
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
            towers = self.note_features(b, src, wave_r, pitch, self.instrument_inputs)
            tr['instrument'] = self.nets['instrument'].classify(towers[0] if len(towers) == 1 else towers)
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
            if stems is not None:
                stems.program = program.data_ptr() if program is not None else None
            if self.guess == 'bank':
                b.subtract(self.bank_mag, self.bank_max, gidx, gfr, onset, normalize=True, relu=True,
                           span=self.span_subtract, stems=stems)
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
                b.subtract(g.mag, g.ref_max, None, gfr, onset, normalize=True, relu=True, span=self.span_subtract,
                           stems=stems)
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

    def prepare_songs(self, songs, refs=None, spectra=None, song0=0, keep_residual=False, keep_stems=False):
        """Set-up of the song walk, once per batch of songs: a song_walk.SongState of one slot per song and ONE admission
        of song i into slot i (SongState.admit: the songs' STFT, training.py:265-269, the song-level constants, :269-282,
        the first windows, section(0, None, timing_frames), :284, the raw-sample table and the per-song integers).
        songs: sequence of 1-d float32 waveforms of more than n_fft / 2 samples.  refs: optional dict(ref_mag, ref_C_1,
        ref_C_inst, ref_C_foc) of [B] tensors instead of the constants computed here.  spectra: optional AudioBatch that
        already holds the songs' STFT (mag, ph, ref_max; songs of equal length, one per row) -- it is read, not changed.
        song0: the index of the first song (state.slot_song).  keep_residual: every slide writes the outgoing half
        window back into the pool (SongState), for walk_songs(residual=True) / state.residual_waves().  keep_stems:
        every subtraction adds what it removed into the instrument stems (SongState), for walk_songs(stems=True) /
        state.stem_waves().  Returns the state walk_songs() advances."""
        song_walk.check_walk(self, stems=keep_stems)
        return song_walk.prepare_songs(self, songs, refs=refs, spectra=spectra, song0=song0, keep_residual=keep_residual,
                                       keep_stems=keep_stems)

    def walk_songs(self, st, max_notes=8, silence=1e-3, poll=16, song0=0, max_steps=None, residual=False, stems=False):
        """The steps of the song walk on a state from prepare_songs(); see run_songs().  max_steps: stop after that many
        steps even if songs are unfinished (the state can be inspected, not resumed).  residual: see run_songs(); the
        state must have been prepared with keep_residual; stems likewise, with keep_stems.  Returns events [steps, B, 9]
        int32 (device)."""
        song_walk.check_walk(self, max_notes, silence, stems=stems)
        return song_walk.walk_songs(st, max_notes, silence, poll=poll, song0=song0, max_steps=max_steps,
                                    residual=residual, stems=stems)

    def run_songs(self, songs, max_notes=8, silence=1e-3, poll=16, song0=0, refs=None, residual=False, stems=False):
        """The reference's own traversal (training.py:284, :296-328) with the predicted note where it has the gold
        note, for B songs at once: ONE live window of timing_frames frames per song, cut from the song's spectrogram
        (one STFT per song) and, whenever the predicted onset lies in its second half, slid by half a window with
        the residual of every subtraction kept.  prepare_songs() + walk_songs().

        songs: sequence of 1-d float32 waveforms (device tensors or arrays) of any lengths > n_fft / 2 samples.
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
        t_song the per-song integers, state.refs the song-level constants.

        residual=True: what the walk left of every song, to listen to (the reference dumps _full_window / _guessed /
        _after_subtr .flac per subtraction, training.py:438-447).  Every slide then stores the half window it pushes
        out back into the song's frames of the spectrogram pool (amt_song_slide_keep), and after the walk
        state.residual is a list with one 1-d float32 device tensor of hop * (frames - 1) samples per song: the iSTFT
        of the residual magnitudes times the song's own phases (util_audio.py:94-97), all songs in one launch
        (amt_istft_ragged).  None stands for a song the walk did not finish.  Events are the same with and without.

        stems=True: what the walk took OUT of every song, split by instrument group (the reference's _guessed.flac
        beside _after_subtr.flac, training.py:426-447) -- a subtractive transcriber is a source separator for free.
        Every subtraction adds before - after of the frames it touches into state.stems[g] at the song's own pool
        frames (amt_subtract_span_stems), g = the index in this loop's `groups` of the decided program's group (0
        without the instrument head).  After the walk state.stem_audio is a list with one [G, hop * (frames - 1)]
        float32 device tensor per song (None: unfinished), the iSTFT of each stem times the song's phases.  For every
        bin of a finished song, STFT magnitude = residual + sum of the stems within (2 max_notes + 2) 2^-24 of it
        (DESIGN 14).  Independent of residual=; events are the same with and without.  ValueError with
        AMT_SUBTRACT_SPAN=0: only the span subtraction keeps stems."""
        song_walk.check_walk(self, max_notes, silence, stems=stems)
        st = song_walk.prepare_songs(self, songs, refs=refs, song0=song0, keep_residual=residual, keep_stems=stems)
        return song_walk.walk_songs(st, max_notes, silence, poll=poll, song0=song0, residual=residual, stems=stems), st

    def iter_song_queue(self, songs, slots, max_notes=8, silence=1e-3, poll=16, pool_frames=None, on_finish=None,
                        residual=False, stems=False):
        """Continuous batching of the song walk: any number of songs of any lengths walked through `slots` live windows,
        a finished slot handed to the next song of the queue (the reference's unit of work is a dataset of songs, one
        song after the other per worker, training.py:623-634).  State, admission and step are run_songs' own
        (song_walk.SongState); a song's records are those run_songs([song]) gives for it alone, whatever shares the
        batch with it.

        songs: a sequence or an iterator of 1-d float32 waveforms (arrays or tensors), consumed lazily -- only the
        songs in a slot, and up to `slots` waiting ones, are held; a song is checked when it is pulled.  Yields
        (song_index, events [k, 9] int32 host array) as each song finishes: the song's own records in step order (kinds
        DETECT / SLIDE / FORCED_SLIDE), `step` counted from 0 within the song, `song` = its index in the queue.

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
        The per-slot tables that run_songs sizes from its one admission (window positions and pieces of the raw-sample
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
        [detect, slide, forced slide, idle]).
        residual=True: yields (song_index, events, residual) -- the song's residual waveform as run_songs(residual=True)
        gives it for that song alone (1-d float32 device tensor).  At a poll point ONE residual_waves() call covers
        every song found finished there; it is enqueued before their regions are released, on the walk's stream, so it
        reads them ahead of the STFT of any later admission.
        stems=True: the song's stems [G, samples] (run_songs(stems=True) for that song alone) are appended to what is
        yielded -- (song_index, events[, residual][, stems]), the optional items in that order.  They too are produced
        before the regions are released; an admission zeroes the stems of the regions it hands out."""
        song_walk.check_walk(self, max_notes, silence, slots, pool_frames, stems=stems)
        return song_walk.iter_song_queue(self, songs, slots, max_notes, silence, poll=poll, pool_frames=pool_frames,
                                         on_finish=on_finish, residual=residual, stems=stems)

    def run_song_queue(self, songs, slots, max_notes=8, silence=1e-3, poll=16, pool_frames=None, on_finish=None,
                       residual=False, stems=False):
        """iter_song_queue() run to its end.  Returns the list of the songs' records, events [k, 9] int32 host arrays,
        in queue order; with residual=True a list of (events, residual waveform) pairs, with stems=True of
        (events[, residual], stems) tuples."""
        out = {}
        for item in self.iter_song_queue(songs, slots, max_notes=max_notes, silence=silence, poll=poll,
                                         pool_frames=pool_frames, on_finish=on_finish, residual=residual,
                                         stems=stems):
            out[item[0]] = tuple(item[1:]) if residual or stems else item[1]
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
