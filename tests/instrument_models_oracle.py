"""Test infrastructure: the CPU oracles of the loop and of the song walk with any of the reference's ten instrument
models (training.py:466-477) standing where oracle.loop.LoopOracle has the plain CQT model.  Composed from the
oracle's own pieces only; the product is not imported.

The instrument towers are built the way the reference composes them (training.py:337-380):
    audio_sw = audio_w.resize(onset, duration, frames, attribs=['mag', 'ph'])                   :337-339
    F        = audio_sw.section_power('mag', lo, lo + instrument_bands), lo = midi_tone_to_FFT(pitch) or of C4   :347-357
    F_log10  = log10(1000 F + 1) / its maximum;  F / ref_mag;  ph = (angle(section_power('ph')) + 3.15) / 6.3   :350-363
    C_sw_inst_foc(_const): instrument_bands bins at 4 x instrument_bins_per_tone from the pitch (from C4) -- a slice
    of ONE global grid from pitch_low, as LoopOracle slices tab_vel                              :365-380
onset and duration are frames in the loop; resize() takes seconds, so each frame is handed over as a time inside its
interval (SongOracle.seconds_of_frame)."""
import hashlib

import numpy as np

from oracle import audio as oa
from oracle import cqt as ocqt
from oracle import rdcnn as orc
from oracle.loop import LoopOracle

from song_oracle import SongOracle           # tests/song_oracle.py

CONST_TONE = 60
# (head, fingerprint of its weights, dtype, input bytes) -> the network's output: the oracle's forward pass is a pure
# function of those, and the runs of one test session repeat many of them (the float32 run before and inside
# compare_windows; iteration 0 of every model sees the same windows through the same timing and pitch heads)
_NET_MEMO = {}


def _sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
# model name -> (head_config name = InstrumentClassifier variant, tower inputs): the reference's list, restated; the
# CPU test pins it and the product's table against the same written-out pairs
MODELS = {
    'instrument': ('instrument', ('C_sw_inst',)),
    'instrument_focused_lin': ('instrument_focused', ('F_sw_inst_foc',)),
    'instrument_focused_lin_log10': ('instrument_focused', ('F_sw_inst_foc_log10',)),
    'instrument_focused_const_lin': ('instrument_focused_const', ('F_sw_inst_foc_const',)),
    'instrument_focused_const_lin_log10': ('instrument_focused_const', ('F_sw_inst_foc_const_log10',)),
    'instrument_dual_lin': ('instrument_dual', ('C_sw_inst', 'F_sw_inst_foc')),
    'instrument_dual_lin_phase': ('instrument_dual', ('F_sw_inst_foc', 'ph')),
    'instrument_focused': ('instrument_focused', ('C_sw_inst_foc',)),
    'instrument_focused_const': ('instrument_focused_const', ('C_sw_inst_foc_const',)),
    'instrument_dual': ('instrument_dual', ('C_sw_inst', 'C_sw_inst_foc')),
}


class InstrumentFeatures:
    """Mixin over LoopOracle: the instrument towers of a model and the conditions the parity tests assert on them."""

    def _init_model(self, model):
        p = self.p
        self.model = model
        self.cfg['instrument'] = orc.head_config(p, MODELS[model][0])
        self.foc_bpt = 4 * p.instrument_bins_per_tone
        n_foc = self.foc_bpt * (p.pitch_high - p.pitch_low) + p.instrument_bands
        self.tab_foc = ocqt.cqt_table(p.sr, float(oa.midi_to_hz(p.pitch_low)), n_foc, 12 * self.foc_bpt)
        self.conditions = dict(min_pi_distance=np.inf, zero_log_tiles=0, steps=0, empty_steps=0)
        self._prints = {}
        if not hasattr(self, '_cqt_memo'):
            self._cqt_memo = {}            # (may be shared between oracles of one test: assign the same dict)

    def _cqt(self, wf, src, grid, b0, n):
        """ocqt.cqt_frames on a slice of a grid, remembered per (waveform, frames, slice): the float32 and float64
        network runs of one test see the same windows."""
        wf, tab = np.asarray(wf), getattr(self, grid)
        key = (hashlib.sha1(np.ascontiguousarray(wf).tobytes()).hexdigest(), tuple(int(t) for t in src), grid, b0, n)
        if key not in self._cqt_memo:
            self._cqt_memo[key] = ocqt.cqt_frames(wf, src, tab[0][b0:b0 + n], tab[1][b0:b0 + n], self.p.H)
        return self._cqt_memo[key]

    def fft_features(self, ac, onset, end, pitch, ref_mag):
        """{name: [instrument_bands, frames] float64} of the four FFT-side arrays and ph, for the live window `ac`;
        ref_mag: the song-level normaliser (mid_wf.ref_mag, training.py:352)."""
        p = self.p
        sec = lambda frame: SongOracle.seconds_of_frame(ac, frame)
        sw = ac.resize(sec(onset), sec(end) - sec(onset), p.instrument_frames, attribs=['mag', 'ph'])
        out = {}
        for suffix, tone in (('', pitch), ('_const', CONST_TONE)):
            lo = ac.midi_tone_to_FFT(tone)
            F = np.asarray(sw.section_power('mag', lo, lo + p.instrument_bands), np.float64)
            lg = np.log10(F * 1000 + 1)
            with np.errstate(divide='ignore', invalid='ignore'):
                out['F_sw_inst_foc%s_log10' % suffix] = lg / np.max(lg)
            out['F_sw_inst_foc%s' % suffix] = F / ref_mag
            out['_zero_tile%s' % suffix] = not np.max(lg) > 0
        lo = ac.midi_tone_to_FFT(pitch)
        ang = np.angle(sw.section_power('ph', lo, lo + p.instrument_bands))
        out['ph'] = (ang + 3.15) / 6.3
        out['_pi_distance'] = float(np.min(np.pi - np.abs(ang)))
        return out

    def instrument_towers(self, ac, wf, src, refs, onset, end, pitch):
        """The model's tower inputs, in order; the test conditions are recorded on the way."""
        p = self.p
        names = MODELS[self.model][1]
        fft = self.fft_features(ac, onset, end, pitch, refs['ref_mag']) if any(not k.startswith('C_') for k in names) else {}
        c = self.conditions
        c['steps'] += 1
        c['empty_steps'] += not end > onset
        towers = []
        for k in names:
            if k == 'C_sw_inst':
                x = self._cqt(wf, src, 'tab_inst', 0, p.instrument_bands) / refs['ref_C_inst']
            elif k.startswith('C_sw_inst_foc'):
                tone = CONST_TONE if k.endswith('_const') else pitch
                x = self._cqt(wf, src, 'tab_foc', self.foc_bpt * (tone - p.pitch_low), p.instrument_bands) \
                    / refs['ref_C_foc']
            else:
                x = fft[k]
                if k == 'ph':
                    c['min_pi_distance'] = min(c['min_pi_distance'], fft['_pi_distance'])
                if k.endswith('_log10'):
                    c['zero_log_tiles'] += fft['_zero_tile_const' if '_const' in k else '_zero_tile']
            towers.append(x)
        return towers

    def _forward(self, name, cfgname, xs):
        xs = [np.asarray(x, np.float32)[None, :, :, None] for x in xs]
        if name not in self._prints:
            self._prints[name] = _sha(*[self.w[name][k] for k in sorted(self.w[name])])
        key = (name, cfgname, self._prints[name], np.dtype(self.dtype).name, _sha(*xs))
        if key not in _NET_MEMO:
            _NET_MEMO[key] = orc.forward(self.w[name], self.cfg[cfgname], xs, self.dtype)[0]
        return _NET_MEMO[key].copy()

    def _predict(self, name, cfgname, x):
        return self._forward(name, cfgname, [x])

    def _predict_towers(self, towers):
        return self._forward('instrument', 'instrument', towers)

    def _subtract(self, ac, m, onset, end, pitch, program, velocity, ref_mag):
        """LoopOracle.run_window's subtraction (audio_complete.subtract with a magnitude subtrahend,
        util_audio.py:240-259, offset in frames) from the window's magnitudes m; ref_mag: the window's own maximum."""
        p = self.p
        T = ac.shape[1]
        n_pitch = p.pitch_high - p.pitch_low + 1
        pr = min(max(program, 0), p.instrument_classes - 1) if program >= 0 else 0
        g = int(self.prog_group[pr]) * n_pitch + min(max(pitch - p.pitch_low, 0), n_pitch - 1)
        if self.guess_fn is not None:
            gw = np.asarray(self.guess_fn(pr, pitch, velocity, max(end - onset, 0)), np.float32)
            gmag = oa.magphase(oa.stft(gw, p.N, p.H))[0]
            gmax, gframes = gmag.max(), gmag.shape[1]
        else:
            gmag, gmax, gframes = self.bank_mag[g], self.bank_max[g], self.bank_frames
        gf = min(max(end - onset, 0) + self.tail_frames, gframes)
        mag_sub = gmag[:, :gf].copy()
        mag_sub *= ref_mag / gmax
        if mag_sub.shape[1] + onset > T:
            mag_sub = mag_sub[:, :T - onset]
        m[:, onset:onset + mag_sub.shape[1]] -= mag_sub
        ac.mag = np.maximum(m, 0, m)


class ModelLoopOracle(InstrumentFeatures, LoopOracle):
    """LoopOracle whose instrument head is `model`; run_window(..., model=) may name another for one window."""

    def __init__(self, *args, model='instrument', **kw):
        LoopOracle.__init__(self, *args, **kw)
        self._init_model(model)

    def run_window(self, wave, refs, window_id=0, force=None, model=None):
        if model is not None and model != self.model:
            self._init_model(model)
        p = self.p
        self._force = force
        self.decisions = []
        ac = oa.AudioCompleteOracle(np.asarray(wave, np.float32), p.N, p.H)
        ac.mag
        T = ac.shape[1]
        events = np.full((self.iters, 7), -1, np.int32)
        for it in range(self.iters):
            self._it = it
            if 'timing' in self.heads:
                ct = oa.AudioCompleteOracle.compress_bands(ac.mag, bands=p.timing_bands)
                ct = oa.AudioCompleteOracle._resize(ct, p.timing_frames) / refs['ref_mag']
                onset = self._round(self._predict('timing_start', 'timing', ct)[0], 0, T - 1, 'timing_start', 5)
                end = self._round(self._predict('timing_end', 'timing', ct)[0], 0, T, 'timing_end', 6)
            else:
                onset, end = 0, p.pitch_frames
            src = ocqt.slice_C_frames(T, onset, end, p.pitch_frames)
            wf = ac.wf
            pitch, program, velocity = 60, -1, -1
            if 'pitch' in self.heads:
                cp = ocqt.cqt_frames(wf, src, self.tab_pitch[0], self.tab_pitch[1], p.H) / refs['ref_C_1']
                pitch = self._round(self._predict('pitch', 'pitch', cp)[0], p.pitch_low, p.pitch_high, 'pitch', 2)
            if 'instrument' in self.heads:
                program = self._argmax(self._predict_towers(self.instrument_towers(ac, wf, src, refs, onset, end, pitch)))
            if 'velocity' in self.heads:
                b0 = self.vel_bpt * (pitch - p.pitch_low)
                cv = ocqt.cqt_frames(wf, src, self.tab_vel[0][b0:b0 + p.bins_velocity],
                                     self.tab_vel[1][b0:b0 + p.bins_velocity], p.H) / refs['ref_C_foc']
                velocity = self._round(self._predict('velocity', 'velocity', cv)[0], 1, 127, 'velocity', 4)
            if self.do_subtract:
                self._subtract(ac, ac.mag, onset, end, pitch, program, velocity, ac.ref_mag)
            events[it] = (window_id, it, pitch, program, velocity, onset, end)
        return events, ac.mag


class ModelSongOracle(InstrumentFeatures, SongOracle):
    """SongOracle whose instrument head is `model`: _detect with the model's towers."""

    def __init__(self, *args, model='instrument', **kw):
        SongOracle.__init__(self, *args, **kw)
        self._init_model(model)

    def _detect(self, ac, refs, onset, end):
        p = self.p
        T = ac.shape[1]
        src = ocqt.slice_C_frames(T, onset, end, p.pitch_frames)
        wf = ac.wf
        pitch, program, velocity = 60, -1, -1
        if 'pitch' in self.heads:
            cp = ocqt.cqt_frames(wf, src, self.tab_pitch[0], self.tab_pitch[1], p.H) / refs['ref_C_1']
            pitch = self._round(self._head('pitch', 'pitch', cp)[0], p.pitch_low, p.pitch_high, 'pitch', 2)
        if 'instrument' in self.heads:
            program = self._argmax(self._predict_towers(self.instrument_towers(ac, wf, src, refs, onset, end, pitch)))
        if 'velocity' in self.heads:
            b0 = self.vel_bpt * (pitch - p.pitch_low)
            cv = ocqt.cqt_frames(wf, src, self.tab_vel[0][b0:b0 + p.bins_velocity],
                                 self.tab_vel[1][b0:b0 + p.bins_velocity], p.H) / refs['ref_C_foc']
            velocity = self._round(self._head('velocity', 'velocity', cv)[0], 1, 127, 'velocity', 4)
        if self.do_subtract:
            self._subtract(ac, np.asarray(ac.mag, np.float32), onset, end, pitch, program, velocity, np.float32(ac.ref_mag))
        return pitch, program, velocity
