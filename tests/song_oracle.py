"""Test infrastructure: CPU restatement of the song-resident sliding-window walk (training.py:284, :296-328 with the
predicted note where the reference has the gold note), composed from the oracle's own pieces only --
oracle.audio.AudioCompleteOracle (section / slice / concat / wf), oracle.cqt, oracle.rdcnn.forward and the rounding
and hand-over rules of oracle.loop.LoopOracle.  It does not import the product.

Walk, per song (frames, not the reference's whole seconds -- int(window_size_note_time / 2) is 0 for a 1-s window):
    song = audio_complete(wave); song.mag                    training.py:265-269
    W = song.section(0, None, timing_frames)                 :284        offset = 0, count = 0
    per step:  onset, end from the timing heads on W         :333-336
        onset >= half                                  -> slide
        count >= max_notes or max(W.mag) <= silence * ref_mag (float32)  -> forced slide      (build-defined, :313-314)
        else detect: the remaining heads, guess, subtraction exactly as LoopOracle.run_window; count += 1
    slide:  offset += half; new = song.section(offset + half, None, half); W.slice(half, 2 half); W.concat(new); count = 0
    finished once offset >= the song's frames                :296
The waveform the CQT heads read is W.wf, whatever the class makes of it: raw song samples while nothing has been
subtracted (section / slice / concat carry _wf along), the iSTFT of mag * ph afterwards (the mag setter clears _wf,
slice and concat keep None)."""
import numpy as np

from oracle import audio as oa
from oracle import cqt as ocqt
from oracle.loop import LoopOracle

DETECT, SLIDE, FORCED_SLIDE, FINISHED = 0, 1, 2, 3


class SongOracle(LoopOracle):
    """LoopOracle's heads, tables, guess bank and rounding; the traversal is the walk above.
    predict: None, or a stub (head name, step) -> float standing for the networks (scripted cases)."""

    def __init__(self, *args, predict=None, **kw):
        super().__init__(*args, **kw)
        self.stub = predict

    def _head(self, name, cfgname, x):
        if self.stub is not None:
            return [self.stub(name, self._it)]
        return self._predict(name, cfgname, x)

    @staticmethod
    def seconds_of_frame(song, frame):
        """A time that audio_complete._seconds_to_frames maps to `frame` (the middle of the frame's interval)."""
        return (frame + 0.5) * song.wf.shape[0] / (song.shape[1] * song.sr)

    def run_song(self, wave, refs, max_notes, silence, song_id=0, force=None, max_steps=None, windows=None):
        """wave float32 [L]; refs as LoopOracle.run_window.  force: None or (product events [steps, 9] of this song,
        bands) -- near-tie decisions adopt the product's integer (LoopOracle._round).  windows: a list that receives a
        copy of the window's magnitudes after every step.
        Returns (events [steps, 9] int32, final window magnitudes [F, T])."""
        p = self.p
        tf = p.timing_frames
        half = int(tf / 2)
        self.decisions = []
        song = oa.AudioCompleteOracle(np.asarray(wave, np.float32), p.N, p.H)
        song.mag
        t_song = song.shape[1]
        W = song.section(0, None, tf)
        offset = count = step = 0
        bound = -(-t_song // half) * (max_notes + 1)
        events = []
        ref_mag32 = np.float32(refs['ref_mag'])
        while offset < t_song and step < (bound if max_steps is None else max_steps):
            self._it = step
            self._force = None
            if force is not None:
                e = force[0][step]
                # LoopOracle's hand-over reads 7-column window events: frames relative to the window
                self._force = ({step: (e[0], e[1], e[3], e[4], e[5], e[6] - e[8], e[7] - e[8])}, force[1])
            ct = oa.AudioCompleteOracle.compress_bands(W.mag, bands=p.timing_bands)
            ct = oa.AudioCompleteOracle._resize(ct, tf) / refs['ref_mag']
            onset = self._round(self._head('timing_start', 'timing', ct)[0], 0, tf - 1, 'timing_start', 5)
            end = self._round(self._head('timing_end', 'timing', ct)[0], 0, tf, 'timing_end', 6)
            silent = np.float32(W.mag.max()) <= np.float32(silence) * ref_mag32
            if onset >= half or count >= max_notes or silent:
                kind = SLIDE if onset >= half else FORCED_SLIDE
                events.append((song_id, step, kind, -1, -1, -1, offset + onset, offset + end, offset))
                offset += half
                new = song.section(self.seconds_of_frame(song, offset + half), None, half)
                W.slice(half, 2 * half)
                W.concat(new)
                count = 0
            else:
                pitch, program, velocity = self._detect(W, refs, onset, end)
                events.append((song_id, step, DETECT, pitch, program, velocity, offset + onset, offset + end, offset))
                count += 1
            if windows is not None:
                windows.append(np.array(W.mag, copy=True))
            step += 1
        self._force = None
        return np.asarray(events, np.int32).reshape(-1, 9), W.mag

    def _detect(self, ac, refs, onset, end):
        """The detect half of LoopOracle.run_window on the live window."""
        p = self.p
        T = ac.shape[1]
        src = ocqt.slice_C_frames(T, onset, end, p.pitch_frames)
        need_wave = any(h in self.heads for h in ('pitch', 'instrument', 'velocity'))
        wf = ac.wf if need_wave else None
        pitch, program, velocity = 60, -1, -1
        if 'pitch' in self.heads:
            cp = ocqt.cqt_frames(wf, src, self.tab_pitch[0], self.tab_pitch[1], p.H) / refs['ref_C_1']
            pitch = self._round(self._head('pitch', 'pitch', cp)[0], p.pitch_low, p.pitch_high, 'pitch', 2)
        if 'instrument' in self.heads:
            ci = ocqt.cqt_frames(wf, src, self.tab_inst[0], self.tab_inst[1], p.H) / refs['ref_C_inst']
            program = self._argmax(self._predict('instrument', 'instrument', ci))
        if 'velocity' in self.heads:
            b0 = self.vel_bpt * (pitch - p.pitch_low)
            cv = ocqt.cqt_frames(wf, src, self.tab_vel[0][b0:b0 + p.bins_velocity],
                                 self.tab_vel[1][b0:b0 + p.bins_velocity], p.H) / refs['ref_C_foc']
            velocity = self._round(self._head('velocity', 'velocity', cv)[0], 1, 127, 'velocity', 4)
        if self.do_subtract:
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
            mag_sub *= np.float32(ac.ref_mag) / gmax                  # audio_complete.subtract, util_audio.py:240-259
            if mag_sub.shape[1] + onset > T:
                mag_sub = mag_sub[:, :T - onset]
            m = np.asarray(ac.mag, np.float32)
            m[:, onset:onset + mag_sub.shape[1]] -= mag_sub
            ac.mag = np.maximum(m, 0, m)
        return pitch, program, velocity


def pad_finished(events, steps, song_id, half):
    """The product keeps a finished song's slot: its records after the finishing slide are kind FINISHED, every field
    -1 but song, step, kind and the final offset."""
    ev = np.asarray(events, np.int32).reshape(-1, 9)
    if steps <= len(ev):
        return ev[:steps]
    assert ev[-1, 2] in (SLIDE, FORCED_SLIDE)
    pad = np.full((steps - len(ev), 9), -1, np.int32)
    pad[:, 0] = song_id
    pad[:, 1] = np.arange(len(ev), steps)
    pad[:, 2] = FINISHED
    pad[:, 8] = ev[-1, 8] + half
    return np.concatenate([ev, pad])


# ---- the songs of the live parity cases and of the full-depth fixture (tests/golden/gen_song_fixtures.py) ---------------
def make_songs(p, seed, half_windows, silent_tail=None, gap=(0.2, 0.45), quantise=False):
    """Synthetic songs of the given lengths (in half windows): one short note every `gap` seconds, rendered by the
    float64 synthesiser restatement; quantise = 24-bit PCM values (exact in float32, the same on every machine)."""
    from oracle import synth as osynth
    rng = np.random.default_rng(seed)
    half_len = p.H * (p.timing_frames // 2)
    out = []
    for i, hw in enumerate(half_windows):
        n = int(round(hw * half_len))
        dur_s = n / p.sr
        notes, t = [], float(rng.uniform(0.02, 0.2))
        while t < (dur_s if silent_tail is None or i != silent_tail else dur_s * 0.35) - 0.15:
            notes.append((0, int(rng.integers(40, 90)), int(rng.integers(60, 120)), t, float(rng.uniform(0.1, 0.3))))
            t += float(rng.uniform(*gap))
        w = osynth.render_window(notes, n, p.sr).numpy()
        if quantise:
            w = np.clip(np.rint(w.astype(np.float64) * 8388608.0), -8388608, 8388607) / 8388608.0
        out.append(w.astype(np.float32))
    return out


# name -> n_fft, window seconds, guess, song seed, lengths in half windows, max_notes, silence, index of the song with a
# silent tail, frames added to timing_start's output bias
WALK_CASES = {
    'bank2048': (2048, 1, 'bank', 11, (2.3, 3.0, 4.4, 5.0), 2, 1e-4, None, 0),
    'render2048': (2048, 1, 'render', 12, (2.0, 3.6, 2.7, 4.1), 2, 1e-4, None, 0),
    'bank4096': (4096, 2, 'bank', 13, (2.5, 3.0, 4.2, 2.1), 2, 1e-4, None, 0),
    'render4096': (4096, 2, 'render', 14, (3.3, 2.0, 2.8, 4.0), 1, 1e-4, None, 0),
    'silence': (2048, 1, 'bank', 15, (4.6, 2.4, 5.0, 3.0), 3, 2e-2, 0, 0),     # the silent tail of song 0 trips `silence`
    # the seeded synthetic timing_start keeps its onsets in the first half of a window (frames 25-42), so every slide
    # above is a forced one; with its output moved up by 18 frames every onset lands in the second half: plain slides
    'plain_slides': (2048, 1, 'bank', 16, (3.2, 4.0, 2.6, 4.8), 3, 1e-4, None, 18),
}
HEADS = ('timing', 'pitch', 'velocity')
# the full-depth fixture: 516-frame windows (half = 258), the real 33-layer heads, two short songs
# (candidates: the generator keeps the first two without a decision near a rounding tie and stores which)
FULL = dict(n_fft=2048, seed=31, lengths=(2.4, 3.0, 2.2, 2.8, 2.6, 3.2), keep=2, max_notes=1, silence=1e-4, gap=(0.9, 1.6))
