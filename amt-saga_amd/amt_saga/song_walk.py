"""The song walk behind TranscriptionLoop.run_songs and run_song_queue: ONE state (SongState: `slots` live windows over a
pool of song frames), ONE admission (SongState.admit: songs into slots), ONE step (SongState.step) and two drivers.
walk_songs() steps a fixed batch -- a state whose every slot was admitted once, by prepare_songs(), and is never
refilled -- with the records kept on the device; iter_song_queue() hands finished slots to the next songs of a queue and
yields each song's records as it finishes.  What the walk computes is described at TranscriptionLoop.run_songs and
iter_song_queue (loop.py), which validate their arguments (check_walk) and delegate here."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .audio import AudioBatch, cqt_window_max, ldf_of
from .device import empty, ptr, require_gpu, stream_ptr, to_dev, zeros

# one record per step and song; onset / end / offset are song frames
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


def check_walk(lp, max_notes=1, silence=0.0, slots=1, pool_frames=None, stems=False):
    """The argument checks of every public entry of the walk, before any device set-up."""
    if stems and not lp.span_subtract:
        raise ValueError('run_songs: stems need the span subtraction (AMT_SUBTRACT_SPAN=0 is set)')
    if int(slots) < 1:
        raise ValueError('run_song_queue: slots must be at least 1')
    if int(max_notes) < 1:
        raise ValueError('run_songs: max_notes must be at least 1')
    if not float(silence) >= 0.0:
        raise ValueError('run_songs: silence must be >= 0')
    if 'timing' not in lp.heads or not lp.do_subtract:
        raise ValueError('run_songs: the walk needs the timing heads and the subtraction')
    if lp.p.timing_frames % 2:
        raise ValueError('Invalid Input shape. run_songs needs an even timing_frames. Got: %d' % lp.p.timing_frames)
    if pool_frames is not None and int(pool_frames) < 1:
        raise ValueError('run_song_queue: pool_frames must be at least 1')


def check_song(p, song):
    """A song as the walk takes it: the 1-d float32 device tensor of a waveform the STFT accepts."""
    w = to_dev(song).reshape(-1)
    if w.numel() < p.H:
        raise ValueError('Invalid Input shape. Expected: a song of at least one hop (%d samples) . Got: %d'
                         % (p.H, w.numel()))
    if w.numel() <= p.N // 2:                                      # amt_stft_mag_ragged would leave it unwritten
        raise ValueError('Invalid Input shape. Expected: a song of more than n_fft / 2 = %d samples '
                         '(reflect padding) . Got: %d' % (p.N // 2, w.numel()))
    return w


class SongState:
    """The walk's state, every attribute allocated here: `slots` live windows (`batch`) over a pool of `pool_frames` song
    frames (s_mag, s_ph, and pool_frames x hop `samples` beside them: a song of T frames has fewer than T hops of
    samples, so the one free list `pool` governs both), the per-slot device integers, the song-level constants `refs`,
    the raw-sample table `seg` with the CQT heads' rows `wave` [slots, l_row], and the host's counters: steps, positions
    (of the longest song admitted), bound (the driver's step cap) and `stats` (see iter_song_queue).  Every slot starts
    idle: finished, song -1, and normalisers of 1 for its discarded heads to divide by.
    keep_residual: every slide stores the half window it pushes out back into the song's pool frames
    (amt_song_slide_keep), so that a FINISHED song's region of s_mag holds its residual spectrogram -- what every
    subtraction left of it -- and residual_waves() can resynthesise it.  Off (the default), the pool is never written
    after the admission's STFT.
    keep_stems: `stems` [G, pool_frames, ldf] beside s_mag, G = len(lp.groups) -- every subtraction adds what it removed
    (before - after, the clipped amount) into the stem of the note's instrument group, lp.prog_group[program] (stem 0
    without the instrument head), at the song's own pool frames (amt_subtract_span_stems).  A song's region of every
    stem is zeroed when it is admitted; nothing is written on a slide, so the flag is independent of keep_residual.  For
    every bin of a finished song, STFT magnitude = residual + sum of the stems, up to rounding;
    stem_waves() resynthesises them."""

    def __init__(self, lp, slots, pool_frames, keep_residual=False, keep_stems=False):
        if not lp._dev_ready:
            lp.setup_device()
        p, dev = lp.p, require_gpu()
        B, pool_frames = int(slots), int(pool_frames)
        tf, ldf = p.timing_frames, ldf_of(p.N)
        self.lp, self.slots, self.keep_residual, self.keep_stems = lp, B, bool(keep_residual), bool(keep_stems)
        self.pool = FramePool(pool_frames)
        self.s_mag, self.s_ph = empty((pool_frames, ldf)), empty((pool_frames, ldf, 2))
        self.samples = empty((pool_frames * p.H,))
        self.stems = empty((len(lp.groups), pool_frames, ldf)) if self.keep_stems else None
        b = self.batch = AudioBatch(None, p.N, p.H)
        b.mag, b.ph, b.ref_max = zeros((B, tf, ldf)), zeros((B, tf, ldf, 2)), zeros((B,))
        self.ref_keys = ['ref_mag'] + [k for k, _ in lp.normalisers]       # ref_mag comes with the STFT
        self.refs = {k: torch.ones((B,), dtype=torch.float32, device=dev) for k in self.ref_keys}
        self.t_song, self.offset, self.count = (zeros((B,), torch.int32) for _ in range(3))
        self.frame_base, self.sample_base = zeros((B,), torch.int64), zeros((B,), torch.int64)
        self.finished, self.clean = (torch.ones((B,), dtype=torch.int32, device=dev) for _ in range(2))
        self.slot_song = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.slide, self.detect, self.kind = (empty((B,), torch.int32) for _ in range(3))
        self.seg = zeros((B, 1, 1, 3), torch.int32)                # grows at an admission that needs more
        self.l_row = (tf * p.H + 3) // 4 * 4
        self.wave = empty((B, self.l_row))
        self.song_of, self.region = [-1] * B, [None] * B           # host: the slot's song (-1: free) and pool region
        self.frames = [0] * B                                      # host: frames of the slot's song
        self.lens = [0] * B                                        # host: samples of the slot's song
        self.residual = None                                       # walk_songs(residual=True): one waveform per slot
        self.stem_audio = None                                     # walk_songs(stems=True): one [G, samples] per slot
        self.steps = self.positions = self.bound = 0
        self.stats = dict(steps=0, songs=0, admissions=0, waits=0, bound=0, slot_steps=[0, 0, 0, 0])

    def admit(self, new, refs=None, spectra=None):
        """Puts new = [(slot, song index, waveform from check_song), ...] into their slots, in that order, up to the first
        song the pool has no region for now: samples into the pool, ONE amt_stft_mag_ragged launch, the song-level CQT
        normalisers per song (cqt_window_max), their rows of the raw-sample table, ONE amt_song_admit (first window
        section(0, None, timing_frames), training.py:284; integers, tables and normalisers of the slot).
        refs: dict of [len(new)] tensors that replace the normalisers (none is computed then).  spectra: an AudioBatch
        whose row j holds the STFT of new[j] (mag, ph, ref_max; read, not changed) in place of the STFT launch.
        Returns the window positions of the admitted songs, one per song."""
        lp, b, sp = self.lp, self.batch, stream_ptr()
        p, B = lp.p, self.slots
        H, tf, ldf = p.H, p.timing_frames, b.mag.shape[2]
        half = tf // 2
        took = []
        for slot, idx, w in new:
            f0 = self.pool.alloc(1 + w.numel() // H)
            if f0 is None:                                         # waits for a region; the songs behind it wait too
                break
            took.append((slot, idx, w, f0))
        if not took:
            return []
        n = len(took)
        lens = [int(w.numel()) for _, _, w, _ in took]
        t_song = [1 + L // H for L in lens]
        fbase = np.asarray([f0 for _, _, _, f0 in took], np.int64)
        for (_, _, w, f0), L in zip(took, lens):
            self.samples[f0 * H:f0 * H + L].copy_(w)
        d_fb, d_sb = to_dev(fbase, torch.int64), to_dev(fbase * H, torch.int64)
        if self.keep_stems:
            # on the walk's stream: behind a stem_waves() of the region's earlier song, ahead of the first subtraction
            for t, f0 in zip(t_song, fbase):
                self.stems[:, f0:f0 + t].zero_()
        if spectra is None:
            ref_mag, d_len = empty((n,)), to_dev(np.asarray(lens, np.int32), torch.int32)
            _lib.check(lp.lib.amt_stft_mag_ragged(b.plan, ptr(self.samples), ptr(d_sb), ptr(d_len), n, max(lens),
                                                  self.samples.numel(), sum(lens), ptr(self.s_mag), ptr(self.s_ph),
                                                  ptr(ref_mag), ptr(d_fb), self.pool.frames, ldf, sp))
        else:
            ref_mag = spectra.ref_max[:n].clone()
            for j, (t, f0) in enumerate(zip(t_song, fbase)):
                if spectra.mag.shape[1] != t:
                    raise ValueError('Invalid Input shape. Expected: %d frames . Got: %d' % (t, spectra.mag.shape[1]))
                self.s_mag[f0:f0 + t], self.s_ph[f0:f0 + t] = spectra.mag[j], spectra.ph[j]
        if refs is None:
            new_refs = [ref_mag] + [
                torch.cat([cqt_window_max(self.samples[f0 * H:f0 * H + L][None, :], getattr(lp, tab), H)
                           for f0, L in zip(fbase, lens)]).contiguous()
                for _, tab in lp.normalisers]
        else:
            new_refs = [to_dev(refs[k]).reshape(n).contiguous() for k in self.ref_keys]
        positions = [-(-t // half) for t in t_song]
        self.positions = max([self.positions] + positions)
        seg, l_row = song_wave_segments(lens, t_song, tf, p.sr, max(positions), min_len=tf * H)
        K, S = max(seg.shape[1], self.seg.shape[1]), max(seg.shape[2], self.seg.shape[2])
        if (K, S) != tuple(self.seg.shape[1:3]):                   # the per-slot piece table grows, its rows are kept
            grown = zeros((B, K, S, 3), torch.int32)
            grown[:, :self.seg.shape[1], :self.seg.shape[2]] = self.seg
            self.seg = grown
        if l_row > self.l_row:
            self.l_row, self.wave = l_row, empty((B, l_row))
        seg_new = np.zeros((n, K, S, 3), np.int32)
        seg_new[:, :seg.shape[1], :seg.shape[2]] = seg
        mask = np.zeros(B, np.int32)
        for j, (slot, idx, _, f0) in enumerate(took):
            mask[slot] = 1 + j
            self.song_of[slot], self.region[slot], self.frames[slot] = idx, int(f0), int(t_song[j])
            self.lens[slot] = lens[j]
        d_mask, d_seg = to_dev(mask, torch.int32), to_dev(seg_new, torch.int32)
        d_ts, d_song = to_dev(np.asarray(t_song, np.int32), torch.int32), \
            to_dev(np.asarray([idx for _, idx, _, _ in took], np.int32), torch.int32)
        a = _lib.song_admit_args(
            w_mag=b.mag, w_ph=b.ph, s_mag=self.s_mag, s_ph=self.s_ph, admit=d_mask, new_frame_base=d_fb, new_t_song=d_ts,
            new_sample_base=d_sb, new_song=d_song, new_seg=d_seg, new_ref=new_refs, frame_base=self.frame_base,
            t_song=self.t_song, sample_base=self.sample_base, slot_song=self.slot_song, seg=self.seg,
            ref=[self.refs[k] for k in self.ref_keys], offset=self.offset, count=self.count, finished=self.finished,
            clean=self.clean, w_stride=tf * ldf, B=B, n_new=n, T=tf, ldf=ldf, K=K, S=S)
        _lib.check(lp.lib.amt_song_admit(C.byref(a), sp))
        b._fmax = None                                             # the admitted windows' per-frame maxima are stale
        self.stats['admissions'] += 1
        self.stats['songs'] += n
        return positions

    def release(self, slot):
        self.pool.release(self.region[slot])
        self.song_of[slot], self.region[slot], self.frames[slot] = -1, None, 0
        self.lens[slot] = 0

    def residual_waves(self, slots):
        """What the walk left of the songs in `slots` (every one finished), as audio: the iSTFT of the residual
        magnitudes their slides wrote back into the pool times the songs' own phases (util_audio.py:94-97; the
        _after_subtr.flac of training.py:438-447 at song length), ONE amt_istft_ragged launch over their regions, on
        the walk's stream.  Returns one 1-d float32 device tensor of hop * (t_song - 1) samples per slot, in the order
        given.  ValueError: a state built without keep_residual, a free slot, or a song that is not finished (part of
        it is still in the window -- e.g. after a max_steps cut -- so its residual is not defined)."""
        if not self.keep_residual:
            raise ValueError('residual_waves: the state was built without keep_residual')
        out, base, lens = self._region_waves('residual_waves', slots, self.s_mag[None])
        return [out[0, int(a):int(a) + n] for a, n in zip(base, lens)]

    def stem_waves(self, slots):
        """What the walk took out of the songs in `slots` (every one finished), per instrument group, as audio: the
        iSTFT of each stem's region times the song's own phases (util_audio.py:94-97; the _guessed.flac of
        training.py:426-447 at song length, split by group), ONE amt_istft_ragged launch per group over the slots'
        regions, on the walk's stream.  Returns one [G, hop * (t_song - 1)] float32 device tensor per slot, in the order
        given; row g belongs to lp.groups[g].  ValueError: a state built without keep_stems, a free slot, or a song
        that is not finished."""
        if not self.keep_stems:
            raise ValueError('stem_waves: the state was built without keep_stems')
        out, base, lens = self._region_waves('stem_waves', slots, self.stems)
        return [out[:, int(a):int(a) + n] for a, n in zip(base, lens)]

    def region_spectra(self, slots):
        """What the walk left and what it took out of the songs in `slots` (every one finished), as magnitude
        spectrograms where they lie: per slot (residual, stems) -- residual the song's region of s_mag, [t_song, ldf],
        with keep_residual, else None; stems [G, t_song, ldf], row g of lp.groups[g], with keep_stems, else None.
        Views of the pool, nothing is copied or launched: they are what audio.spectrogram_png draws, valid until the
        slot is released.  ValueError: a state built with neither flag, a free slot, or a song that is not finished."""
        if not (self.keep_residual or self.keep_stems):
            raise ValueError('region_spectra: the state was built without keep_residual and without keep_stems')
        out = []
        for b in self._finished_slots('region_spectra', slots):
            f0, t = self.region[b], self.frames[b]
            out.append((self.s_mag[f0:f0 + t] if self.keep_residual else None,
                        self.stems[:, f0:f0 + t] if self.keep_stems else None))
        return out

    def _finished_slots(self, who, slots):
        """`slots` as integers, every one holding a finished song; else the ValueError of residual_waves."""
        slots = [int(b) for b in slots]
        if not slots:
            return slots
        fin = self.finished.cpu().numpy()
        for b in slots:
            if not 0 <= b < self.slots or self.region[b] is None:
                raise ValueError('%s: slot %d holds no song' % (who, b))
            if not fin[b]:
                raise ValueError('%s: the song in slot %d is not finished' % (who, b))
        return slots

    def _region_waves(self, who, slots, mags):
        """The iSTFT of the slots' regions of every mags[g] ([G, pool_frames, ldf]) times s_ph, one amt_istft_ragged
        launch per g.  Returns (out [G, samples], first sample per slot, samples per slot)."""
        G = int(mags.shape[0])
        slots = self._finished_slots(who, slots)
        if not slots:
            return empty((G, 0)), [], []
        lp, H = self.lp, self.lp.p.H
        frames = [self.frames[b] for b in slots]
        lens = [H * (t - 1) for t in frames]
        base = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        out = empty((G, int(base[-1])))
        if base[-1] > 0:
            d_fb = to_dev(np.asarray([self.region[b] for b in slots], np.int64), torch.int64)
            d_tf = to_dev(np.asarray(frames, np.int32), torch.int32)
            d_ob = to_dev(base[:-1].copy(), torch.int64)
            for g in range(G):
                _lib.check(lp.lib.amt_istft_ragged(self.batch.plan, ptr(mags[g]), ptr(self.s_ph), ptr(d_fb), ptr(d_tf),
                                                   len(slots), max(frames), self.pool.frames, mags.shape[2], ptr(out[g]),
                                                   ptr(d_ob), int(base[-1]), stream_ptr()))
        return out, base[:-1], lens

    def step(self, max_notes, silence, row, song0=None):
        """One step of the walk for every slot: the loop's _step() (the head sequence of iterate()) with the walk's
        waveform and its slide / detect decision before the subtraction, the step's records into row [slots, 9] (device),
        the slide.  The records' song is song0 + slot, or the slot's own song (slot_song) where song0 is None."""
        lp, b, sp = self.lp, self.batch, stream_ptr()
        p, lib, B = lp.p, lp.lib, self.slots
        tf, ldf = p.timing_frames, b.mag.shape[2]
        half = tf // 2
        lp.refs = self.refs

        def wave_fn():
            # util_audio.py:94-97 for windows that had a subtraction (their _wf is None: the mag setter cleared it, slice
            # and concat keep None); the raw samples section / slice / concat carry along for the others
            _lib.check(lib.amt_istft(b.plan, ptr(b.mag), ptr(b.ph), B, tf, ldf, tf * ldf, ptr(self.wave), self.l_row, sp))
            _lib.check(lib.amt_song_wave(ptr(self.samples), ptr(self.sample_base), ptr(self.seg), B,
                                         int(self.seg.shape[1]), int(self.seg.shape[2]), ptr(self.offset), half,
                                         ptr(self.clean), ptr(self.finished), ptr(self.wave), self.l_row, self.l_row,
                                         p.H * (tf - 1), sp))
            return self.wave

        def decide(onset, end, gfr):
            wmax = empty((B,))
            _lib.check(lib.amt_song_decide(ptr(onset), ptr(b._fmax[0]), B, tf, ptr(self.refs['ref_mag']), float(silence),
                                           half, int(max_notes), ptr(self.finished), ptr(self.count), ptr(self.clean),
                                           ptr(self.slide), ptr(self.detect), ptr(self.kind), ptr(gfr), ptr(wmax), sp))
            b.ref_max = wmax                                       # np.max(audio_w.mag) at the subtraction (:170-174)

        stem = None
        if self.keep_stems:
            # (_step adds the step's decided programs; without the instrument head everything is stem 0)
            stem = _lib.stem_args(stems=self.stems, frame_base=self.frame_base, offset=self.offset, t_song=self.t_song,
                                  prog_group=lp.prog_group, n_prog=int(lp.prog_group.shape[0]),
                                  G=int(self.stems.shape[0]), pool_frames=self.pool.frames)
        onset, end, pitch, program, velocity = lp._step(b, wave_fn, fmax=True, before_subtract=decide, stems=stem)
        note = (ptr(self.kind), ptr(pitch), ptr(program), ptr(velocity), ptr(onset), ptr(end), ptr(self.offset),
                ptr(row), sp)
        if song0 is None:
            _lib.check(lib.amt_song_pack_events_slots(B, ptr(self.slot_song), self.steps, *note))
        else:
            _lib.check(lib.amt_song_pack_events(B, int(song0), self.steps, *note))
        slide = lib.amt_song_slide_keep if self.keep_residual else lib.amt_song_slide
        _lib.check(slide(ptr(b.mag), ptr(b.ph), B, tf, ldf, tf * ldf, ptr(self.s_mag), ptr(self.s_ph),
                         ptr(self.frame_base), ptr(self.t_song), ptr(self.slide), ptr(self.offset), ptr(self.count),
                         ptr(self.finished), sp))
        b._fmax = None                                             # the slid windows' per-frame maxima are stale
        self.steps += 1


def prepare_songs(lp, songs, refs=None, spectra=None, song0=0, keep_residual=False, keep_stems=False):
    """A fixed batch: as many slots as songs, a pool of exactly their frames, ONE admission of song i into slot i."""
    waves = [check_song(lp.p, s) for s in songs]
    if not waves:
        raise ValueError('run_songs: no songs given')
    st = SongState(lp, len(waves), sum(1 + w.numel() // lp.p.H for w in waves), keep_residual=keep_residual,
                   keep_stems=keep_stems)
    st.admit([(i, int(song0) + i, w) for i, w in enumerate(waves)], refs=refs, spectra=spectra)
    return st


def walk_songs(st, max_notes, silence, poll=16, song0=0, max_steps=None, residual=False, stems=False):
    """Steps a fixed batch to its end (or max_steps) with nothing read back but finished.sum() every `poll` steps.
    residual (a state with keep_residual): afterwards st.residual = one entry per slot, the finished songs' residual
    waveforms from ONE residual_waves() call, None for a song the walk left unfinished.
    stems (a state with keep_stems): afterwards st.stem_audio = one entry per slot, the finished songs' [G, samples]
    stem waveforms from ONE stem_waves() call, None for an unfinished song.
    Returns events [steps, slots, 9] int32 (device), FINISHED records of idle slots included."""
    if residual and not st.keep_residual:
        raise ValueError('walk_songs: residual needs a state prepared with keep_residual')
    if stems and not st.keep_stems:
        raise ValueError('walk_songs: stems need a state prepared with keep_stems')
    B = st.slots
    st.bound = st.positions * (int(max_notes) + 1)
    if max_steps is not None:
        st.bound = min(st.bound, int(max_steps))
    events = empty((st.bound, B, len(SONG_EVENT_FIELDS)), torch.int32)
    st.steps = 0
    while st.steps < st.bound:
        st.step(max_notes, silence, events[st.steps], song0)
        if st.steps % max(int(poll), 1) == 0 and int(st.finished.sum()) == B:
            break
    if residual or stems:
        fin = st.finished.cpu().numpy()
        done = [b for b in range(B) if fin[b] and st.region[b] is not None]
    if residual:
        st.residual = [None] * B
        for b, w in zip(done, st.residual_waves(done)):
            st.residual[b] = w
    if stems:
        st.stem_audio = [None] * B
        for b, w in zip(done, st.stem_waves(done)):
            st.stem_audio[b] = w
    return events[:st.steps]


def iter_song_queue(lp, songs, slots, max_notes, silence, poll=16, pool_frames=None, on_finish=None, residual=False,
                    stems=False):
    """Pulls and checks the first `slots` songs (no song at all is an error of the call, not of the first next()) and
    returns the generator of the queue's walk."""
    p, B, poll = lp.p, int(slots), max(int(poll), 1)
    it, ahead, pulled = iter(songs), [], [0]

    def pull(n):
        """Songs waiting for a slot: up to n, checked when they are pulled."""
        while len(ahead) < n:
            w = next(it, None)
            if w is None:
                break
            ahead.append((pulled[0], check_song(p, w)))
            pulled[0] += 1

    pull(B)
    if not ahead:
        raise ValueError('run_songs: no songs given')
    if pool_frames is None:
        pool_frames = B * max(1 + w.numel() // p.H for _, w in ahead)

    def walk():
        st = SongState(lp, B, pool_frames, keep_residual=residual, keep_stems=stems)
        stats = lp.queue_stats = st.stats
        chunk = empty((poll, B, len(SONG_EVENT_FIELDS)), torch.int32)
        host_chunk = torch.empty(tuple(chunk.shape), dtype=torch.int32, pin_memory=True)
        host_fin = torch.empty((B,), dtype=torch.int32, pin_memory=True)
        records = {}

        def admit():
            free = [s < 0 for s in st.song_of]
            pull(sum(free))
            plan = admission_plan(free, ahead[0][0] if ahead else pulled[0], len(ahead))
            got = st.admit([(slot, idx, ahead[j][1]) for j, (slot, idx) in enumerate(plan)])
            stats['waits'] += len(got) < len(plan)
            for (_, idx), positions in zip(plan, got):
                records[idx] = []
                stats['bound'] += -(-(positions * (int(max_notes) + 1)) // poll) * poll
            del ahead[:len(got)]

        admit()
        while any(s >= 0 for s in st.song_of):
            for r in range(poll):
                st.step(max_notes, silence, chunk[r])
            host_chunk.copy_(chunk, non_blocking=True)
            host_fin.copy_(st.finished, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            ev = host_chunk.numpy()
            stats['steps'] = st.steps
            kinds = np.bincount(ev[:, :, 2].ravel(), minlength=4)
            for k in range(4):
                stats['slot_steps'][k] += int(kinds[k])
            done = []
            for slot, idx in enumerate(st.song_of):
                if idx < 0:
                    continue
                rows = ev[:, slot, :]
                records[idx].append(rows[rows[:, 2] != SONG_FINISHED].copy())
                if host_fin[slot]:
                    done.append((slot, idx))
            # the residual of every song found finished here, in ONE launch, enqueued BEFORE any region is released:
            # on the walk's stream it runs ahead of the STFT a later admission writes into such a region
            # (and their stems likewise: the zeroing of a later admission follows on the same stream)
            waves = st.residual_waves([slot for slot, _ in done]) if residual and done else []
            stem_w = st.stem_waves([slot for slot, _ in done]) if stems and done else []
            for k, (slot, idx) in enumerate(done):
                if on_finish is not None:
                    on_finish(idx, slot, st)
                out = np.concatenate(records.pop(idx))
                out[:, 1] = np.arange(len(out))
                st.release(slot)
                yield (idx, out) + ((waves[k],) if residual else ()) + ((stem_w[k],) if stems else ())
            admit()
            if st.steps > stats['bound']:
                raise RuntimeError('run_song_queue: %d steps, past the bound of the admitted songs (%d)'
                                   % (st.steps, stats['bound']))

    return walk()
