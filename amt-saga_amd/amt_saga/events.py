"""Note-event assembly and Standard MIDI File output.

The loop emits fixed-size records per window and iteration
    {window, iter, pitch, program, velocity, onset_frame, end_frame}      (int32 x 7)
This module turns them into a song-level note list and writes it as a MIDI
file -- the step the reference does with ``note_sequence.add_note`` / ``save``
(util_audio.py:594-639, 790-792; magenta / pretty_midi, neither available here)
after the sliding-window advance of training.py:317-328 (6-s windows moved by
half a window).  Host-side, plain Python: a few hundred integers per song.

  * frames -> seconds is the reference's own map (util_audio.py:269-272):
        t = frames / T / sr * len(wf)
    shifted by the window's start inside the song;
  * notes that the 50 %-overlapped windows both report (same pitch and program,
    onsets within `merge_tol_s`) are merged, keeping the longer one;
  * the file is SMF format 1, 480 ticks per quarter at 120 bpm (1 tick = 1/960 s),
    one track per program (channels 0-15 round-robin, skipping 9 = drums);
  * given the beats of amt_saga.beat, write_midi writes a tempo map instead (tempo_anchors): every beat on a multiple
    of 480 ticks, time 0 on tick 0, note times unchanged in seconds to within half a tick plus the tempo rounding.
"""
import struct

import numpy as np

TICKS_PER_QUARTER = 480
TEMPO_US_PER_QUARTER = 500000            # 120 bpm
TICKS_PER_SECOND = TICKS_PER_QUARTER * 1e6 / TEMPO_US_PER_QUARTER


def frames_to_seconds(frames, n_frames, n_samples, sr):
    """audio_complete._frames_to_seconds (util_audio.py:269-272)."""
    return np.asarray(frames, dtype=np.float64) / n_frames / sr * n_samples


def events_to_notes(events, n_frames, n_samples, sr=44100, window_start_s=None, hop_windows_s=None):
    """events: int array [..., 7] (any leading shape).  window_start_s[w] gives the
    start of window w in the song (default: w * hop_windows_s, default hop = half a
    window, training.py:317-328).  Returns a list of dicts sorted by start time."""
    ev = np.asarray(events).reshape(-1, 7)
    win_len_s = n_samples / sr
    if hop_windows_s is None:
        hop_windows_s = win_len_s / 2.0
    notes = []
    for w, it, pitch, program, velocity, on, off in ev:
        if pitch < 0 or on < 0:
            continue
        t0 = float(window_start_s[w]) if window_start_s is not None else w * hop_windows_s
        start = t0 + float(frames_to_seconds(on, n_frames, n_samples, sr))
        end = t0 + float(frames_to_seconds(max(off, on + 1), n_frames, n_samples, sr))
        notes.append(dict(pitch=int(pitch), program=int(max(program, 0)),
                          velocity=int(velocity) if velocity > 0 else 64,
                          start=start, end=end, window=int(w), iter=int(it)))
    notes.sort(key=lambda n: (n['start'], n['pitch'], n['program']))
    return notes


def song_events_to_notes(events, song_frames, song_samples, sr=44100):
    """Records of TranscriptionLoop.run_songs -- int array [..., 9] = {song, step, kind, pitch, program, velocity,
    onset_frame, end_frame, offset_frame}, frames counted in the song -- to notes with absolute times.  Only kind 0
    (detect) carries a note.  song_frames / song_samples: frames and samples of the song (or sequences indexed by the
    record's song field); frames -> seconds is the reference's map on the SONG (util_audio.py:269-272).  One live window
    per song sees every frame from one residual only: there are no overlap duplicates to merge."""
    ev = np.asarray(events).reshape(-1, 9)
    notes = []
    for song, step, kind, pitch, program, velocity, on, off, offset in ev:
        if kind != 0 or pitch < 0:
            continue
        T = song_frames[song] if np.ndim(song_frames) else song_frames
        n = song_samples[song] if np.ndim(song_samples) else song_samples
        notes.append(dict(pitch=int(pitch), program=int(max(program, 0)),
                          velocity=int(velocity) if velocity > 0 else 64,
                          start=float(frames_to_seconds(on, T, n, sr)),
                          end=float(frames_to_seconds(max(off, on + 1), T, n, sr)),
                          song=int(song), step=int(step), window=int(offset)))
    notes.sort(key=lambda n: (n['song'], n['start'], n['pitch'], n['program']))
    return notes


def merge_overlap_duplicates(notes, merge_tol_s=0.05):
    """Drop the second report of a note seen by two overlapping windows."""
    out = []
    for n in sorted(notes, key=lambda n: (n['program'], n['pitch'], n['start'])):
        if out:
            m = out[-1]
            if (m['program'] == n['program'] and m['pitch'] == n['pitch'] and
                    m['window'] != n['window'] and abs(m['start'] - n['start']) <= merge_tol_s):
                if n['end'] - n['start'] > m['end'] - m['start']:
                    out[-1] = n
                continue
        out.append(n)
    out.sort(key=lambda n: (n['start'], n['pitch'], n['program']))
    return out


def _vlq(v):
    v = int(v)
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(reversed(out))


QUANTIZE_DIVISIONS = (1, 2, 3, 4, 6, 8, 12)          # grid points per quarter that divide 480 ticks
MAX_TEMPO_US = 0xFFFFFF                              # a set-tempo event holds three bytes


def tempo_anchors(beats):
    """[(seconds, tick)] of a tempo map through the beat times `beats` (seconds, strictly increasing, none negative; at
    least two): it starts at (0, 0) -- nothing is shifted against the audio -- and every beat it keeps falls on a multiple
    of 480 ticks, one quarter per beat.  The lead-in, with i0 = beats[1] - beats[0]: a first beat before i0 / 2 is
    dropped as a grid point ([0, beats[1]) is one quarter); otherwise [0, beats[0]) holds max(1, round(beats[0] / i0))
    quarters."""
    b = [float(t) for t in beats]
    if len(b) < 2 or b[0] < 0 or any(not y > x for x, y in zip(b, b[1:])) or b[-1] == float('inf'):
        raise ValueError('Invalid Input shape. Expected: at least two beat times, >= 0 and strictly increasing . Got: %d'
                         % len(b))
    i0 = b[1] - b[0]
    if b[0] < i0 / 2:
        b, lead = b[1:], 1
    else:
        lead = max(1, int(round(b[0] / i0)))
    return [(0.0, 0)] + [(t, TICKS_PER_QUARTER * (lead + k)) for k, t in enumerate(b)]


def _anchor_tempos(anchors):
    """round(us per quarter) of every anchor's segment, the last anchor repeating the segment before it."""
    tempos = []
    for (s0, k0), (s1, k1) in zip(anchors, anchors[1:]):
        us = int(round((s1 - s0) * 1e6 * TICKS_PER_QUARTER / (k1 - k0)))
        if not 1 <= us <= MAX_TEMPO_US:
            raise ValueError('Invalid Input shape. Expected: beats between 1 us and %.3f s a quarter apart . Got: %.6f s'
                             % (MAX_TEMPO_US * 1e-6, (s1 - s0) * TICKS_PER_QUARTER / (k1 - k0)))
        tempos.append(us)
    return tempos + tempos[-1:]


def _anchor_ticks(anchors):
    """seconds -> tick (a float) by piecewise-linear interpolation through the anchors, the last segment extended."""
    secs = [a[0] for a in anchors]

    def tick(t):
        k = min(max(int(np.searchsorted(secs, t, side='right')) - 1, 0), len(anchors) - 2)
        (s0, k0), (s1, k1) = anchors[k], anchors[k + 1]
        return k0 + (t - s0) * (k1 - k0) / (s1 - s0)
    return tick


def write_midi(notes, path, beats=None, quantize=None):
    """Write the note list as a format-1 Standard MIDI File: 480 ticks per quarter at 120 bpm.
    beats: beat times in seconds (beat.beat_track's).  With at least two, the first track carries the tempo map of
    tempo_anchors(beats) -- one set-tempo event per anchor, round(us per quarter) of the segment it opens -- and note
    ticks come from the interpolation through the anchors, so a beat is a bar-line candidate in a notation program while
    every note keeps its time in seconds to within half a tick plus the tempo rounding.  quantize=DIV (1, 2, 3, 4, 6, 8,
    12) then snaps onsets to 480 / DIV ticks and keeps each duration, at least one tick.  beats=None, an empty list or a
    single beat writes the fixed-tempo file, byte for byte what it was without these arguments (quantize has no grid
    to snap to there and is not applied)."""
    if quantize is not None and not (isinstance(quantize, (int, np.integer)) and not isinstance(quantize, bool)
                                     and quantize in QUANTIZE_DIVISIONS):
        raise ValueError('write_midi: quantize must be one of %s . Got: %r' % (', '.join(map(str, QUANTIZE_DIVISIONS)), quantize))
    mapped = beats is not None and len(beats) >= 2
    if mapped:
        anchors = tempo_anchors(beats)
        tick_of = _anchor_ticks(anchors)
        head, last = b'', 0
        for (_, k), us in zip(anchors, _anchor_tempos(anchors)):
            head += _vlq(k - last) + b'\xff\x51\x03' + struct.pack('>I', us)[1:]
            last = k
        head += b'\x00\xff\x2f\x00'
    else:
        tick_of = lambda t: t * TICKS_PER_SECOND                      # noqa: E731
        head = b'\x00\xff\x51\x03' + struct.pack('>I', TEMPO_US_PER_QUARTER)[1:] + b'\x00\xff\x2f\x00'
    grid = TICKS_PER_QUARTER // int(quantize) if mapped and quantize else 0
    programs = sorted({n['program'] for n in notes})
    chans = [c for c in range(16) if c != 9]
    tracks = [head]
    for i, prog in enumerate(programs):
        ch = chans[i % len(chans)]
        evs = []
        for n in notes:
            if n['program'] != prog:
                continue
            t_on = max(int(round(tick_of(n['start']))), 0) if mapped else int(round(tick_of(n['start'])))
            t_off = max(int(round(tick_of(n['end']))), t_on + 1)
            if grid:
                snapped = (2 * t_on + grid) // (2 * grid) * grid       # the nearest grid point, a tie upwards
                t_on, t_off = snapped, snapped + (t_off - t_on)
            evs.append((t_on, 1, bytes([0x90 | ch, n['pitch'] & 0x7F, min(max(n['velocity'], 1), 127)])))
            evs.append((t_off, 0, bytes([0x80 | ch, n['pitch'] & 0x7F, 0])))
        evs.sort(key=lambda e: (e[0], e[1]))
        data = b'\x00' + bytes([0xC0 | ch, prog & 0x7F])
        last = 0
        for t, _, msg in evs:
            data += _vlq(t - last) + msg
            last = t
        data += b'\x00\xff\x2f\x00'
        tracks.append(data)
    with open(path, 'wb') as f:
        f.write(b'MThd' + struct.pack('>IHHH', 6, 1, len(tracks), TICKS_PER_QUARTER))
        for t in tracks:
            f.write(b'MTrk' + struct.pack('>I', len(t)) + t)


def _read_vlq(buf, i):
    v = 0
    while True:
        b = buf[i]; i += 1
        v = (v << 7) | (b & 0x7F)
        if not b & 0x80:
            return v, i


def _tempo_seconds(tempos, div):
    """tick -> seconds under a tempo map: tempos = [(tick, us per quarter)] from every track, in file order.  120 bpm
    holds until the first event; of two events on one tick the later one in the file holds."""
    marks = [(0, TEMPO_US_PER_QUARTER)] + sorted(tempos, key=lambda m: m[0])         # (stable: file order within a tick)
    ticks, rates, starts = [], [], []
    for tick, tempo in marks:
        if ticks and tick == ticks[-1]:
            rates[-1] = tempo
            continue
        starts.append(starts[-1] + (tick - ticks[-1]) * rates[-1] / float(div) * 1e-6 if ticks else 0.0)
        ticks.append(tick)
        rates.append(tempo)

    def seconds(t):
        k = int(np.searchsorted(ticks, t, side='right')) - 1
        return starts[k] + (t - ticks[k]) * rates[k] / float(div) * 1e-6
    return seconds


def read_midi(path, full=False):
    """Standard MIDI File reader for the note content note_sequence.save() / write_midi produce:
    format 0/1, ticks-per-quarter division, set-tempo meta events (the first tempo applies to the whole
    file, as in the single-tempo files magenta writes), running status, note-on with velocity 0 as
    note-off, program changes.  Returns notes sorted by start time (seconds).
    full=True (gold files, whose tempo changes): every set-tempo event of every track is honoured -- one tempo map for
    the file, as format 1 keeps it -- and each note also carries its `channel`."""
    data = open(path, 'rb').read()
    if data[:4] != b'MThd':
        raise ValueError('not a Standard MIDI File')
    _, fmt, ntr, div = struct.unpack('>IHHH', data[4:14])
    if div & 0x8000:
        raise ValueError('SMPTE time division is not supported')
    pos = 14
    raw_notes = []
    tempo = None
    tempos = []
    for _ in range(ntr):
        if data[pos:pos + 4] != b'MTrk':
            raise ValueError('missing MTrk chunk')
        ln = struct.unpack('>I', data[pos + 4:pos + 8])[0]
        trk = data[pos + 8:pos + 8 + ln]
        pos += 8 + ln
        i, t, status = 0, 0, 0
        prog = {}
        open_notes = {}
        while i < len(trk):
            d, i = _read_vlq(trk, i)
            t += d
            if trk[i] & 0x80:
                status = trk[i]; i += 1
            if status == 0xFF:                                   # meta event
                typ = trk[i]
                ln2, i = _read_vlq(trk, i + 1)
                if typ == 0x51 and tempo is None:
                    tempo = int.from_bytes(trk[i:i + 3], 'big')
                if typ == 0x51:
                    tempos.append((t, int.from_bytes(trk[i:i + 3], 'big')))
                i += ln2
                continue
            if status in (0xF0, 0xF7):                           # sysex
                ln2, i = _read_vlq(trk, i)
                i += ln2
                continue
            hi, ch = status & 0xF0, status & 0x0F
            if hi == 0xC0:
                prog[ch] = trk[i]; i += 1
            elif hi == 0xD0:
                i += 1
            elif hi in (0x90, 0x80):
                p, v = trk[i], trk[i + 1]; i += 2
                if hi == 0x90 and v > 0:
                    open_notes.setdefault((ch, p), []).append((t, v))
                elif open_notes.get((ch, p)):
                    t0, v0 = open_notes[(ch, p)].pop(0)     # overlapping same-pitch notes: FIFO
                    raw_notes.append((p, prog.get(ch, 0), v0, t0, t, ch))
            else:
                i += 2
    if full:
        seconds = _tempo_seconds(tempos, div)
        notes = [dict(pitch=p, program=pr, velocity=v, start=seconds(t0), end=seconds(t1), channel=ch)
                 for p, pr, v, t0, t1, ch in raw_notes]
        notes.sort(key=lambda n: (n['start'], n['pitch'], n['program']))
        return notes
    us_per_tick = (tempo if tempo is not None else TEMPO_US_PER_QUARTER) / float(div)
    notes = [dict(pitch=p, program=pr, velocity=v, start=t0 * us_per_tick * 1e-6, end=t1 * us_per_tick * 1e-6)
             for p, pr, v, t0, t1, _ in raw_notes]
    notes.sort(key=lambda n: (n['start'], n['pitch'], n['program']))
    return notes
