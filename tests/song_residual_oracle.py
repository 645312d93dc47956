"""Test infrastructure: the residual spectrogram of a song walk -- what every subtraction left of the song -- assembled
from the CPU restatement's own output (tests/song_oracle.SongOracle.run_song(..., windows=[...]) and its events).  It does
not import the product.

A half window leaves the live window at every slide.  At a slide record of step s the outgoing half is the first `half`
columns of the window as it was BEFORE the slide, i.e. after step s - 1 (for s = 0: section(0, None, timing_frames) of the
song, training.py:284); it holds song frames [offset, offset + half) of that record, cropped to the song's frames (later
columns are the window's zero padding).  The walk ends once offset >= frames (training.py:296), so every frame below
t_song must have left exactly once."""
import numpy as np

SLIDE, FORCED_SLIDE = 1, 2


def assemble_residual(song, events, windows, timing_frames):
    """song: oracle.audio.AudioCompleteOracle of the whole song; events [steps, 9] and windows (one [F, >= T] array per
    step) as run_song returns / fills them.  Returns the residual magnitudes [F, t_song] float32."""
    tf = int(timing_frames)
    half = tf // 2
    song.mag                                                       # as run_song: section() then cuts the song's own STFT
    t_song = song.shape[1]
    first = np.asarray(song.section(0, None, tf).mag)
    out = np.zeros((first.shape[0], t_song), np.float32)
    seen = np.zeros(t_song, np.int64)
    events = np.asarray(events).reshape(-1, 9)
    assert len(windows) == len(events)
    for s, e in enumerate(events):
        if e[2] not in (SLIDE, FORCED_SLIDE):
            continue
        before = first if s == 0 else np.asarray(windows[s - 1])
        off = int(e[8])
        n = int(np.clip(t_song - off, 0, half))
        out[:, off:off + n] = before[:, :n]
        seen[off:off + n] += 1
    assert np.all(seen == 1), 'every frame below t_song leaves the window exactly once: %s' % np.flatnonzero(seen != 1)
    return out
