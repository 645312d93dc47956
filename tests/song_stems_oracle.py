"""Test infrastructure: the instrument stems of a song walk -- what every subtraction took out of the song, per
instrument group -- assembled from the CPU restatement's own output (tests/song_oracle.SongOracle.run_song(...,
windows=[...]) and its events).  It does not import the product.

A DETECT record of step s stands for one subtraction on the live window: the window before it is windows[s - 1] (for
s = 0: section(0, None, timing_frames) of the song, training.py:284), the window after it windows[s], and what the step
removed is before - after, element by element in float32 -- the clipped amount, since after = max(before - guess, 0)
(util_audio.py:250-259).  Window column t is song frame offset_frame + t; columns at or past the song's frames are the
window's zero padding and belong to no stem.  The record's stem is prog_group[clamp(program)], the clamp of
tests/features_reference.note_select, the group clamped into [0, G); without a table (a walk without the instrument head)
everything is stem 0."""
import numpy as np

DETECT = 0


def stem_of(program, prog_group, G):
    """The stem index of a decided program: prog_group[clamp(program, 0, n_prog - 1)] clamped into [0, G); 0 without a
    table."""
    if prog_group is None:
        return 0
    pr = min(max(int(program), 0), len(prog_group) - 1)
    return min(max(int(prog_group[pr]), 0), int(G) - 1)


def assemble_stems(song, events, windows, timing_frames, prog_group, G):
    """song: oracle.audio.AudioCompleteOracle of the whole song; events [steps, 9] and windows (one [F, >= T] array per
    step) as run_song returns / fills them; prog_group: int array [n_prog] of stem indices, or None (stem 0).
    Returns (stems [G, F, t_song] float32, covered [G, t_song] bool: the song frames the DETECT records of each group
    reach -- every frame of the window from the record's onset on, an upper bound of what its guess touches)."""
    tf = int(timing_frames)
    song.mag                                                       # as run_song: section() then cuts the song's own STFT
    t_song = song.shape[1]
    first = np.asarray(song.section(0, None, tf).mag, np.float32)
    stems = np.zeros((int(G), first.shape[0], t_song), np.float32)
    covered = np.zeros((int(G), t_song), bool)
    events = np.asarray(events).reshape(-1, 9)
    assert len(windows) == len(events)
    for s, e in enumerate(events):
        if e[2] != DETECT:
            continue
        before = first if s == 0 else np.asarray(windows[s - 1], np.float32)
        after = np.asarray(windows[s], np.float32)
        off = int(e[8])
        n = int(np.clip(t_song - off, 0, tf))
        g = stem_of(e[4], prog_group, G)
        removed = before[:, :n] - after[:, :n]                     # float32, as the product rounds it
        stems[g][:, off:off + n] = stems[g][:, off:off + n] + removed
        covered[g, min(int(e[6]), t_song):off + n] = True          # onset_frame is a song frame
    return stems, covered
