"""CPU: the restatement of the song walk (tests/song_oracle.py) on cases with a known answer -- the networks replaced
by scripted onsets, so the sequence of offsets, slides, forced slides and the finishing step is exact -- and the
product's host-side table of the window's raw samples against what audio_complete.wf carries through section / slice /
concat."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import song_oracle as so                                        # noqa: E402


def _params():
    from amt_saga.hyperparams import Hyperparams
    return Hyperparams(N=2048, window_size_note_time=1)          # 86 frames, half = 43


def _oracle(p, script, end=80):
    def predict(name, step):
        return float(script[step]) if name == 'timing_start' else float(end)
    return so.SongOracle(p, ('timing',), {}, subtract=False, predict=predict)


def test_slides_only_window_is_a_section_of_the_song():
    """Onsets always in the second half: every step slides; after k slides without a subtraction the window equals
    section(k * half, None, timing_frames) of the song, magnitudes and phases bit for bit; the walk ends when the offset
    passes the song's last frame."""
    from oracle import audio as oa
    p = _params()
    tf, half = p.timing_frames, p.timing_frames // 2
    rng = np.random.default_rng(1)
    wave = (rng.standard_normal(p.H * 200 + 37) * 0.1).astype(np.float32)        # 201 frames: 4.67 half windows
    orc = _oracle(p, [60] * 20)
    wins = []
    ev, _ = orc.run_song(wave, {'ref_mag': 1.0}, max_notes=3, silence=0.0, song_id=4, windows=wins)
    assert ev.shape == (5, 9)
    assert ev[:, 2].tolist() == [so.SLIDE] * 5
    assert ev[:, 8].tolist() == [0, 43, 86, 129, 172]                              # 215 >= 201: finished
    assert ev[:, 6].tolist() == [60, 103, 146, 189, 232] and ev[:, 0].tolist() == [4] * 5
    assert np.all(ev[:, 3:6] == -1)
    song = oa.AudioCompleteOracle(wave, p.N, p.H)
    song.mag
    for k in range(1, 5):                                            # the windows the walk goes on to use
        want = song.section(so.SongOracle.seconds_of_frame(song, k * half), None, tf)
        assert want.mag.shape == (p.N // 2 + 1, tf)
        # a section that STARTS past the song's last frame comes back (end - frames) columns wide, not `half`
        # (util_audio.py:311-316 pads by the distance to the song's end): the class then carries extra zero columns
        # behind the window, which the next slice drops again
        assert np.array_equal(wins[k - 1][:, :tf], want.mag), k
        assert np.all(wins[k - 1][:, tf:] == 0)
    assert np.all(wins[3][:, 201 - 172:] == 0) and np.any(wins[3][:, :201 - 172] != 0)   # zero past the song's end
    assert np.all(wins[4] == 0)


def test_scripted_walk_detects_forced_slides_and_silence():
    p = _params()
    rng = np.random.default_rng(2)
    wave = np.zeros(p.H * 215, np.float32)                         # 216 frames; audible up to frame ~100, then silence
    wave[:p.H * 100] = (rng.standard_normal(p.H * 100) * 0.1).astype(np.float32)
    script = [10, 12, 9,        # two detects, then count == max_notes: forced slide       offset 0
              50,               # onset in the second half: slide                          offset 43
              5, 70,            # detect, slide                                            offset 86
              3, 3, 3, 3, 3]    # silent windows: forced slides until the end              offset 129 ...
    orc = _oracle(p, script)
    ev, _ = orc.run_song(wave, {'ref_mag': 1.0}, max_notes=2, silence=1e-6, song_id=0)
    kinds = [so.DETECT, so.DETECT, so.FORCED_SLIDE, so.SLIDE, so.DETECT, so.SLIDE, so.FORCED_SLIDE, so.FORCED_SLIDE,
             so.FORCED_SLIDE]
    assert ev[:, 2].tolist() == kinds
    assert ev[:, 8].tolist() == [0, 0, 0, 43, 86, 86, 129, 172, 215]               # 258 >= 216: finished after 9 steps
    assert ev[:, 6].tolist() == [10, 12, 9, 93, 91, 156, 132, 175, 218]
    assert ev[:, 7].tolist() == [o + 80 for o in ev[:, 8].tolist()]
    assert ev[[0, 1, 4], 3].tolist() == [60, 60, 60] and np.all(ev[[2, 3, 5, 6, 7, 8], 3] == -1)
    padded = so.pad_finished(ev, 12, 0, 43)
    assert padded.shape == (12, 9) and padded[9:, 2].tolist() == [so.FINISHED] * 3 and padded[9:, 8].tolist() == [258] * 3
    # a song shorter than one window: one position per half window it touches, zero padded
    short = so.SongOracle(p, ('timing',), {}, subtract=False, predict=lambda n, s: 60.0)
    ev2, w2 = short.run_song(wave[:p.H * 30], {'ref_mag': 1.0}, max_notes=2, silence=0.0)
    assert ev2[:, 8].tolist() == [0] and ev2[:, 2].tolist() == [so.SLIDE] and np.all(w2 == 0)


@pytest.mark.parametrize('n_fft,wsec,lens', [
    (2048, 1, [512 * 85]), (2048, 1, [512 * 200 + 37]), (2048, 1, [512 * 30]), (2048, 1, [512 * 129]),
    (2048, 1, [512 * 128 + 511]),
    (2048, 1, [512 * 85, 512 * 30, 512 * 200 + 37, 512 * 129]),                       # one call, songs of unequal length
    (4096, 2, [1024 * 171, 1024 * 300 + 5, 1024 * 90, 1024 * 258]),                   # 172 frames, half = 86
])
def test_raw_sample_table_matches_the_class(n_fft, wsec, lens):
    """amt_saga.loop.song_wave_segments (the host table behind amt_song_wave) against AudioCompleteOracle: while nothing
    has been subtracted, the window's wf after k slides is exactly the listed song samples, zeros elsewhere."""
    from amt_saga.hyperparams import Hyperparams
    from amt_saga.loop import song_wave_segments                  # needs run_songs' module-level helper
    from oracle import audio as oa
    p = Hyperparams(N=n_fft, window_size_note_time=wsec)
    tf, half = p.timing_frames, p.timing_frames // 2
    waves = [(np.arange(1, n + 1) % 8191 + 1 + i).astype(np.float32) for i, n in enumerate(lens)]   # no zero sample
    t_song = [1 + n // p.H for n in lens]
    K = max(-(-T // half) for T in t_song)
    seg, l_row = song_wave_segments(lens, t_song, tf, p.sr, K, min_len=tf * p.H)
    assert seg.shape[:2] == (len(lens), K) and l_row >= tf * p.H
    for i, wave in enumerate(waves):
        song = oa.AudioCompleteOracle(wave, p.N, p.H)
        song.mag
        assert song.shape[1] == t_song[i]
        W = song.section(0, None, tf)
        offset = 0
        for k in range(-(-t_song[i] // half)):
            row = np.zeros(max(l_row, len(W.wf)), np.float64)
            for d, s, n in seg[i, k]:
                assert s + n <= len(wave)
                row[d:d + n] = wave[s:s + n]
            assert np.array_equal(row[:len(W.wf)], np.asarray(W.wf, np.float64)), (i, k)
            assert np.all(row[len(W.wf):] == 0)
            assert np.all(np.asarray(W.wf)[l_row:] == 0)                           # nothing audible is cut off
            offset += half
            new = song.section(so.SongOracle.seconds_of_frame(song, offset + half), None, half)
            W.slice(half, 2 * half)
            W.concat(new)


def test_run_songs_is_part_of_the_loop_interface():
    from amt_saga import loop
    assert loop.SONG_EVENT_FIELDS == ('song', 'step', 'kind', 'pitch', 'program', 'velocity', 'onset_frame',
                                      'end_frame', 'offset_frame')
    assert (loop.SONG_DETECT, loop.SONG_SLIDE, loop.SONG_FORCED_SLIDE, loop.SONG_FINISHED) == \
        (so.DETECT, so.SLIDE, so.FORCED_SLIDE, so.FINISHED)
    assert callable(loop.TranscriptionLoop.run_songs)
