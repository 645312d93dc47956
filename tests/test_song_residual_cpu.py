"""CPU: the residual of a song walk as the restatement defines it (tests/song_residual_oracle.py over
tests/song_oracle.py) on cases with a known answer, and the argument checks of the residual options that need no
device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import song_oracle as so                                        # noqa: E402
import song_residual_oracle as sro                              # noqa: E402


def _params():
    from amt_saga.hyperparams import Hyperparams
    return Hyperparams(N=2048, window_size_note_time=1)          # 86 frames, half = 43


@pytest.mark.parametrize('hops', [200, 30, 128, 129, 85])
def test_nothing_detected_residual_is_the_song(hops):
    """Onsets always in the second half: nothing is ever subtracted, and the halves that leave the window are the
    song's own frames -- every one of them, once, bit for bit; also for a song shorter than half a window and for songs
    ending on a half boundary."""
    from oracle import audio as oa
    p = _params()
    rng = np.random.default_rng(hops)
    wave = (rng.standard_normal(p.H * hops + 37) * 0.1).astype(np.float32)
    orc = so.SongOracle(p, ('timing',), {}, subtract=False,
                        predict=lambda name, step: 60.0 if name == 'timing_start' else 80.0)
    wins = []
    ev, _ = orc.run_song(wave, {'ref_mag': 1.0}, max_notes=3, silence=0.0, windows=wins)
    song = oa.AudioCompleteOracle(wave, p.N, p.H)
    res = sro.assemble_residual(song, ev, wins, p.timing_frames)
    assert res.shape == (p.N // 2 + 1, 1 + len(wave) // p.H)
    assert np.array_equal(res, np.asarray(song.mag, np.float32))


def test_scripted_detections_leave_less_than_the_song():
    """Scripted detections with a subtraction each: the residual lies between 0 and the song's spectrogram everywhere,
    below it somewhere, and equals it on the frames no guess reached."""
    from oracle import audio as oa
    p = _params()
    rng = np.random.default_rng(3)
    wave = (rng.standard_normal(p.H * 215) * 0.1).astype(np.float32)
    guess = (rng.standard_normal(p.H * 12) * 0.1).astype(np.float32)
    script = [10, 12, 9, 50, 5, 70, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3]
    orc = so.SongOracle(p, ('timing',), {}, subtract=True, guess_fn=lambda *a: guess,
                        predict=lambda name, step: float(script[step]) if name == 'timing_start' else 80.0)
    wins = []
    ev, _ = orc.run_song(wave, {'ref_mag': 1.0}, max_notes=2, silence=0.0, windows=wins)
    assert np.sum(ev[:, 2] == so.DETECT) >= 4
    song = oa.AudioCompleteOracle(wave, p.N, p.H)
    res = sro.assemble_residual(song, ev, wins, p.timing_frames)
    full = np.asarray(song.mag, np.float32)
    assert res.shape == full.shape and np.all(res >= 0) and np.all(res <= full) and np.any(res < full)
    touched = np.zeros(full.shape[1], bool)
    for e in ev[ev[:, 2] == so.DETECT]:
        touched[e[6]:e[6] + 13 + 80] = True                         # no guess is longer than its 13 frames
    assert np.any(~touched) and np.array_equal(res[:, ~touched], full[:, ~touched])


def test_oracle_helper_refuses_a_walk_that_is_not_over():
    from oracle import audio as oa
    p = _params()
    wave = (np.random.default_rng(5).standard_normal(p.H * 200) * 0.1).astype(np.float32)
    orc = so.SongOracle(p, ('timing',), {}, subtract=False, predict=lambda name, step: 60.0)
    wins = []
    ev, _ = orc.run_song(wave, {'ref_mag': 1.0}, max_notes=3, silence=0.0, max_steps=2, windows=wins)
    with pytest.raises(AssertionError):
        sro.assemble_residual(oa.AudioCompleteOracle(wave, p.N, p.H), ev, wins, p.timing_frames)


def test_residual_arguments_without_a_device(tmp_path):
    """The checks that come before any device set-up: the window traversal has no song-level residual, the command line
    says so before it reads a file, and the new keywords exist where the documentation puts them."""
    import inspect
    from amt_saga import loop, song_walk, transcribe as tr
    with pytest.raises(ValueError, match='residual'):
        tr.transcribe(np.zeros(4096, np.float32), traversal='windows', residual=True)
    with pytest.raises(ValueError, match='residual'):
        tr.transcribe(np.zeros(4096, np.float32), residual=True)    # 'windows' is the default
    missing = str(tmp_path / 'missing.flac')
    with pytest.raises(SystemExit, match='--traversal song'):
        tr.main([missing, str(tmp_path / 'o.mid'), '--residual', str(tmp_path / 'r.flac')])
    with pytest.raises(SystemExit, match='--traversal song'):
        tr.main([missing, str(tmp_path / 'o.mid'), '--residual', str(tmp_path / 'r.flac'), '--traversal', 'windows'])
    assert not os.path.exists(str(tmp_path / 'r.flac'))
    for fn, kw in ((song_walk.SongState.__init__, 'keep_residual'), (song_walk.prepare_songs, 'keep_residual'),
                   (song_walk.walk_songs, 'residual'), (song_walk.iter_song_queue, 'residual'),
                   (loop.TranscriptionLoop.run_songs, 'residual'), (loop.TranscriptionLoop.iter_song_queue, 'residual'),
                   (loop.TranscriptionLoop.run_song_queue, 'residual'), (tr.transcribe, 'residual'),
                   (tr.iter_transcribe_songs, 'residual')):
        par = inspect.signature(fn).parameters[kw]
        assert par.default is False, (fn.__qualname__, kw)          # off by default: every existing call is unchanged
    assert callable(song_walk.SongState.residual_waves)


def test_entry_points_declared_and_bound():
    from amt_saga import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'amt_saga.h')).read()
    for name in ('amt_song_slide_keep', 'amt_istft_ragged'):
        assert name in _lib.PROTOTYPES and ('int %s(' % name) in header
    assert len(_lib.PROTOTYPES['amt_istft_ragged'][1]) == 13
    assert _lib.PROTOTYPES['amt_song_slide_keep'] == _lib.PROTOTYPES['amt_song_slide']
