"""CPU: the instrument stems of a song walk as the restatement defines them (tests/song_stems_oracle.py over
tests/song_oracle.py) on cases with a known answer -- above all the identity STFT magnitude = residual + sum of stems
within its derived rounding bound -- and the argument checks of the stem options that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import song_oracle as so                                        # noqa: E402
import song_residual_oracle as sro                              # noqa: E402
import song_stems_oracle as sso                                 # noqa: E402

U = 2.0 ** -24                                                  # unit roundoff of float32


def identity_bound(orig, max_notes):
    """|orig - (residual + sum of stems)| <= (2 max_notes + 2) u orig, elementwise, evaluated in float64.  The residual
    of an element only decreases, so the exact removed amounts telescope to orig - residual; their float32 roundings sum
    to at most u orig; each of the n accumulations adds at most u orig; a frame sits in the window for at most two
    positions of at most max_notes detections each, n <= 2 max_notes; one more unit for the second-order terms."""
    return (2 * int(max_notes) + 2) * U * np.asarray(orig, np.float64)


def _params():
    from amt_saga.hyperparams import Hyperparams
    return Hyperparams(N=2048, window_size_note_time=1)          # 86 frames, half = 43


class ScriptedPrograms(so.SongOracle):
    """The scripted-detection set-up with a scripted instrument decision: the program of step s is programs[s]."""
    programs = ()

    def _detect(self, ac, refs, onset, end):
        pitch, _, velocity = super()._detect(ac, refs, onset, end)
        return pitch, int(self.programs[self._it % len(self.programs)]), velocity


@pytest.mark.parametrize('hops', [200, 30, 129])
def test_nothing_detected_stems_are_zero(hops):
    """Onsets always in the second half: no DETECT record, every stem exactly zero (and nothing covered)."""
    from oracle import audio as oa
    p = _params()
    wave = (np.random.default_rng(hops).standard_normal(p.H * hops + 37) * 0.1).astype(np.float32)
    orc = so.SongOracle(p, ('timing',), {}, subtract=False,
                        predict=lambda name, step: 60.0 if name == 'timing_start' else 80.0)
    wins = []
    ev, _ = orc.run_song(wave, {'ref_mag': 1.0}, max_notes=3, silence=0.0, windows=wins)
    song = oa.AudioCompleteOracle(wave, p.N, p.H)
    stems, covered = sso.assemble_stems(song, ev, wins, p.timing_frames, np.array([0, 1, 2], np.int32), 3)
    assert stems.shape == (3, p.N // 2 + 1, 1 + len(wave) // p.H) and stems.dtype == np.float32
    assert not stems.any() and not covered.any()


def _scripted(max_notes=2):
    from oracle import audio as oa
    p = _params()
    rng = np.random.default_rng(3)
    wave = (rng.standard_normal(p.H * 215) * 0.1).astype(np.float32)
    guess = (rng.standard_normal(p.H * 12) * 0.1).astype(np.float32)
    script = [10, 12, 9, 50, 5, 70, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3]
    orc = ScriptedPrograms(p, ('timing',), {}, subtract=True, guess_fn=lambda *a: guess,
                           predict=lambda name, step: float(script[step]) if name == 'timing_start' else 80.0)
    # programs below, inside and past the table (stems 0, 2, 1, and 1 for those past it); consecutive steps share a
    # group, so overlapping guesses accumulate in one stem
    orc.programs = [1, 1, -1, 7, 0, 0, 9, 9, 2, 2, 1, 0, 0, 9, 0, 1]
    table = np.array([0, 2, 1, 1], np.int32)
    wins = []
    ev, _ = orc.run_song(wave, {'ref_mag': 1.0}, max_notes=max_notes, silence=0.0, windows=wins)
    song = oa.AudioCompleteOracle(wave, p.N, p.H)
    return p, song, ev, wins, table


def test_identity_residual_plus_stems_is_the_song():
    """Scripted detections over three groups: residual (assemble_residual) + sum of stems is the song's spectrogram
    within the derived bound, elementwise; every stem >= 0; something was removed in at least two groups."""
    max_notes = 2
    p, song, ev, wins, table = _scripted(max_notes)
    det = ev[ev[:, 2] == so.DETECT]
    groups = {sso.stem_of(e[4], table, 3) for e in det}
    assert len(det) >= 4 and len(groups) >= 2
    res = sro.assemble_residual(song, ev, wins, p.timing_frames)
    stems, _ = sso.assemble_stems(song, ev, wins, p.timing_frames, table, 3)
    full = np.asarray(song.mag, np.float32)
    assert np.all(stems >= 0)
    assert sum(bool(stems[g].any()) for g in range(3)) >= 2
    gap = np.abs(full.astype(np.float64) - (res.astype(np.float64) + stems.astype(np.float64).sum(axis=0)))
    bound = identity_bound(full, max_notes)
    print('identity: largest gap / bound %.3f, largest gap %.3e' % (float((gap / np.maximum(bound, 1e-300)).max()),
                                                                     float(gap.max())))
    assert np.all(gap <= bound)
    assert np.any(res < full)


def test_stem_is_zero_outside_its_groups_records():
    """A stem holds nothing outside the song frames its own group's DETECT records reach, and everything in stem 0
    when no table is given."""
    p, song, ev, wins, table = _scripted()
    stems, covered = sso.assemble_stems(song, ev, wins, p.timing_frames, table, 3)
    for g in range(3):
        assert covered[g].any() and not covered[g].all()
        assert not stems[g][:, ~covered[g]].any(), g
    one, cov = sso.assemble_stems(song, ev, wins, p.timing_frames, None, 3)
    assert not one[1:].any() and not cov[1:].any()
    assert np.array_equal(cov[0], covered.any(axis=0))
    assert sso.stem_of(-1, table, 3) == 0 and sso.stem_of(1, table, 3) == 2 and sso.stem_of(99, table, 3) == 1
    assert sso.stem_of(1, table, 2) == 1 and sso.stem_of(5, None, 3) == 0


def test_stem_arguments_without_a_device(tmp_path):
    """The checks that come before any device set-up: the window traversal has no song-level stems, the command line
    says so before it reads a file, and the new keywords exist, off by default, where the documentation puts them."""
    import inspect
    from amt_saga import audio, loop, song_walk, transcribe as tr
    with pytest.raises(ValueError, match='stems'):
        tr.transcribe(np.zeros(4096, np.float32), traversal='windows', stems=True)
    with pytest.raises(ValueError, match='stems'):
        tr.transcribe(np.zeros(4096, np.float32), stems=True)       # 'windows' is the default
    missing = str(tmp_path / 'missing.flac')
    with pytest.raises(SystemExit, match='--traversal song'):
        tr.main([missing, str(tmp_path / 'o.mid'), '--stems-dir', str(tmp_path / 'stems')])
    with pytest.raises(SystemExit, match='--traversal song'):
        tr.main([missing, str(tmp_path / 'o.mid'), '--stems-dir', str(tmp_path / 'stems'), '--traversal', 'windows'])
    assert not os.path.exists(str(tmp_path / 'stems'))
    for fn, kw in ((song_walk.SongState.__init__, 'keep_stems'), (song_walk.prepare_songs, 'keep_stems'),
                   (song_walk.walk_songs, 'stems'), (song_walk.iter_song_queue, 'stems'), (song_walk.check_walk, 'stems'),
                   (loop.TranscriptionLoop.prepare_songs, 'keep_stems'), (loop.TranscriptionLoop.walk_songs, 'stems'),
                   (loop.TranscriptionLoop.run_songs, 'stems'), (loop.TranscriptionLoop.iter_song_queue, 'stems'),
                   (loop.TranscriptionLoop.run_song_queue, 'stems'), (tr.transcribe, 'stems'),
                   (tr.iter_transcribe_songs, 'stems')):
        par = inspect.signature(fn).parameters[kw]
        assert par.default is False, (fn.__qualname__, kw)          # off by default: every existing call is unchanged
    for fn in (audio.AudioBatch.subtract, loop.TranscriptionLoop._step):
        assert inspect.signature(fn).parameters['stems'].default is None
    assert callable(song_walk.SongState.stem_waves)

    class NoSpan:                                                   # what check_walk reads of a loop
        span_subtract = False
    with pytest.raises(ValueError, match='AMT_SUBTRACT_SPAN'):
        song_walk.check_walk(NoSpan(), stems=True)


def test_stems_entry_point_checks_without_gpu():
    """amt_subtract_span_stems is declared, bound and validates on the host: NULL arguments, a NULL stems / frame_base /
    offset / t_song, G < 1 and pool_frames < 1 return AMT_E_INVALID before anything is launched (the pointers below are
    never dereferenced)."""
    from amt_saga import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'amt_saga.h')).read()
    assert 'int amt_subtract_span_stems(' in header and 'typedef struct amt_stem_args' in header
    assert len(_lib.PROTOTYPES['amt_subtract_span_stems'][1]) == 5
    assert [n for n, _ in _lib.StemArgs._fields_] == ['stems', 'frame_base', 'offset', 't_song', 'program', 'prog_group',
                                                      'n_prog', 'G', 'pool_frames']
    assert ctypes.sizeof(_lib.StemArgs) == 6 * 8 + 2 * 4 + 8
    lib = _lib.load()
    fake = 4096                                                     # a non-NULL address; no check reads through it
    a = _lib.SubtractArgs()
    a.resid, a.guess = fake, fake
    a.B, a.T, a.ldf, a.F = 2, 12, 1028, 1025
    a.resid_stride, a.guess_stride = 12 * 1028, 12 * 1028
    a.guess_frames_all, a.normalize, a.relu, a.overkill_factor = 5, 0, 1, 1.0

    def stem(**kw):
        f = dict(stems=fake, frame_base=fake, offset=fake, t_song=fake, program=None, prog_group=None, n_prog=0, G=3,
                 pool_frames=40)
        f.update(kw)
        return _lib.stem_args(**f)
    call = lib.amt_subtract_span_stems
    assert call(None, fake, 12, ctypes.byref(stem()), None) == _lib.AMT_E_INVALID
    assert call(ctypes.byref(a), None, 12, ctypes.byref(stem()), None) == _lib.AMT_E_INVALID
    assert call(ctypes.byref(a), fake, 12, None, None) == _lib.AMT_E_INVALID
    for bad in (dict(stems=None), dict(frame_base=None), dict(offset=None), dict(t_song=None), dict(G=0),
                dict(pool_frames=0)):
        assert call(ctypes.byref(a), fake, 12, ctypes.byref(stem(**bad)), None) == _lib.AMT_E_INVALID, bad
    a.relu = 0                                                      # amt_subtract_span's own checks come first
    assert call(ctypes.byref(a), fake, 12, ctypes.byref(stem()), None) == _lib.AMT_E_UNSUPPORTED
    a.relu, a.ldf = 1, 1027
    assert call(ctypes.byref(a), fake, 12, ctypes.byref(stem()), None) == _lib.AMT_E_SHAPE
    with pytest.raises(ValueError):
        _lib.stem_args(nonsense=1)
