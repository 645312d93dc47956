"""CPU: the two rules of amt_saga.transcribe that every entry point goes through -- _result, the one place that orders
(notes, events[, residual][, stems][, percussive][, beats]) from a Song, and _prepare, the one place that sequences
resample, beat tracking and the harmonic/percussive split.  Host tensors and recording stubs: no device."""
import itertools

import numpy as np
import pytest
import torch

from amt_saga import transcribe as tr
from amt_saga.hyperparams import Hyperparams

OPTIONAL = ('residual', 'stems', 'percussive', 'beats')


def test_song_fields_default_to_none():
    song = tr.Song(3, 1000)
    assert (song.index, song.samples) == (3, 1000)
    assert all(getattr(song, k) is None for k in ('notes', 'events') + OPTIONAL)
    assert set(tr.Song.__slots__) == {'index', 'samples', 'notes', 'events'} | set(OPTIONAL)


@pytest.mark.parametrize('wants', list(itertools.product((False, True), repeat=4)))
def test_result_orders_the_tuple(wants):
    """All 16 combinations of the four wants: notes and events, then exactly the wanted items in the documented order,
    whatever the other fields hold; the queue's form has the index in front."""
    marks = {k: object() for k in ('notes', 'events') + OPTIONAL}
    song = tr.Song(7, 1234, **marks)
    expect = (marks['notes'], marks['events']) + tuple(marks[k] for k, w in zip(OPTIONAL, wants) if w)
    got = tr._result(song, *wants)
    assert isinstance(got, tuple) and len(got) == len(expect) and all(g is e for g, e in zip(got, expect))
    indexed = tr._result(song, *wants, indexed=True)
    assert indexed[0] == 7 and len(indexed) == 1 + len(expect) and all(g is e for g, e in zip(indexed[1:], expect))
    by_name = tr._result(song, **dict(zip(OPTIONAL, wants)))
    assert len(by_name) == len(expect) and all(g is e for g, e in zip(by_name, expect))


def test_result_keeps_a_wanted_none():
    """A wanted item that is None (the residual of a walk that stopped early) keeps its place."""
    song = tr.Song(0, 10, notes=[], events='e', stems='s')
    assert tr._result(song, True, True, False, False) == ([], 'e', None, 's')


@pytest.fixture
def calls(monkeypatch):
    """resample, beat_track and hpss replaced by stubs that record (name, the signal they saw, keywords); _device_mono
    by its host twin."""
    seen = []

    def resample(wf, sr_in, sr_out):
        seen.append(('resample', wf, dict(sr_in=sr_in, sr_out=sr_out)))
        return torch.as_tensor(np.asarray(wf, dtype=np.float32)).reshape(-1) + 1.0

    def beat_track(waves, sr, **kw):
        seen.append(('track', waves[0], dict(kw, sr=sr, n=len(waves))))
        return [dict(period=7, tempo=120.0, beats=[0.5], frames=[43])]

    def hpss(waves, **kw):
        seen.append(('split', waves[0], dict(kw, n=len(waves))))
        return [(waves[0] * 0.75, waves[0] * 0.25, 'spectra the caller does not look at')]
    monkeypatch.setattr(tr.audio, 'resample', resample)
    monkeypatch.setattr(tr.beat_mod, 'beat_track', beat_track)
    monkeypatch.setattr(tr.audio, 'hpss', hpss)
    monkeypatch.setattr(tr, '_device_mono', lambda wf: torch.as_tensor(np.asarray(wf, dtype=np.float32)).reshape(-1))
    return seen


@pytest.mark.parametrize('rate, beats, split', list(itertools.product((None, 22050), (False, True), (False, True))))
def test_prepare_sequences_resample_track_split(calls, rate, beats, split):
    p = Hyperparams(N=2048)
    wf = np.linspace(-0.5, 0.5, 3 * p.N, dtype=np.float32)
    tracked = dict(bpm=(60, 200)) if beats else None
    opts = dict(kernel=(17, 31)) if split else None
    out, drums, found = tr._prepare(wf, rate, p, tracked, opts)
    names = [c[0] for c in calls]
    assert names == [n for n, on in (('resample', rate is not None), ('track', beats), ('split', split)) if on]
    given = torch.as_tensor(wf) + 1.0 if rate is not None else torch.as_tensor(wf)    # the signal as given, at p.sr
    for name, saw, kw in calls:
        if name == 'resample':
            assert saw is wf and kw == dict(sr_in=22050, sr_out=p.sr)
        else:                                                       # track and split both see the UNSPLIT signal
            assert saw.dtype == torch.float32 and saw.ndim == 1 and torch.equal(saw, given), name
    if beats:
        assert calls[names.index('track')][2] == dict(bpm=(60, 200), sr=p.sr, n_fft=p.N, hop=p.H, n=1)
        assert found == dict(period=7, tempo=120.0, beats=[0.5], frames=[43])
    else:
        assert found is None
    if split:
        assert calls[-1][2] == dict(kernel=(17, 31), n_fft=p.N, hop=p.H, n=1)
        assert torch.equal(out, given * 0.75) and torch.equal(drums, given * 0.25)
    else:
        assert drums is None
        assert torch.equal(torch.as_tensor(out), given)
        assert out is wf or rate is not None                       # untouched: the array handed in goes on as it is


@pytest.mark.parametrize('n', [1, 1023, 1024])
def test_prepare_gives_a_short_signal_no_beats_without_a_call(calls, n):
    """p.N // 2 samples or fewer: the STFT's padding has nothing to reflect, so the empty beat dict and no call; the
    split is still made, and one sample more is tracked."""
    p = Hyperparams(N=2048)
    assert p.N // 2 == 1024
    wf = np.full(n, 0.25, np.float32)
    out, drums, found = tr._prepare(wf, None, p, {}, None)
    assert found == dict(period=0, tempo=None, beats=[], frames=[]) and calls == [] and out is wf and drums is None
    _, drums, found = tr._prepare(wf, None, p, {}, {})
    assert found == dict(period=0, tempo=None, beats=[], frames=[]) and [c[0] for c in calls] == ['split']
    assert drums is not None
    del calls[:]
    _, _, found = tr._prepare(np.full(p.N // 2 + 1, 0.25, np.float32), None, p, {}, None)
    assert [c[0] for c in calls] == ['track'] and found['period'] == 7
