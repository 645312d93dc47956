"""GPU: beat tracking (amt_beat_envelope, amt_beat_track, amt_saga.beat, the transcription's beats argument) against
tests/beat_reference.py fed the device's own magnitudes.  After one float32 step per cell the rule is all-integer, so
every comparison is exact: flux, envelope, period, count, beats, C and back."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beat_reference as R                                         # noqa: E402

pytestmark = pytest.mark.gpu

FILL_E, FILL_FLUX = 0xABCD, -77                                    # what an output holds before a launch


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import beat, _lib
    from amt_saga.device import stream_ptr
    return dict(torch=torch, beat=beat, _lib=_lib, lib=_lib.load(), stream_ptr=stream_ptr)


def envelope_pool(F):
    """The songs of one F of the corpus -- every T, a silent song and one with a NaN ref between live ones -- in one
    pool with gaps of 2 sentinel frames and 5.0 in the pad columns: (songs [(name, S, ref)], pool, frame bases)."""
    songs = [(name, S, ref) for name, S, ref, _ in R.env_corpus() if S.shape[1] == F]
    songs.insert(2, ('silent', np.zeros((40, F), np.float32), np.float32(0.0)))
    songs.insert(5, ('ref nan', R.env_content('random', 12, F, 1), np.float32('nan')))
    ldf = (F + 3) // 4 * 4 + 4
    gap = 2
    pool = np.full((gap + sum(S.shape[0] + gap for _, S, _ in songs), ldf), 9.0, np.float32)
    pool[:, F:] = 5.0
    fbase, at = [], gap
    for _, S, _ in songs:
        pool[at:at + S.shape[0], :F] = S
        fbase.append(at)
        at += S.shape[0] + gap
    return songs, pool, fbase


def launch_envelope(env, pool, fbase, frames, F, refs, w):
    torch, beat, _lib = env['torch'], env['beat'], env['_lib']
    pf = int(pool.shape[0])
    e = torch.from_numpy(np.full(pf, FILL_E, np.uint16)).cuda()
    flux = torch.full((pf,), FILL_FLUX, dtype=torch.int32, device='cuda')
    need = env['lib'].amt_beat_scratch_bytes(len(frames), pf, 0, 0)
    scratch = torch.empty((need,), dtype=torch.uint8, device='cuda')
    a = beat.env_args(mag=pool, ref=torch.tensor(refs, dtype=torch.float32).cuda(),
                      frame_base=torch.tensor(fbase, dtype=torch.int64).cuda(),
                      t_frames=torch.tensor(frames, dtype=torch.int32).cuda(), env=e, flux=flux, scratch=scratch,
                      scratch_bytes=need, n=len(frames), pool_frames=pf, max_frames=max(frames), ldf=int(pool.shape[1]),
                      F=F, w=w)
    assert env['lib'].amt_beat_envelope(ctypes.byref(a), env['stream_ptr']()) == _lib.AMT_OK
    torch.cuda.synchronize()
    return e.cpu().numpy(), flux.cpu().numpy()


@pytest.mark.parametrize('F', R.ENV_F)
def test_envelope_corpus_against_the_reference(env, F):
    """Every T at this F in one ragged call per w, magnitudes above ref, a silent song and a NaN ref between live ones,
    junk in the pad columns, gaps between the songs: flux and envelope equal the reference's, frames of no song are not
    written; then amt_saga.beat.onset_envelopes on views of the pool, on a packed copy and with the maxima taken on the
    device.  Prints the count of mismatching cells (expected 0)."""
    torch, beat = env['torch'], env['beat']
    songs, pool, fbase = envelope_pool(F)
    assert {S.shape[0] for _, S, _ in songs} >= set(R.ENV_T)
    frames, refs = [S.shape[0] for _, S, _ in songs], [float(r) for _, _, r in songs]
    d_pool = torch.from_numpy(pool).cuda()
    fluxes = [R.flux_of(S, ref) for _, S, ref in songs]
    owned = np.zeros(pool.shape[0], bool)
    for b, t in zip(fbase, frames):
        owned[b:b + t] = True
    wrong = cells = 0
    for w in R.ENV_W:
        e, flux = launch_envelope(env, d_pool, fbase, frames, F, refs, w)
        assert (e[~owned] == FILL_E).all() and (flux[~owned] == FILL_FLUX).all(), w
        for (name, S, ref), b, t, fl in zip(songs, fbase, frames, fluxes):
            want = R.envelope_from_flux(fl, w, bool(ref > 0))
            wrong += int((flux[b:b + t] != np.asarray(fl)).sum()) + int((e[b:b + t] != np.asarray(want)).sum())
            cells += 2 * t
            assert flux[b:b + t].tolist() == fl, (name, w, 'flux')
            assert e[b:b + t].tolist() == want, (name, w, 'e')
    print('envelope F=%d: %d mismatches in %d cells' % (F, wrong, cells))
    assert wrong == 0
    # the Python layer: views with gaps in one pool (read in place), then a packed copy of separate tensors
    want = [R.envelope_from_flux(fl, 43, bool(ref > 0)) for fl, (_, _, ref) in zip(fluxes, songs)]
    views = [d_pool[b:b + t, :F] for b, t in zip(fbase, frames)]
    d_refs = torch.tensor(refs, dtype=torch.float32).cuda()
    got = beat.onset_envelopes(views, refs=d_refs, w=43, flux=True)
    torch.cuda.synchronize()
    assert [g[0].cpu().tolist() for g in got] == want and [g[1].cpu().tolist() for g in got] == fluxes
    copies = [v.clone() for v in views]
    got = beat.onset_envelopes(copies, refs=refs, w=43)
    assert [g.cpu().tolist() for g in got] == want
    # refs=None: the maxima of the live bins, taken on the device -- the pad columns hold 5.0 and must not be seen
    tops = [np.float32(S.max()) if S.size else np.float32(0) for _, S, _ in songs]
    got = beat.onset_envelopes(views, w=43)
    assert [g.cpu().tolist() for g in got] == [R.envelope(S, top, 43)[1] for (_, S, _), top in zip(songs, tops)]


_TRACK_CORPUS = {name: (lags, kw, envs) for name, lags, kw, envs in R.track_corpus()}
_WANT = {}


def track_reference(name):
    """The reference's results of one corpus group, computed once and shared."""
    if name not in _WANT:
        (lag_lo, lag_hi, fps), kw, envs = _TRACK_CORPUS[name]
        prior, pen = R.lag_tables(lag_lo, lag_hi, fps, **kw)
        _WANT[name] = [R.track(e, lag_lo, lag_hi, prior, pen) for e in envs]
    return _WANT[name]


def same_track(got, want, tag):
    assert got['period'] == want['period'], (tag, 'period', got['period'], want['period'])
    assert got['frames'] == want['beats'], (tag, 'beats')
    assert got['C'].cpu().tolist() == want['C'], (tag, 'C')
    assert got['back'].cpu().tolist() == want['back'], (tag, 'back')


@pytest.mark.parametrize('name', sorted(_TRACK_CORPUS))
def test_track_corpus_against_the_reference(env, name):
    """All envelopes of the group -- zeros, a constant, a spike, a zero-length song, impulse trains at every lag, T around
    lag_lo and around chunk multiples, random envelopes -- in ONE ragged call: period, count, beats, C and back equal the
    reference's; a song alone gives what it gave inside the batch."""
    torch, beat = env['torch'], env['beat']
    (lag_lo, lag_hi, fps), kw, envs = _TRACK_CORPUS[name]
    p = beat.params_for_lags(lag_lo, lag_hi, fps, **kw)
    assert np.array_equal(p[3], R.lag_tables(lag_lo, lag_hi, fps, **kw)[0]) and np.array_equal(p[4], R.lag_tables(lag_lo, lag_hi, fps, **kw)[1])
    d_envs = [torch.from_numpy(np.asarray(e).astype(np.uint16)).cuda() for e in envs]
    got = beat.track(d_envs, params=p, debug=True)
    torch.cuda.synchronize()
    want = track_reference(name)
    assert len(got) == len(want) == len(envs)
    for i, (g, w_) in enumerate(zip(got, want)):
        same_track(g, w_, (name, i, len(envs[i])))
        assert g['beats'] == [f * 512.0 / 44100.0 for f in g['frames']]
        assert len(g['frames']) <= R.bound(len(envs[i]), lag_lo)
    assert any(g['period'] for g in got) and any(not g['period'] for g in got) or 'flat' in name
    for i in sorted({1, 5, len(envs) // 2, len(envs) - 2, len(envs) - 1} & set(range(len(envs)))):
        alone = beat.track([d_envs[i]], params=p, debug=True)[0]
        same_track(alone, want[i], (name, i, 'alone'))


def test_track_unequal_songs_in_one_call_and_through_the_abi(env):
    """Many songs of unequal lengths, zero-length ones included, through amt_beat_track itself with gaps in the pool: the
    reference's results, frames of no song and beats behind a song's count left as they were."""
    torch, beat, _lib = env['torch'], env['beat'], env['_lib']
    lag_lo, lag_hi, fps = 5, 40, 30.0
    p = beat.params_for_lags(lag_lo, lag_hi, fps)
    rng = np.random.default_rng(4)
    lens = [0, 333, 1, 64, 0, 1000, 65, 41, 7, 500]
    envs = [np.minimum(R.E_MAX, (rng.random(t) ** 6 * 9000).astype(np.int64)) + R.impulses(t, 11 + i, first=i % 5, height=5000)
            for i, t in enumerate(lens)]
    gap = 3
    pf = gap + sum(t + gap for t in lens)
    pool = np.full(pf, 0x1234, np.uint16)
    fbase, at = [], gap
    for e, t in zip(envs, lens):
        pool[at:at + t] = e
        fbase.append(at)
        at += t + gap
    bounds = [R.bound(t, lag_lo) for t in lens]
    bbase = [int(b) for b in np.concatenate([[0], np.cumsum(bounds)])[:-1]]
    total, n = sum(bounds), len(lens)
    cuda = lambda a, dt: torch.tensor(a, dtype=dt).cuda()            # noqa: E731
    period, count = torch.full((n,), -5, dtype=torch.int32).cuda(), torch.full((n,), -5, dtype=torch.int32).cuda()
    beats = torch.full((total,), -9, dtype=torch.int32).cuda()
    C, back = torch.full((pf,), -3, dtype=torch.int64).cuda(), torch.full((pf,), -4, dtype=torch.int32).cuda()
    need = env['lib'].amt_beat_scratch_bytes(n, pf, lag_hi, total)
    scratch = torch.empty((need,), dtype=torch.uint8, device='cuda')
    a = beat.track_args(env=torch.from_numpy(pool).cuda(), frame_base=cuda(fbase, torch.int64), t_frames=cuda(lens, torch.int32),
                        prior=cuda(p[3], torch.int32), pen=cuda(np.ascontiguousarray(p[4]), torch.int32),
                        beat_base=cuda(bbase, torch.int64), period=period, count=count, beats=beats, C=C, back=back,
                        scratch=scratch, scratch_bytes=need, n=n, pool_frames=pf, beats_total=total, max_frames=max(lens),
                        lag_lo=lag_lo, lag_hi=lag_hi)
    assert env['lib'].amt_beat_track(ctypes.byref(a), env['stream_ptr']()) == _lib.AMT_OK
    torch.cuda.synchronize()
    period, count, beats, C, back = (x.cpu().numpy() for x in (period, count, beats, C, back))
    owned = np.zeros(pf, bool)
    for i, (e, t, b, bb) in enumerate(zip(envs, lens, fbase, bbase)):
        want = R.track(e, lag_lo, lag_hi, p[3], p[4])
        assert (int(period[i]), int(count[i])) == (want['period'], len(want['beats'])), i
        assert beats[bb:bb + count[i]].tolist() == want['beats'], i
        assert (beats[bb + count[i]:bb + bounds[i]] == -9).all(), i
        assert C[b:b + t].tolist() == want['C'] and back[b:b + t].tolist() == want['back'], i
        owned[b:b + t] = True
    assert (C[~owned] == -3).all() and (back[~owned] == -4).all()
    assert sum(1 for c in count if c > 1) >= 4


CLICKS = [(60, {}), (90, {}), (120, {}), (133, {}), (174, {}), (100, dict(jitter_s=0.01)), (120, dict(slow=0.002)),
          (75, dict(jitter_s=0.01, slow=0.002)), (200, {})]


def test_click_songs_through_beat_track(env):
    """The nine click songs in ONE beat_track call: the conditions of the CPU test (periods within one lag, equal counts,
    every beat within two hops of gold both ways; at 200 bpm the half tempo, period 52, 29 beats on gold beats), and
    every song's period and beats equal to the reference fed the device's own magnitudes."""
    torch, beat = env['torch'], env['beat']
    made = [R.click_song(bpm, seed=bpm, **kw) for bpm, kw in CLICKS]
    keep = {}
    got = beat.beat_track([torch.from_numpy(y).cuda() for y, _ in made], 44100, keep=keep)
    mag, refs = keep['mag'].cpu().numpy(), keep['refs'].cpu().numpy()
    lag_lo, lag_hi, w, prior, pen = R.tables(44100, 512)
    for (bpm, kw), (y, gold), g, b, t, ref in zip(CLICKS, made, got, keep['frame_base'], keep['frames'], refs):
        assert t == 1 + len(y) // 512
        S = mag[b:b + t, :1025]
        _, e = R.envelope(S, ref, w)
        assert keep['env'][b:b + t].cpu().tolist() == e, bpm
        want = R.track(e, lag_lo, lag_hi, prior, pen)
        assert g['period'] == want['period'] and g['frames'] == want['beats'], bpm
        assert g['beats'] == [f * 512 / 44100 for f in g['frames']]
        if bpm == 200:
            assert g['period'] == 52 and len(g['beats']) == 29
            R.click_conditions(g['beats'], g['period'], gold, bpm, count=29, half=True)
            assert abs(g['tempo'] - 100.0) < 2.0
        elif kw:
            two_hops = 2 * 512 / 44100
            assert len(g['beats']) == len(gold), (bpm, kw)
            assert all(np.abs(gold - x).min() <= two_hops for x in g['beats']), (bpm, kw)
            assert all(np.abs(np.asarray(g['beats']) - x).min() <= two_hops for x in gold), (bpm, kw)
        else:
            R.click_conditions(g['beats'], g['period'], gold, bpm)
            assert abs(g['tempo'] - bpm) < 0.02 * bpm
    assert [g['period'] for g in got[:5]] == [86, 57, 43, 39, 30] and [len(g['beats']) for g in got[:5]] == [18, 26, 35, 39, 51]
    # a song alone is the song inside the batch
    alone = beat.beat_track([torch.from_numpy(made[3][0]).cuda()], 44100)[0]
    assert alone == got[3]
    quiet = beat.beat_track([torch.zeros(30000).cuda()], 44100)[0]
    assert quiet == dict(period=0, frames=[], beats=[], tempo=None)


def test_transcribe_with_beats_appends_beat_track_and_changes_nothing_else(env, tmp_path):
    torch, beat = env['torch'], env['beat']
    from amt_saga import events, transcribe as tr
    from amt_saga.hyperparams import Hyperparams
    p = Hyperparams(N=2048, window_size_note_time=1)
    lp = tr._make_loop(p, 1, ('timing', 'pitch', 'instrument', 'velocity'), (0, 1, 2), None, 'bank')
    wf, _ = R.click_song(150, sr=p.sr, seconds=2.4 * p.H * (p.timing_frames - 1) / p.sr, first=0.3, tail=0.4, seed=5)
    want = beat.beat_track([torch.from_numpy(wf).cuda()], p.sr, n_fft=p.N, hop=p.H)[0]
    assert len(want['beats']) >= 4 and want['period'] > 0
    plain = tr.transcribe(wf, p, iters=1, loop=lp, traversal='song')
    notes, evs, found = tr.transcribe(wf, p, iters=1, loop=lp, traversal='song', beats=True)
    assert found == want and len(plain) == 2 and notes == plain[0] and np.array_equal(evs, plain[1])
    out = tr.transcribe_songs([wf, wf[:len(wf) // 2]], p, slots=2, iters=1, loop=lp, beats=True)
    assert [len(o) for o in out] == [3, 3] and out[0][2] == want
    assert out[1][2] == beat.beat_track([torch.from_numpy(wf[:len(wf) // 2]).cuda()], p.sr, n_fft=p.N, hop=p.H)[0]
    assert [dict(nt, song=0) for nt in plain[0]] == out[0][0]
    # the tempo map of what was found: every kept beat on a multiple of 480 ticks
    path = str(tmp_path / 'song.mid')
    events.write_midi(notes, path, beats=found['beats'])
    assert all(k % 480 == 0 for _, k in events.tempo_anchors(found['beats']))
    assert len(events.read_midi(path, full=True)) == len(notes)


def test_command_lines_write_the_tempo_map_and_the_beats(env, tmp_path):
    """Both modes: --tempo-map puts beat_track's beats of the file into the .mid (one set-tempo event per anchor) and
    leaves every note where it was in seconds; --beats-out / --beats-dir write them one per line; with --hpss the beats
    are those of the signal before the split; with --beats-out alone the .mid keeps its one fixed tempo."""
    torch, beat = env['torch'], env['beat']
    from amt_saga import events, flac, transcribe as tr
    sr = 44100
    wf, _ = R.click_song(150, sr=sr, seconds=5.0, first=0.3, tail=0.4, seed=5)
    src, other = str(tmp_path / 'clip.flac'), str(tmp_path / 'other.flac')
    flac.save_float(wf, src, sr)
    flac.save_float(wf[:len(wf) // 2], other, sr)
    wf24 = flac.load_float(src)[0].astype(np.float32)
    want = beat.beat_track([torch.from_numpy(wf24).cuda()], sr)[0]
    assert len(want['beats']) >= 4
    lines = ''.join('%.6f\n' % t for t in want['beats'])
    plain, mapped, btxt = str(tmp_path / 'plain.mid'), str(tmp_path / 'map.mid'), str(tmp_path / 'beats.txt')
    tr.main([src, plain, '--iters', '1', '--traversal', 'song', '--beats-out', btxt])       # beats only: the old .mid
    assert open(btxt).read() == lines
    tr.main([src, mapped, '--iters', '1', '--traversal', 'song', '--tempo-map', '--beats-out', btxt])
    assert open(btxt).read() == lines
    anchors = events.tempo_anchors(want['beats'])
    data = open(mapped, 'rb').read()
    assert data.count(b'\xff\x51\x03') == len(anchors) and open(plain, 'rb').read().count(b'\xff\x51\x03') == 1
    old, new = events.read_midi(plain, full=True), events.read_midi(mapped, full=True)
    assert len(old) == len(new)
    for a, b in zip(old, new):
        assert (a['pitch'], a['program']) == (b['pitch'], b['program']) and abs(a['start'] - b['start']) <= 2.5e-3
    # with --hpss: the beats of the signal as given, not of its harmonic part
    tr.main([src, str(tmp_path / 'h.mid'), '--iters', '1', '--hpss', '--tempo-map', '--quantize', '4', '--beats-out', btxt])
    assert open(btxt).read() == lines
    # the song queue
    mid, bdir = str(tmp_path / 'mid'), str(tmp_path / 'beats')
    tr.main(['--songs', src, other, '--out-dir', mid, '--slots', '2', '--iters', '1', '--tempo-map', '--beats-dir', bdir])
    assert sorted(os.listdir(bdir)) == ['clip.beats.txt', 'other.beats.txt']
    assert open(os.path.join(bdir, 'clip.beats.txt')).read() == lines
    assert open(os.path.join(mid, 'clip.mid'), 'rb').read() == data
    half = beat.beat_track([torch.from_numpy(flac.load_float(other)[0].astype(np.float32)).cuda()], sr)[0]
    assert open(os.path.join(bdir, 'other.beats.txt')).read() == ''.join('%.6f\n' % t for t in half['beats'])
