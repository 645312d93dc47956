"""GPU: the song-resident sliding-window traversal (TranscriptionLoop.run_songs, amt_song_*): the slide kernel alone
against numpy indexing, the live walk against the CPU restatement (tests/song_oracle.py), the shared step against run(),
and the product path transcribe(traversal='song')."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import song_oracle as so                                        # noqa: E402
from oracle import synth as osynth                              # noqa: E402
from oracle.compare import bands_for                            # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import synth, loop, hyperparams, audio, _lib
    return dict(torch=torch, synth=synth, loop=loop, hp=hyperparams, audio=audio, _lib=_lib, lib=_lib.load())


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def test_slide_kernel_vs_numpy(env):
    """amt_song_slide on random spectrograms: songs shorter than a window, ending inside the fetched half, ending
    exactly on a half boundary, long ones; random masks.  Sliding songs bit-exact against numpy indexing, the others
    bit-identical to before the call; offset / count / finished as restated.  An odd window is rejected."""
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    rng = np.random.default_rng(7)
    T, half, ldf = 86, 43, 1028
    # fetched song frames: [offset + 86, offset + 129).  t_song inside that range = the song ends inside the fetched
    # half (150 @ 43: 21 of 43 rows; 216 @ 129: one row; 257 @ 129: all but one); 129 @ 43 / 215 @ 129: ends exactly where
    # the fetch starts; 172 @ 43: exactly where it ends; 400 @ 172, 600 @ 0, 300 @ 86: whole fetches; 30, 60: shorter
    # than a window
    t_song = [30, 86, 100, 129, 172, 173, 400, 215, 60, 130, 150, 216, 257, 172, 600, 300, 215, 150]
    offs = [0, 0, 43, 43, 86, 129, 172, 172, 43, 86, 43, 129, 129, 43, 0, 86, 129, 43]
    mask = [1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    B = len(t_song)
    fbase = np.concatenate(([0], np.cumsum(t_song)))
    s_mag = rng.standard_normal((fbase[-1], ldf)).astype(np.float32)
    s_ph = rng.standard_normal((fbase[-1], ldf, 2)).astype(np.float32)
    w_mag = rng.standard_normal((B, T, ldf)).astype(np.float32)
    w_ph = rng.standard_normal((B, T, ldf, 2)).astype(np.float32)
    count = rng.integers(0, 5, B).astype(np.int32)
    d = dict(wm=torch.from_numpy(w_mag).cuda(), wp=torch.from_numpy(w_ph).cuda(), sm=torch.from_numpy(s_mag).cuda(),
             sp=torch.from_numpy(s_ph).cuda(), fb=torch.from_numpy(fbase[:-1].astype(np.int64)).cuda(),
             ts=_i32(torch, t_song), sl=_i32(torch, mask), off=_i32(torch, offs), cnt=_i32(torch, count),
             fin=_i32(torch, np.zeros(B)))
    call = lambda t: lib.amt_song_slide(d['wm'].data_ptr(), d['wp'].data_ptr(), B, t, ldf, T * ldf, d['sm'].data_ptr(),
                                        d['sp'].data_ptr(), d['fb'].data_ptr(), d['ts'].data_ptr(), d['sl'].data_ptr(),
                                        d['off'].data_ptr(), d['cnt'].data_ptr(), d['fin'].data_ptr(), None)
    assert call(85) == _lib.AMT_E_INVALID                          # odd timing_frames: rejected, nothing launched
    assert call(T) == _lib.AMT_OK
    torch.cuda.synchronize()
    gm, gp = d['wm'].cpu().numpy(), d['wp'].cpu().numpy()
    fetched = []
    for b in range(B):
        if not mask[b]:
            assert np.array_equal(gm[b], w_mag[b]) and np.array_equal(gp[b], w_ph[b]), b
            continue
        o = offs[b] + half
        for got, w, s in ((gm[b], w_mag[b], s_mag), (gp[b], w_ph[b], s_ph)):
            want = np.zeros_like(w)
            want[:half] = w[half:]
            song = s[fbase[b]:fbase[b + 1]]
            fresh = song[o + half:o + 2 * half]
            want[half:half + len(fresh)] = fresh
            assert np.array_equal(got, want), b
        fetched.append(int(np.clip(t_song[b] - (o + half), 0, half)))
    assert sum(n == half for n in fetched) >= 3 and sorted(n for n in fetched if 0 < n < half) == [1, 21, 42]
    want_off = [o + half * m for o, m in zip(offs, mask)]
    assert d['off'].cpu().tolist() == want_off
    assert d['cnt'].cpu().tolist() == [0 if m else int(c) for m, c in zip(mask, count)]
    assert d['fin'].cpu().tolist() == [int(m and o >= t) for m, o, t in zip(mask, want_off, t_song)]


# What the CPU restatement ALONE gives for the seeds of song_oracle.WALK_CASES (tests/golden/gen_song_fixtures.py screen,
# stored in tests/golden/song_fixtures.npz): (live steps, decisions inside their tie band) with float32 heads, the same
# with float64 heads, and whether the two runs agree on every integer.  Usable: at most 1 step in 10 near a tie.
SCREENED = {'bank2048': (54, 1, 54, 1, 1), 'render2048': (45, 1, 45, 1, 1), 'bank4096': (45, 1, 45, 1, 1),
            'render4096': (30, 0, 30, 0, 1), 'silence': (60, 0, 60, 0, 1), 'plain_slides': (17, 0, 17, 0, 1)}


def test_walk_seeds_were_screened():
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'song_fixtures.npz'))
    for name in so.WALK_CASES:
        live32, near32, live64, near64, same = (int(v) for v in fx['screen_' + name])
        assert (live32, near32, live64, near64, same) == SCREENED[name], name
        assert near32 * 10 <= live32 and near64 * 10 <= live64, name


@pytest.mark.parametrize('case', list(so.WALK_CASES))
def test_walk_vs_cpu_restatement(env, case):
    """Live walk parity: the real heads on short windows, >= 4 songs of unequal length per batch.  Integer events
    bit-exact, the heads' floats inside oracle/compare.py's bands, the final residual window to 1e-4; a decision within
    the band of a rounding tie is handed to the restatement (LoopOracle._round), never skipped, and at most 1 step in
    10 of a case may need that (SCREENED: what the restatement alone says about these seeds)."""
    nfft, wsec, guess, seed, lengths, max_notes, silence, silent, shift = so.WALK_CASES[case]
    torch, synth = env['torch'], env['synth']
    p = env['hp'].Hyperparams(N=nfft, window_size_note_time=wsec)
    heads = so.HEADS
    lp = env['loop'].TranscriptionLoop(p, heads=heads, guess=guess)
    if shift:
        w = {k: v.copy() for k, v in lp.nets['timing_start'].weights.items()}
        w['dense2/bias'] = w['dense2/bias'] + np.float32(shift)
        lp.nets['timing_start'].set_weights(w)
    lp.setup_device()
    songs = so.make_songs(p, seed, lengths, silent)
    lp.trace = []
    events, state = lp.run_songs(songs, max_notes=max_notes, silence=silence, poll=4, song0=3)
    torch.cuda.synchronize()
    trace, lp.trace = [{k: v.cpu().numpy() for k, v in t.items()} for t in lp.trace], None
    ev = events.cpu().numpy()
    steps, B = ev.shape[0], len(songs)
    assert ev.shape == (steps, B, 9) and len(trace) == steps
    assert state.finished.cpu().tolist() == [1] * B and steps <= state.bound
    table = synth.prog_group_table(p.instrument_classes)

    def guess_fn(program, pitch, velocity, frames):
        dur = min(float(np.float32(frames) * np.float32(p.H / p.sr)), 1.0)
        return osynth.render_window([(int(table[program]), pitch, velocity if velocity > 0 else 100, 0.0, dur)],
                                    lp.bank_len, p.sr).numpy()
    bank = osynth.guess_bank_waves((0,), p.pitch_low, p.pitch_high, sr=p.sr) if guess == 'bank' else None
    orc = so.SongOracle(p, heads, {k: n.weights for k, n in lp.nets.items()}, bank_waves=bank,
                        guess_fn=guess_fn if guess == 'render' else None)
    bands = bands_for(p)
    refs = {k: v.cpu().numpy() for k, v in state.refs.items()}
    mags = state.batch.mag.cpu().numpy()
    half, tf, F = p.timing_frames // 2, p.timing_frames, p.N // 2 + 1
    forced = live = 0
    kinds = np.zeros(4, int)
    for i in range(B):
        r = {k: float(v[i]) for k, v in refs.items()}
        ev_ref, mag_ref = orc.run_song(songs[i], r, max_notes, silence, song_id=3 + i, force=(ev[:, i, :], bands))
        for name, it, y, margin, v, was_forced in orc.decisions:
            dlt = float(np.abs(np.asarray(trace[it][name][i], np.float64).ravel() - np.asarray(y, np.float64).ravel()).max())
            print('song %d step %d %s product-oracle %.2e margin %.3f%s' % (i, it, name, dlt, margin,
                                                                            ' HANDED OVER' if was_forced else ''))
            assert dlt <= bands[name], ('float', i, name, it, dlt, bands[name])
            forced += was_forced
        live += len(ev_ref)
        want = so.pad_finished(ev_ref, steps, 3 + i, half)
        assert np.array_equal(ev[:, i, :], want), ('events', i, ev[:, i, :].tolist(), want.tolist())
        kinds += np.bincount(want[:, 2], minlength=4)
        assert np.all(mag_ref[:, tf:] == 0)
        scale = max(float(mag_ref.max()), 1e-30)
        assert np.abs(mags[i][:, :F].T - mag_ref[:, :tf]).max() / scale < 1e-4, ('residual', i)
    print('walk %s N=%d: %d steps x %d songs, %d live; kinds detect/slide/forced/finished = %s; %d decisions handed over'
          % (guess, nfft, steps, B, live, kinds.tolist(), forced))
    assert forced * 10 <= live, (forced, live)
    assert kinds[so.SLIDE] + kinds[so.FORCED_SLIDE] >= sum(-(-(1 + len(s) // p.H) // half) for s in songs)
    if shift:
        assert kinds[so.SLIDE] > 0                                 
    else:
        assert kinds[so.DETECT] > 0 and kinds[so.FORCED_SLIDE] > 0     # max_notes / silence are small enough to be hit
    if silent is not None:
        # the silent tail: forced slides of song `silent` that follow fewer than max_notes detections
        e = ev[:, silent, :]
        runs = [int(np.sum((e[:, 8] == o) & (e[:, 2] == so.DETECT))) for o in e[e[:, 2] == so.FORCED_SLIDE, 8]]
        assert min(runs) < max_notes, runs


def test_one_window_song_equals_run(env):
    """The shared step: songs exactly one window long, max_notes = iters, both traversals on the SAME spectrogram (the
    AudioBatch prepare() made is handed to prepare_songs as the songs' STFT) and the same normalisers.  Every onset stays
    in the first half, so the walk detects `iters` times before its first slide, and every one of the iters x songs
    records carries the pitch / program / velocity / frames run() emits, bit for bit; so do the residuals."""
    torch, synth = env['torch'], env['synth']
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    heads, iters, B = ('timing', 'pitch', 'instrument', 'velocity'), 3, 6
    lp = env['loop'].TranscriptionLoop(p, heads=heads, iters=iters, groups=(0, 1, 2)).setup_device()
    L = p.H * (p.timing_frames - 1)
    wave, _ = synth.make_windows(B, L, seed=21, notes_per_window=(1, 3), groups=(0, 1, 2), max_onset=0.3, device='cuda')
    b = lp.prepare(wave)
    refs = {k: v.clone() for k, v in lp.refs.items()}
    st = lp.prepare_songs([w for w in wave], refs=refs, spectra=b)
    assert torch.equal(st.batch.mag, b.mag) and torch.equal(st.batch.ph, b.ph)
    ev_s = lp.walk_songs(st, max_notes=iters, silence=0.0, poll=1, max_steps=iters).cpu().numpy()
    # run()'s iterations on the same AudioBatch
    lp.refs = refs
    ev_r = torch.empty((iters, B, 7), dtype=torch.int32, device='cuda')
    for it in range(iters):
        lp.iterate(b, it, ev_r)
    ev_r = ev_r.cpu().numpy()
    assert np.all(ev_s[:iters, :, 2] == so.DETECT), ev_s[:iters, :, 2]
    assert np.array_equal(ev_s[:iters, :, 3:8], ev_r[:, :, 2:7])
    assert ev_s.shape[0] == iters and torch.equal(st.batch.mag, b.mag) and torch.equal(st.batch.ref_max, b.ref_max)


def test_spectra_and_refs_go_through_the_admission(env):
    """prepare_songs(refs=, spectra=) is the one admission with two of its inputs given.  As the test above with three
    songs and two iterations, on a spectrogram that is NOT the songs' STFT (magnitudes, maxima and ref_mag halved: exact,
    so the features are the same floats), so that only a copy from `spectra` can put it into the windows: the AudioBatch
    is unchanged afterwards, the state's normalisers are the given ones, and none is computed -- the loop's normaliser
    tables are None during the call."""
    torch, synth = env['torch'], env['synth']
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    heads, iters, B = ('timing', 'pitch', 'instrument', 'velocity'), 2, 3
    lp = env['loop'].TranscriptionLoop(p, heads=heads, iters=iters, groups=(0, 1, 2)).setup_device()
    L = p.H * (p.timing_frames - 1)
    wave, _ = synth.make_windows(B, L, seed=21, notes_per_window=(1, 3), groups=(0, 1, 2), max_onset=0.3, device='cuda')
    b = lp.prepare(wave)
    b.mag.mul_(0.5)
    b.ref_max.mul_(0.5)
    refs = {k: v.clone() for k, v in lp.refs.items()}
    refs['ref_mag'].mul_(0.5)
    before = (b.mag.clone(), b.ph.clone(), b.ref_max.clone())
    given = {k: v.clone() for k, v in refs.items()}
    tabs = (lp.tab_ref1, lp.tab_refi, lp.tab_reff)
    lp.tab_ref1 = lp.tab_refi = lp.tab_reff = None
    try:
        st = lp.prepare_songs([w for w in wave], refs=refs, spectra=b)
    finally:
        lp.tab_ref1, lp.tab_refi, lp.tab_reff = tabs
    assert torch.equal(b.mag, before[0]) and torch.equal(b.ph, before[1]) and torch.equal(b.ref_max, before[2])
    assert torch.equal(st.batch.mag, b.mag) and torch.equal(st.batch.ph, b.ph)
    assert set(st.refs) == set(given)
    for k, v in given.items():
        assert torch.equal(st.refs[k], v) and torch.equal(refs[k], v), k
    assert st.slot_song.tolist() == [0, 1, 2] and st.finished.tolist() == [0, 0, 0]
    ev_s = lp.walk_songs(st, max_notes=iters, silence=0.0, poll=1, max_steps=iters).cpu().numpy()
    lp.refs = refs
    ev_r = torch.empty((iters, B, 7), dtype=torch.int32, device='cuda')
    for it in range(iters):
        lp.iterate(b, it, ev_r)
    ev_r = ev_r.cpu().numpy()
    assert np.all(ev_s[:iters, :, 2] == so.DETECT), ev_s[:iters, :, 2]
    assert np.array_equal(ev_s[:iters, :, 3:8], ev_r[:, :, 2:7])
    assert ev_s.shape[0] == iters and torch.equal(st.batch.mag, b.mag) and torch.equal(st.batch.ref_max, b.ref_max)


def test_full_depth_fixture(env):
    """The walk at the production window (516 frames, half = 258, the real 33-layer heads) against the committed CPU
    restatement (tests/golden/gen_song_fixtures.py): integer events bit-exact, every pre-rounding head float inside
    oracle/compare.py's bands, the final residual window (per-frame maxima and 20-band compression) to 1e-4 of its
    maximum; the product's song-level normalisers against the restatement's own, on which both walks run."""
    torch = env['torch']
    from oracle import audio as oa
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'song_fixtures.npz'))
    c = so.FULL
    p = env['hp'].Hyperparams(N=c['n_fft'])
    assert p.timing_frames == 516
    cand = so.make_songs(p, c['seed'], c['lengths'], gap=c['gap'], quantise=True)
    songs = [cand[int(k)] for k in fx['full_kept']]
    assert len(songs) >= 2
    for j, w in enumerate(songs):
        assert len(w) == int(fx['full_%d_samples' % j])
        assert abs(np.abs(w.astype(np.float64)).sum() - float(fx['full_%d_wave_sum' % j])) < 1e-6
    keys = ('ref_mag', 'ref_C_1', 'ref_C_foc')
    orefs = {k: np.array([fx['full_%d_refs' % j][i] for j in range(len(songs))], np.float32) for i, k in enumerate(keys)}
    lp = env['loop'].TranscriptionLoop(p, heads=so.HEADS).setup_device()
    own = lp.prepare_songs(songs).refs
    for k in keys:
        rel = np.abs(own[k].cpu().numpy() - orefs[k]) / orefs[k]
        assert rel.max() < 1e-4, ('normaliser', k, rel)
    lp.trace = []
    events, st = lp.run_songs(songs, max_notes=c['max_notes'], silence=c['silence'], poll=2,
                              refs={k: torch.from_numpy(v).cuda() for k, v in orefs.items()})
    trace, lp.trace = [{k: v.cpu().numpy() for k, v in t.items()} for t in lp.trace], None
    ev = events.cpu().numpy()
    bands = bands_for(p)
    half, F = p.timing_frames // 2, p.N // 2 + 1
    mags = st.batch.mag.cpu().numpy()
    for j in range(len(songs)):
        want = so.pad_finished(fx['full_%d_events' % j], ev.shape[0], j, half)
        want[:, 0] = j                                             # the generator walks every song on its own, as song 0
        assert np.array_equal(ev[:, j, :], want), ('events', j, ev[:, j, :].tolist(), want.tolist())
        for name, step, y in zip(fx['full_%d_dec_name' % j], fx['full_%d_dec_step' % j], fx['full_%d_dec_float' % j]):
            d = abs(float(trace[int(step)][str(name)][j].ravel()[0]) - float(y))
            print('full song %d step %d %s product-oracle %.2e' % (j, step, name, d))
            assert d <= bands[str(name)], ('float', j, str(name), int(step), d)
        mag = mags[j][:, :F].T
        fmax, bands20 = fx['full_%d_fmax' % j], fx['full_%d_bands' % j]
        scale = max(float(fmax.max()), 1e-30)
        assert np.abs(mag.max(axis=0) - fmax).max() / scale < 1e-4
        assert np.abs(oa.AudioCompleteOracle.compress_bands(mag, bands=p.timing_bands) - bands20).max() / scale < 1e-4
    assert np.any(ev[:, :, 2] == so.DETECT) and np.any(ev[:, :, 2] != so.DETECT)


def test_run_songs_argument_checks(env):
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    lp = env['loop'].TranscriptionLoop(p, heads=('timing', 'pitch')).setup_device()
    song = np.zeros(p.H * 50, np.float32)
    with pytest.raises(ValueError):
        lp.run_songs([])
    with pytest.raises(ValueError, match='Invalid Input shape'):
        lp.run_songs([song, song[:p.H - 1]])
    with pytest.raises(ValueError):
        lp.run_songs([song], max_notes=0)
    odd = env['loop'].TranscriptionLoop(env['hp'].Hyperparams(N=4096, window_size_note_time=1), heads=('timing',))
    with pytest.raises(ValueError, match='Invalid Input shape'):
        odd.setup_device().run_songs([song])                        # 43 frames: the halves of the window overlap
    with pytest.raises(ValueError):
        env['loop'].TranscriptionLoop(p, heads=('pitch',)).setup_device().run_songs([song])


def test_transcribe_song_traversal(env, tmp_path):
    """transcribe(traversal='song'): notes with absolute times inside the song, none reported twice across a half-window
    boundary, MIDI round trip; traversal='windows' is the default path, unchanged."""
    from amt_saga import events, transcribe as tr
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    L = p.H * (p.timing_frames - 1)
    n = int(3.2 * L)
    notes_in = [(0, 60, 100, 0.2, 0.5), (0, 64, 90, 0.9, 0.4), (1, 67, 80, 1.6, 0.6), (2, 72, 110, 2.4, 0.3)]
    wf = osynth.render_window(notes_in, n, p.sr).numpy()
    heads = ('timing', 'pitch', 'instrument', 'velocity')
    notes, evs = tr.transcribe(wf, p, iters=2, heads=heads, traversal='song')
    assert evs.ndim == 3 and evs.shape[1:] == (1, 9)
    det = evs[evs[:, 0, 2] == so.DETECT, 0, :]
    assert len(notes) == len(det) > 0
    dur = n / p.sr
    assert all(0 <= e['start'] < e['end'] and e['start'] < dur and 21 <= e['pitch'] <= 108 for e in notes)
    # one live window: a frame of the song is looked at from one residual only, so no (pitch, program, onset frame)
    # comes twice the way the overlapped windows report it
    # ... also not a few frames apart: the tolerance merge_overlap_duplicates uses for the overlapped windows (0.05 s)
    for i, a in enumerate(notes):
        for b2 in notes[i + 1:]:
            if a['pitch'] == b2['pitch'] and a['program'] == b2['program'] and a['window'] != b2['window']:
                assert abs(a['start'] - b2['start']) > 0.05, (a, b2)
    mid = str(tmp_path / 'song.mid')
    events.write_midi(notes, mid)
    rd = events.read_midi(mid)
    assert len(rd) == len(notes)
    key = lambda e: (e['pitch'], e['program'], round(e['start'] * events.TICKS_PER_SECOND))
    assert sorted(key(e) for e in rd) == sorted(key(e) for e in notes)
    a_notes, a_evs = tr.transcribe(wf, p, iters=2, heads=heads)
    b_notes, b_evs = tr.transcribe(wf, p, iters=2, heads=heads, traversal='windows')
    assert np.array_equal(a_evs, b_evs) and a_notes == b_notes and a_evs.shape[2] == 7
    with pytest.raises(ValueError):
        tr.transcribe(wf, p, traversal='nope')
    path = str(tmp_path / 'clip.flac')
    from amt_saga import flac
    flac.save_float(wf, path, p.sr)
    tr.main([path, str(tmp_path / 'cli.mid'), '--iters', '1', '--traversal', 'song'])
    assert os.path.getsize(str(tmp_path / 'cli.mid')) > 20
