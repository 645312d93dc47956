"""GPU: the residual audio of a song walk -- amt_song_slide_keep against numpy, amt_istft_ragged bit for bit against
amt_istft per signal, the live walk's residual spectrogram against the one assembled from the CPU restatement
(tests/song_residual_oracle.py), the queue against run_songs on every song alone, transcribe() and the command line."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import song_oracle as so                                        # noqa: E402
import song_residual_oracle as sro                              # noqa: E402
from oracle import audio as oa                                  # noqa: E402
from oracle import synth as osynth                              # noqa: E402
from oracle.compare import bands_for                            # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-4                                                      # tests/test_gpu_audio.py: relative to the maximum


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import synth, loop, hyperparams, audio, _lib
    return dict(torch=torch, synth=synth, loop=loop, hp=hyperparams, audio=audio, _lib=_lib, lib=_lib.load())


def _make_loop(env, nfft, wsec, guess, shift=0, heads=so.HEADS):
    p = env['hp'].Hyperparams(N=nfft, window_size_note_time=wsec)
    lp = env['loop'].TranscriptionLoop(p, heads=heads, guess=guess)
    if shift:
        w = {k: v.copy() for k, v in lp.nets['timing_start'].weights.items()}
        w['dense2/bias'] = w['dense2/bias'] + np.float32(shift)
        lp.nets['timing_start'].set_weights(w)
    return p, lp.setup_device()


@pytest.fixture(scope='module')
def bank2048(env):
    """One loop (2048-point, 86-frame windows, bank guess) shared by the tests that do not change its weights."""
    return _make_loop(env, 2048, 1, 'bank')


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _stft(env, p, wave):
    w = wave if env['torch'].is_tensor(wave) else env['torch'].from_numpy(np.asarray(wave, np.float32)).cuda()
    return env['audio'].AudioBatch(w.reshape(1, -1), p.N, p.H).stft(with_phase=True)


def _relmax(a, b):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-30)


# ---- 1. the slide that keeps the outgoing half ---------------------------------------------------------------------------
def test_slide_keep_vs_numpy(env):
    """amt_song_slide_keep on six slots whose regions lie next to each other in one pool, sentinel rows before, between
    and after them.  Window and state: exactly amt_song_slide's on a copy.  Pool: the written rows are the old window
    rows 0 .. 42, cropped to the song -- 30 rows of a song shorter than half a window; ONE row of a song that ends one
    row into the outgoing half, several halves in; 42 rows (the song's last frame is the half's last row but one); all
    43 of a song that ends exactly on the half's boundary and of a long one -- and every other float of the pool, all
    of s_ph, the sentinels and the region of the slot that does not slide (between two that do) are untouched."""
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    rng = np.random.default_rng(17)
    T, half, ldf, gap = 86, 43, 132, 2
    t_song = [30, 130, 200, 85, 129, 400]
    offs = [0, 129, 43, 43, 86, 172]
    mask = [1, 1, 0, 1, 1, 1]
    rows = [30, 1, 0, 42, 43, 43]                                  # pool rows each slot must write
    B = len(t_song)
    fbase, at = [], gap
    for t in t_song:
        fbase.append(at)
        at += t + gap
    pool = at
    s_mag = rng.standard_normal((pool, ldf)).astype(np.float32)
    s_ph = rng.standard_normal((pool, ldf, 2)).astype(np.float32)
    sentinel = np.ones(pool, bool)
    for f, t in zip(fbase, t_song):
        sentinel[f:f + t] = False
    s_mag[sentinel], s_ph[sentinel] = -7.0, -7.0
    assert sentinel.sum() == gap * (B + 1)
    w_mag = rng.standard_normal((B, T, ldf)).astype(np.float32)
    w_ph = rng.standard_normal((B, T, ldf, 2)).astype(np.float32)
    count = rng.integers(1, 5, B).astype(np.int32)

    def state():
        return dict(wm=torch.from_numpy(w_mag).cuda(), wp=torch.from_numpy(w_ph).cuda(), sm=torch.from_numpy(s_mag).cuda(),
                    sp=torch.from_numpy(s_ph).cuda(), fb=torch.from_numpy(np.asarray(fbase, np.int64)).cuda(),
                    ts=_i32(torch, t_song), sl=_i32(torch, mask), off=_i32(torch, offs), cnt=_i32(torch, count),
                    fin=_i32(torch, np.zeros(B)))

    def call(fn, d, t=T):
        return fn(d['wm'].data_ptr(), d['wp'].data_ptr(), B, t, ldf, T * ldf, d['sm'].data_ptr(), d['sp'].data_ptr(),
                  d['fb'].data_ptr(), d['ts'].data_ptr(), d['sl'].data_ptr(), d['off'].data_ptr(), d['cnt'].data_ptr(),
                  d['fin'].data_ptr(), None)
    ref, got = state(), state()
    assert call(lib.amt_song_slide, ref) == _lib.AMT_OK
    assert call(lib.amt_song_slide_keep, got, 85) == _lib.AMT_E_INVALID      # odd window: rejected, nothing launched
    assert call(lib.amt_song_slide_keep, got) == _lib.AMT_OK
    torch.cuda.synchronize()
    for k in ('wm', 'wp', 'off', 'cnt', 'fin'):
        assert torch.equal(ref[k], got[k]), k
    assert got['fin'].cpu().tolist() == [1, 1, 0, 1, 1, 0]
    assert np.array_equal(ref['sm'].cpu().numpy(), s_mag)          # the plain slide never writes the pool
    want = s_mag.copy()
    for b in range(B):
        if mask[b]:
            n = int(np.clip(t_song[b] - offs[b], 0, half))
            assert n == rows[b]
            want[fbase[b] + offs[b]:fbase[b] + offs[b] + n] = w_mag[b, :n]
    pm = got['sm'].cpu().numpy()
    assert np.array_equal(pm, want)
    assert np.all(pm[sentinel] == -7.0)
    assert np.array_equal(pm[fbase[2]:fbase[2] + t_song[2]], s_mag[fbase[2]:fbase[2] + t_song[2]])
    assert int((pm != s_mag).any(axis=1).sum()) == sum(rows)       # (random floats: a written row differs)
    assert np.array_equal(got['sp'].cpu().numpy(), s_ph)


# ---- 2. the song-length inverse transform --------------------------------------------------------------------------------
def _istft_one(env, plan, mag, ph, T, hop, ldf):
    torch = env['torch']
    out = torch.empty(hop * (T - 1), device='cuda')
    st = env['lib'].amt_istft(plan, mag.data_ptr(), ph.data_ptr(), 1, T, ldf, T * ldf, out.data_ptr(), out.numel(), None)
    assert st == env['_lib'].AMT_OK
    return out


def _ragged_case(env, nfft, t_frames, rng, overflow=None):
    """One amt_istft_ragged launch over regions in shuffled order with gaps, odd out_base values; every signal against
    amt_istft (B = 1) on its region, bit for bit; nothing else in the output touched.  overflow: index of a signal
    whose samples are made to pass n_out -- it must stay unwritten, the others correct."""
    torch, lib, _lib, audio = env['torch'], env['lib'], env['_lib'], env['audio']
    hop, ldf = nfft // 4, audio.ldf_of(nfft)
    plan = audio._plan(nfft, hop, True)
    n = len(t_frames)
    lens = [hop * (t - 1) for t in t_frames]
    fb, ob, f_at, o_at = np.zeros(n, np.int64), np.zeros(n, np.int64), 3, 5
    order = [int(i) for i in rng.permutation(n)]
    if overflow is not None:                                       # the overflowing signal comes last in the output
        order = [i for i in order if i != overflow] + [overflow]
    for i in order:
        fb[i], ob[i] = f_at, o_at
        f_at += t_frames[i] + int(rng.integers(0, 3))
        o_at += lens[i] + 1 + 2 * int(rng.integers(0, 3))          # odd steps from 5: bases of every alignment
    assert any(int(v) % 4 for v in ob)                             # at least one out_base is no multiple of 4
    pool_frames, n_out = f_at + 2, o_at + 3
    if overflow is not None:
        n_out = int(ob[overflow]) + lens[overflow] - 1             # one sample short
    gen = torch.Generator(device='cuda').manual_seed(nfft + n)
    mag = torch.rand((pool_frames, ldf), device='cuda', generator=gen)
    ph = torch.randn((pool_frames, ldf, 2), device='cuda', generator=gen)
    ph = ph / ph.norm(dim=2, keepdim=True)
    out = torch.full((max(n_out, o_at + 3),), -7.0, device='cuda')
    d_fb, d_ob, d_t = torch.from_numpy(fb).cuda(), torch.from_numpy(ob).cuda(), _i32(torch, t_frames)
    st = lib.amt_istft_ragged(plan, mag.data_ptr(), ph.data_ptr(), d_fb.data_ptr(), d_t.data_ptr(), n, max(t_frames),
                              pool_frames, ldf, out.data_ptr(), d_ob.data_ptr(), n_out, None)
    assert st == _lib.AMT_OK
    torch.cuda.synchronize()
    written = torch.zeros(out.numel(), dtype=torch.bool, device='cuda')
    for i in range(n):
        if i == overflow or lens[i] == 0:
            continue
        one = _istft_one(env, plan, mag[fb[i]:fb[i] + t_frames[i]], ph[fb[i]:fb[i] + t_frames[i]], t_frames[i], hop, ldf)
        assert torch.equal(out[ob[i]:ob[i] + lens[i]], one), (nfft, t_frames[i], 'signal %d' % i)
        assert float(one.abs().max()) > 0
        written[ob[i]:ob[i] + lens[i]] = True
    assert bool((out[~written] == -7.0).all())                     # sentinels: only the signals' own ranges changed
    return plan, mag, ph, d_fb, d_ob, d_t, pool_frames, n_out, out


@pytest.mark.parametrize('nfft', [2048, 4096])
def test_ragged_istft_bit_identical(env, nfft):
    """t_frames 3, 4, 87 (22 segments) and 10 / 11 / 12: a signal of T frames is hop * (T + 1) padded samples, cut in
    segments of 4 hops (what amt_istft takes for one signal of this size), so T = 11 ends ON a segment boundary, 10 one
    frame below and 12 one above it.  A one-frame signal has no samples and writes nothing.  Then: a signal whose samples
    pass n_out is left unwritten while the others are correct; a longer signal than max_frames is left unwritten;
    plans outside the streaming form are AMT_E_UNSUPPORTED."""
    torch, lib, _lib, audio = env['torch'], env['lib'], env['_lib'], env['audio']
    rng = np.random.default_rng(nfft + 1)
    t_frames = [3, 4, 87, 10, 11, 12, 1]
    _ragged_case(env, nfft, [87], rng)
    _ragged_case(env, nfft, t_frames, rng)
    _ragged_case(env, nfft, t_frames, rng, overflow=2)
    hop, ldf = nfft // 4, audio.ldf_of(nfft)
    plan, mag, ph, d_fb, d_ob, d_t, pool_frames, n_out, out = _ragged_case(env, nfft, [5, 9], rng)
    # max_frames below the longest signal: that signal is skipped as a whole, the other is written
    before = out.clone()
    out.fill_(-7.0)
    assert lib.amt_istft_ragged(plan, mag.data_ptr(), ph.data_ptr(), d_fb.data_ptr(), d_t.data_ptr(), 2, 5, pool_frames, ldf,
                                out.data_ptr(), d_ob.data_ptr(), n_out, None) == _lib.AMT_OK
    torch.cuda.synchronize()
    ob = d_ob.cpu().numpy()
    assert torch.equal(out[ob[0]:ob[0] + hop * 4], before[ob[0]:ob[0] + hop * 4])
    assert bool((out[ob[1]:ob[1] + hop * 8] == -7.0).all())
    # a region that leaves the pool: skipped
    out.fill_(-7.0)
    assert lib.amt_istft_ragged(plan, mag.data_ptr(), ph.data_ptr(), d_fb.data_ptr(), d_t.data_ptr(), 2, 9, 4, ldf,
                                out.data_ptr(), d_ob.data_ptr(), n_out, None) == _lib.AMT_OK
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    for bad in (audio._plan(nfft, nfft // 8, True), audio._plan(nfft, hop, False), audio._plan(512, 128, True)):
        assert lib.amt_istft_ragged(bad, mag.data_ptr(), ph.data_ptr(), d_fb.data_ptr(), d_t.data_ptr(), 2, 9, pool_frames,
                                    ldf, out.data_ptr(), d_ob.data_ptr(), n_out, None) == _lib.AMT_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_ragged_istft_longer_segments(env):
    """The one size at which the cut changes: amt_istft gives ONE signal segments of 8 hops once 4-hop segments would
    come to more than 2 x 2047 of them, i.e. from 16376 frames on.  One frame below and on that threshold, with a short
    signal between them in the same launch: each bit-identical to amt_istft on it alone."""
    _ragged_case(env, 2048, [16375, 6, 16376], np.random.default_rng(5))


# ---- 3. the live walk ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['bank2048', 'plain_slides', 'bank4096'])
def test_walk_residual_vs_cpu_restatement(env, case):
    """run_songs(residual=True) on the screened seeds of song_oracle.WALK_CASES (events bit-exact, test_gpu_song_loop):
    each song's pool region against the residual assembled from the restatement's windows, to 1e-4 of the song's
    spectrogram maximum (the bar test_walk_vs_cpu_restatement applies to the final window); the region's phases
    bit-identical to a fresh STFT of the song; the residual waveform against oracle.audio.istft of the PRODUCT's own
    residual spectrogram times those phases, to REL of its maximum -- so the spectrogram's and the transform's errors are
    judged apart."""
    nfft, wsec, guess, seed, lengths, max_notes, silence, silent, shift = so.WALK_CASES[case]
    torch = env['torch']
    p, lp = _make_loop(env, nfft, wsec, guess, shift)
    songs = so.make_songs(p, seed, lengths, silent)
    events, st = lp.run_songs(songs, max_notes=max_notes, silence=silence, poll=4, song0=3, residual=True)
    torch.cuda.synchronize()
    ev = events.cpu().numpy()
    B = len(songs)
    assert st.finished.cpu().tolist() == [1] * B and len(st.residual) == B
    bank = osynth.guess_bank_waves((0,), p.pitch_low, p.pitch_high, sr=p.sr)
    orc = so.SongOracle(p, so.HEADS, {k: n.weights for k, n in lp.nets.items()}, bank_waves=bank)
    bands = bands_for(p)
    refs = {k: v.cpu().numpy() for k, v in st.refs.items()}
    F, half = p.N // 2 + 1, p.timing_frames // 2
    subtracted = 0
    for i, wave in enumerate(songs):
        t = 1 + len(wave) // p.H
        f0 = st.region[i]
        wins = []
        ev_ref, _ = orc.run_song(wave, {k: float(v[i]) for k, v in refs.items()}, max_notes, silence, song_id=3 + i,
                                 force=(ev[:, i, :], bands), windows=wins)
        assert np.array_equal(ev[:, i, :], so.pad_finished(ev_ref, ev.shape[0], 3 + i, half)), ('events', i)
        song = oa.AudioCompleteOracle(np.asarray(wave, np.float32), p.N, p.H)
        want = sro.assemble_residual(song, ev_ref, wins, p.timing_frames)
        got = st.s_mag[f0:f0 + t].cpu().numpy()
        full = np.asarray(song.mag, np.float32)
        scale = float(full.max())
        err = np.abs(got[:, :F].T - want).max() / scale
        print('%s song %d: %d frames, residual spectrogram product-oracle %.2e of the maximum' % (case, i, t, err))
        assert err < 1e-4, ('residual spectrogram', i, err)
        assert np.all(got[:, F:] == 0)
        subtracted += int(np.any(want < full))
        fresh = _stft(env, p, wave)
        assert fresh.T == t and torch.equal(st.s_ph[f0:f0 + t], fresh.ph[0]), ('phases', i)
        y = st.residual[i]
        assert y.dtype == torch.float32 and tuple(y.shape) == (p.H * (t - 1),)
        ph = st.s_ph[f0:f0 + t].cpu().numpy()
        ref = oa.istft(got[:, :F].T * (ph[:, :F, 0] + 1j * ph[:, :F, 1]).T, p.H)
        werr = _relmax(y.cpu().numpy(), ref)
        print('%s song %d: residual waveform product-oracle %.2e of the maximum' % (case, i, werr))
        assert werr < REL, ('residual waveform', i, werr)
    if not shift:
        assert subtracted > 0                                      # the case detects: something was taken out


# ---- 4. nothing detected, 5. opt-in ---------------------------------------------------------------------------------------
def test_nothing_detected_and_opt_in(env, bank2048):
    """silence so large that every step is a forced slide: the residual region is the song's STFT magnitudes bit for bit
    and the residual waveform is amt_istft of that spectrogram bit for bit.  Opt-in: without residual=True the pool after
    a full, detecting walk is bit-identical to the STFT (nothing writes it), state.residual is None, and the events of the
    same walk with residual=True are identical."""
    torch = env['torch']
    p, lp = bank2048
    songs = so.make_songs(p, 23, (2.3, 0.6, 3.0, 4.4))
    ev, st = lp.run_songs(songs, max_notes=2, silence=1e9, poll=4, residual=True)
    e = ev.cpu().numpy()
    assert not np.any(e[:, :, 2] == so.DETECT) and np.any(e[:, :, 2] == so.FORCED_SLIDE)
    for i, wave in enumerate(songs):
        fresh = _stft(env, p, wave)
        t, f0 = fresh.T, st.region[i]
        assert torch.equal(st.s_mag[f0:f0 + t], fresh.mag[0]) and torch.equal(st.s_ph[f0:f0 + t], fresh.ph[0]), i
        one = _istft_one(env, fresh.plan, fresh.mag, fresh.ph, t, p.H, fresh.ldf)
        assert torch.equal(st.residual[i], one), i
    ev0, st0 = lp.run_songs(songs, max_notes=2, silence=1e-4, poll=4)
    ev1, st1 = lp.run_songs(songs, max_notes=2, silence=1e-4, poll=4, residual=True)
    assert np.any(ev0.cpu().numpy()[:, :, 2] == so.DETECT)
    assert torch.equal(ev0, ev1)
    assert st0.residual is None and not st0.keep_residual and st1.keep_residual
    assert torch.equal(st0.batch.mag, st1.batch.mag) and torch.equal(st0.batch.ph, st1.batch.ph)
    assert torch.equal(st0.s_ph, st1.s_ph) and not torch.equal(st0.s_mag, st1.s_mag)
    for i, wave in enumerate(songs):
        fresh = _stft(env, p, wave)
        f0 = st0.region[i]
        assert torch.equal(st0.s_mag[f0:f0 + fresh.T], fresh.mag[0]), i
        assert bool((st1.s_mag[f0:f0 + fresh.T] <= fresh.mag[0]).all()) and bool((st1.s_mag[f0:f0 + fresh.T] >= 0).all())
    with pytest.raises(ValueError, match='keep_residual'):
        st0.residual_waves([0])
    with pytest.raises(ValueError, match='keep_residual'):
        lp.walk_songs(lp.prepare_songs(songs[:1]), residual=True)


# ---- 6. the queue ---------------------------------------------------------------------------------------------------------
def test_queue_residual_equals_run_songs(env, bank2048):
    """Five songs of different lengths through 2 slots and a pool of 2 x the longest song's frames + 40, small enough that
    regions are handed out again (the pool is never larger than three of the five songs): every yielded residual is
    run_songs([song], residual=True)'s, bit for bit, and so are the records; run_song_queue pairs them in queue order.  A
    max_steps-cut fixed batch: None for the unfinished song, ValueError from residual_waves for its slot."""
    torch = env['torch']
    p, lp = bank2048
    songs = so.make_songs(p, 29, (3.1, 1.4, 4.0, 0.7, 2.6))
    frames = [1 + len(s) // p.H for s in songs]
    pool = 2 * max(frames) + 40
    assert pool < sum(sorted(frames)[-3:])
    alone = []
    for s in songs:
        ev, st = lp.run_songs([s], max_notes=2, silence=1e-4, poll=16, residual=True)
        e = ev.cpu().numpy()[:, 0, :]
        alone.append((e[e[:, 2] != so.FINISHED], st.residual[0].clone()))
    regions, got = [], {}
    for idx, evs, res in lp.iter_song_queue(iter(songs), 2, max_notes=2, silence=1e-4, poll=4, pool_frames=pool,
                                            on_finish=lambda i, slot, st: regions.append(st.region[slot]), residual=True):
        got[idx] = (evs, res.clone())
    assert sorted(got) == list(range(5)) and len(set(regions)) < 5          # a region was used twice
    for i, (e, res) in enumerate(alone):
        assert np.array_equal(got[i][0][:, 2:], e[:, 2:]), i
        assert tuple(res.shape) == (p.H * (frames[i] - 1),)
        assert torch.equal(got[i][1], res), ('residual of song %d' % i)
    pairs = lp.run_song_queue(iter(songs), 2, max_notes=2, silence=1e-4, poll=4, pool_frames=pool, residual=True)
    assert len(pairs) == 5 and all(torch.equal(r, alone[i][1]) for i, (_, r) in enumerate(pairs))
    plain = lp.run_song_queue(iter(songs), 2, max_notes=2, silence=1e-4, poll=4, pool_frames=pool)
    assert all(np.array_equal(a, b[0]) for a, b in zip(plain, pairs))
    # a cut walk: the short song (0.7 half windows: one slide) is finished after two steps, the long one is not
    st = lp.prepare_songs([songs[3], songs[2]], keep_residual=True)
    lp.walk_songs(st, max_notes=2, silence=1e9, poll=1, max_steps=2, residual=True)
    assert st.finished.cpu().tolist() == [1, 0]
    assert st.residual[1] is None and torch.equal(st.residual[0], st.residual_waves([0])[0])
    with pytest.raises(ValueError, match='not finished'):
        st.residual_waves([0, 1])
    with pytest.raises(ValueError):
        st.residual_waves([2])


# ---- 7. transcribe and the command line ----------------------------------------------------------------------------------
def test_transcribe_residual_and_command_line(env, tmp_path):
    """transcribe(traversal='song', residual=True) returns (notes, events, residual); the command line writes the same
    residual through flac.save_float: the file decodes with CRC and MD5 verified, holds hop * (T - 1) samples at the
    model's rate and equals the returned residual after the writer's 24-bit quantisation.  --songs --residual-dir writes
    <stem>.residual.flac per song."""
    from amt_saga import flac, transcribe as tr
    p = env['hp'].Hyperparams(N=2048, sr=44100)                   # the command line's model: 516-frame windows
    n = int(1.3 * p.H * (p.timing_frames - 1))
    notes_in = [(0, 60, 100, 0.2, 0.5), (0, 64, 90, 0.9, 0.4), (1, 67, 80, 2.6, 0.6), (2, 72, 110, 5.4, 0.3)]
    wf = osynth.render_window(notes_in, n, p.sr).numpy()
    src = str(tmp_path / 'clip.flac')
    flac.save_float(wf, src, p.sr)
    wf24 = flac.load_float(src)[0]                                 # what the command line reads
    lp = tr._make_loop(p, 1, ('timing', 'pitch', 'instrument', 'velocity'), (0, 1, 2), None, 'bank')   # transcribe()'s own
    notes, evs, res = tr.transcribe(wf24, p, iters=1, traversal='song', residual=True, loop=lp)
    plain = tr.transcribe(wf24, p, iters=1, traversal='song', loop=lp)
    assert len(plain) == 2 and np.array_equal(plain[1], evs) and plain[0] == notes
    T = 1 + n // p.H
    assert res.is_cuda and tuple(res.shape) == (p.H * (T - 1),)
    with pytest.raises(ValueError, match='residual'):
        tr.transcribe(wf24, p, iters=1, residual=True, loop=lp)
    out = str(tmp_path / 'left.flac')
    tr.main([src, str(tmp_path / 'cli.mid'), '--iters', '1', '--traversal', 'song', '--residual', out])
    pcm, sr, bps = flac.decode(out, verify=True)
    assert (sr, bps) == (p.sr, 24) and pcm.shape == (p.H * (T - 1), 1)
    y = res.cpu().numpy().astype(np.float64)
    want = np.clip(np.rint(y * 8388608.0), -8388608, 8388607).astype(np.int64)
    assert np.array_equal(pcm[:, 0], want) and np.any(want != 0)
    with pytest.raises(SystemExit, match='--traversal song'):
        tr.main([src, str(tmp_path / 'x.mid'), '--iters', '1', '--residual', str(tmp_path / 'x.flac')])
    other = str(tmp_path / 'other.flac')
    flac.save_float(wf[:n // 2], other, p.sr)
    rdir = str(tmp_path / 'res')
    tr.main(['--songs', src, other, '--out-dir', str(tmp_path / 'mid'), '--slots', '2', '--iters', '1',
             '--residual-dir', rdir])
    pcm2, sr2, _ = flac.decode(os.path.join(rdir, 'clip.residual.flac'), verify=True)
    assert sr2 == p.sr and np.array_equal(pcm2[:, 0], want)         # the queue's residual is run_songs' for the song alone
    pcm3, _, _ = flac.decode(os.path.join(rdir, 'other.residual.flac'), verify=True)
    assert pcm3.shape == (p.H * (n // 2 // p.H), 1)
    assert sorted(os.listdir(str(tmp_path / 'mid'))) == ['clip.mid', 'other.mid']
