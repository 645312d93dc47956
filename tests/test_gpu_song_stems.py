"""GPU: the instrument stems of a song walk -- amt_subtract_span_stems against numpy float32 bit for bit, the live walk's
identity STFT magnitude = residual + sum of stems within its derived bound, stem 0 against the stems assembled from the
CPU restatement (tests/song_stems_oracle.py), the queue against run_songs on every song alone, transcribe() and both
modes of the command line."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import song_oracle as so                                        # noqa: E402
import song_stems_oracle as sso                                 # noqa: E402
from oracle import audio as oa                                  # noqa: E402
from oracle import synth as osynth                              # noqa: E402
from oracle.compare import bands_for                            # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-4                                                      # tests/test_gpu_song_residual.py: relative to the maximum
U = 2.0 ** -24                                                  # unit roundoff of float32
ALL_HEADS = ('timing', 'pitch', 'instrument', 'velocity')


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import synth, loop, hyperparams, audio, _lib
    return dict(torch=torch, synth=synth, loop=loop, hp=hyperparams, audio=audio, _lib=_lib, lib=_lib.load())


def _make_loop(env, nfft, wsec, guess, shift=0, heads=so.HEADS, groups=(0,)):
    p = env['hp'].Hyperparams(N=nfft, window_size_note_time=wsec)
    lp = env['loop'].TranscriptionLoop(p, heads=heads, guess=guess, groups=groups)
    if shift:
        w = {k: v.copy() for k, v in lp.nets['timing_start'].weights.items()}
        w['dense2/bias'] = w['dense2/bias'] + np.float32(shift)
        lp.nets['timing_start'].set_weights(w)
    return p, lp.setup_device()


@pytest.fixture(scope='module')
def grouped2048(env):
    """One loop (2048-point, 86-frame windows, bank guess) with the instrument head for real and three groups."""
    return _make_loop(env, 2048, 1, 'bank', heads=ALL_HEADS, groups=(0, 1, 2))


def _stft(env, p, wave):
    w = wave if env['torch'].is_tensor(wave) else env['torch'].from_numpy(np.asarray(wave, np.float32)).cuda()
    return env['audio'].AudioBatch(w.reshape(1, -1), p.N, p.H).stft(with_phase=True)


def _istft_one(env, plan, mag, ph, T, hop, ldf):
    out = env['torch'].empty(hop * (T - 1), device='cuda')
    st = env['lib'].amt_istft(plan, mag.data_ptr(), ph.data_ptr(), 1, T, ldf, T * ldf, out.data_ptr(), out.numel(), None)
    assert st == env['_lib'].AMT_OK
    return out


def identity_bound(orig, max_notes):
    """(2 max_notes + 2) 2^-24 orig, elementwise in float64: derived in tests/test_song_stems_cpu.py and DESIGN 14."""
    return (2 * int(max_notes) + 2) * U * np.asarray(orig, np.float64)


# ---- 1. the kernel against numpy float32 ------------------------------------------------------------------------------------
def _np_step(resid, stems, guess, c, fbase, pool, prog_group, n_prog, G):
    """numpy float32 restatement of one amt_subtract_span_stems launch, in place on resid [B, T, ldf] and stems
    [G, pool, ldf]; c: the launch's per-slot integers.  Returns the stem rows it wrote as (group, pool row)."""
    B, T = resid.shape[:2]
    wrote = []
    for b in range(B):
        g = int(c['gidx'][b])
        scale = np.float32(c['rmax'][b]) / np.float32(c['gmax'][g])
        off = max(int(c['onset'][b]), 0)
        t_end = min(off + int(c['gfr'][b]), T)
        grp = 0
        if c['program'] is not None and prog_group is not None:
            pr = min(max(int(c['program'][b]), 0), n_prog - 1)
            grp = int(prog_group[pr])
        grp = min(max(grp, 0), G - 1)
        for t in range(off, t_end):
            before = resid[b, t].copy()
            sub = (guess[g, t - off] * scale) * np.float32(c['overkill'])
            after = np.maximum(before - sub, np.float32(0))
            resid[b, t] = after
            sf = int(c['offset'][b]) + t
            row = fbase[b] + sf
            if 0 <= sf < int(c['t_song'][b]) and 0 <= row < pool:
                stems[grp, row] = stems[grp, row] + (before - after)
                wrote.append((grp, row))
    return wrote


@pytest.mark.parametrize('nfft', [2048, 4096])
def test_span_stems_kernel_vs_numpy(env, nfft):
    """T = 12, six slots over adjacent pool regions with two sentinel rows before, between and after them, G = 3, ldf 1028
    (257 float4 per row: four lane passes plus one lane) and 2052.  Launch 1: guess frames 0, 1, 5 and 7; a span clipped
    at T (slot 4); a span that crosses t_song (slot 2: song frames 10 .. 12 of a 10-frame song are the two sentinels
    behind it and slot 3's first row -- the window rows there are nonzero on purpose, the walk never has that); programs
    -1, 0 (both stem 1), n_prog + 3 and a table entry past G (both stem 2: two slots in one group), a negative entry.
    Launch 2: other, overlapping spans on the result (accumulation).  Launch 3: program NULL.  Launch 4: prog_group
    NULL.  Launch 5: a song that claims frames past the end of the pool -- those rows are skipped.  After every launch:
    stems equal numpy's in every float of the pool (sentinels, other songs' regions and other groups' stems included);
    residual, frame_max and new_max bit-identical to amt_subtract_span on a copy of the same inputs."""
    torch, lib, _lib, audio = env['torch'], env['lib'], env['_lib'], env['audio']
    rng = np.random.default_rng(nfft)
    ldf, F = audio.ldf_of(nfft), nfft // 2 + 1
    assert ldf == {2048: 1028, 4096: 2052}[nfft]
    B, T, G, Tg, gap, n_guess, n_prog = 6, 12, 3, 9, 2, 4, 5
    t_song = [30, 9, 10, 25, 40, 16]
    fbase, at = [], gap
    for t in t_song:
        fbase.append(at)
        at += t + gap
    pool = at
    sentinel = np.ones(pool, bool)
    for f, t in zip(fbase, t_song):
        sentinel[f:f + t] = False
    prog_group = np.array([1, 0, 7, -3, 2], np.int32)
    resid = rng.random((B, T, ldf)).astype(np.float32)
    guess = (rng.random((n_guess, Tg, ldf)) * 0.7).astype(np.float32)
    stems = rng.random((G, pool, ldf)).astype(np.float32)
    stems[:, sentinel] = -7.0
    gmax = guess[:, :, :F].max(axis=(1, 2))
    launches = [
        dict(gfr=[0, 1, 7, 5, 7, 5], onset=[3, 0, 4, 2, 9, 1], offset=[0, 4, 2, 12, 24, 0], program=[-1, 0, n_prog + 3, 2, 3, 1],
             table=True, overkill=1.25),
        dict(gfr=[6, 3, 7, 5, 2, 9], onset=[1, 0, 2, 4, 10, 0], offset=[0, 4, 2, 12, 24, 0], program=[1, 4, 0, 0, 2, 3],
             table=True, overkill=1.0),
        dict(gfr=[5, 1, 0, 7, 3, 2], onset=[0, 5, 1, 3, 8, 11], offset=[12, 0, 0, 6, 30, 6], program=None, table=True,
             overkill=0.5),
        dict(gfr=[1, 7, 5, 0, 5, 7], onset=[11, 1, 0, 0, 6, 4], offset=[18, 0, 0, 0, 28, 4], program=[4, 3, 2, 1, 0, -1],
             table=False, overkill=1.0),
        # slot 5 claims 100 frames: song frames 16, 17 are the sentinels behind its region, 18 .. lie past the pool
        dict(gfr=[0, 0, 0, 0, 0, 9], onset=[0, 0, 0, 0, 0, 2], offset=[0, 0, 0, 0, 0, 10], program=[0, 0, 0, 0, 0, 1],
             table=True, overkill=1.0, t_song=t_song[:5] + [100]),
    ]

    def dev(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()

    d_guess, d_gmax, d_pg = dev(guess), dev(gmax), dev(prog_group)
    d_fb = dev(fbase, np.int64)
    d_stems = dev(stems)
    for k, c in enumerate(launches):
        c = dict(c, gidx=rng.integers(0, n_guess, B).astype(np.int32), gmax=gmax, t_song=c.get('t_song', t_song))
        fmax = resid[:, :, :F].max(axis=2)
        c['rmax'] = fmax.max(axis=1)
        d_r, d_r0 = dev(resid), dev(resid)
        d_fm, d_fm0 = dev(fmax), dev(fmax)
        d_rmax, d_gidx = dev(c['rmax']), dev(c['gidx'])
        d_gfr, d_on, d_off, d_ts = (dev(c[n], np.int32) for n in ('gfr', 'onset', 'offset', 't_song'))
        d_prog = dev(c['program'], np.int32) if c['program'] is not None else None
        d_nm, d_nm0 = torch.full((B,), -1.0, device='cuda'), torch.full((B,), -1.0, device='cuda')

        def args(r, nm):
            a = _lib.SubtractArgs()
            a.resid, a.resid_max, a.guess, a.guess_max = r.data_ptr(), d_rmax.data_ptr(), d_guess.data_ptr(), d_gmax.data_ptr()
            a.guess_index, a.guess_frames, a.offset_frames = d_gidx.data_ptr(), d_gfr.data_ptr(), d_on.data_ptr()
            a.new_max, a.resid_stride, a.guess_stride = nm.data_ptr(), T * ldf, Tg * ldf
            a.B, a.T, a.ldf, a.F = B, T, ldf, F
            a.guess_frames_all, a.normalize, a.relu, a.overkill_factor = 0, 1, 1, float(c['overkill'])
            return a
        s = _lib.stem_args(stems=d_stems, frame_base=d_fb, offset=d_off, t_song=d_ts, program=d_prog,
                           prog_group=d_pg if c['table'] else None, n_prog=n_prog, G=G, pool_frames=pool)
        a0, a1 = args(d_r0, d_nm0), args(d_r, d_nm)
        assert lib.amt_subtract_span(ctypes.byref(a0), d_fm0.data_ptr(), Tg, None) == _lib.AMT_OK
        assert lib.amt_subtract_span_stems(ctypes.byref(a1), d_fm.data_ptr(), Tg, ctypes.byref(s), None) == _lib.AMT_OK
        torch.cuda.synchronize()
        assert torch.equal(d_r, d_r0) and torch.equal(d_fm, d_fm0) and torch.equal(d_nm, d_nm0), ('launch', k)
        before = stems.copy()
        wrote = _np_step(resid, stems, guess, c, fbase, pool, prog_group if c['table'] else None, n_prog, G)
        assert np.array_equal(d_r.cpu().numpy(), resid), ('residual against numpy', k)
        got = d_stems.cpu().numpy()
        assert np.array_equal(got, stems), ('stems against numpy', k)
        assert np.array_equal(d_nm.cpu().numpy(), resid[:, :, :F].max(axis=(1, 2))), ('new_max', k)
        changed = {(int(g), int(r)) for g, r in zip(*np.nonzero((got != before).any(axis=2)))}
        assert changed == set(wrote) and len(wrote) == len(set(wrote)), ('rows written', k)
        if k < 4:
            assert np.all(got[:, sentinel] == -7.0), ('sentinels', k)
        else:                                                      # the two sentinel rows slot 5 claims, no others
            rows = {r for _, r in wrote}
            assert rows == set(range(fbase[5] + 12, pool)) and np.all(got[:, sentinel][:, :-gap] == -7.0)
        if k == 0:
            groups = sorted({g for g, _ in wrote})
            assert groups == [0, 1, 2]                             # (program 2 -> table 7 -> stem 2; 3 -> -3 -> stem 0)
            # slot 0 has no guess frames, slot 2 stops at its t_song (song frames 6 .. 9 of window rows 4 .. 10)
            assert not any(fbase[0] <= r < fbase[0] + t_song[0] for _, r in wrote)
            assert sorted(r - fbase[2] for _, r in wrote if fbase[2] <= r < fbase[3] - gap) == [6, 7, 8, 9]
            assert sum(1 for _, r in wrote if fbase[3] <= r < fbase[3] + t_song[3]) == 5      # slot 3's own rows only
        if k in (2, 3):
            assert {g for g, _ in wrote} == {0}
    assert not np.array_equal(resid, np.zeros_like(resid))


# ---- 2. the live walk: the identity ----------------------------------------------------------------------------------------
def _covered(ev_song, t, tf, prog_group, G):
    """[G, t] bool: the song frames the DETECT records of each group reach (from the onset to the window's end)."""
    cov = np.zeros((G, t), bool)
    for e in ev_song[ev_song[:, 2] == so.DETECT]:
        cov[sso.stem_of(e[4], prog_group, G), min(int(e[6]), t):min(int(e[8]) + tf, t)] = True
    return cov


def test_walk_identity_residual_plus_stems(env, grouped2048):
    """run_songs(residual=True, stems=True) with every head and three groups on four short songs: for every bin of every
    frame, the fresh STFT magnitude = residual + sum of stems within (2 max_notes + 2) 2^-24 of it; each stem is zero
    outside its group's DETECT records and nowhere negative; phases bit-identical to the fresh STFT; residual wave + sum
    of stem waves against amt_istft of the fresh STFT to 1e-4 of the song's maximum.  Events with and without stems are
    identical, and without stems no stem buffer exists."""
    torch = env['torch']
    p, lp = grouped2048
    max_notes = 2
    songs = so.make_songs(p, 41, (2.3, 3.0, 0.6, 4.4))
    events, st = lp.run_songs(songs, max_notes=max_notes, silence=1e-4, poll=4, residual=True, stems=True)
    torch.cuda.synchronize()
    ev = events.cpu().numpy()
    B, G, tf = len(songs), 3, p.timing_frames
    assert st.finished.cpu().tolist() == [1] * B and len(st.stem_audio) == B
    assert tuple(st.stems.shape) == (G, st.pool.frames, st.s_mag.shape[1]) and st.stems.dtype == torch.float32
    table = lp.prog_group.cpu().numpy()
    det = ev[ev[:, :, 2] == so.DETECT]
    per_group = np.bincount([sso.stem_of(e[4], table, G) for e in det], minlength=G)
    print('walk: %d notes, per group %s%s' % (len(det), per_group.tolist(),
                                              '' if (per_group > 0).sum() > 1 else ' -- the seeded heads put every '
                                              'note into ONE group: the identity below is checked on that stem alone'))
    assert len(det) > 0
    worst = 0.0
    for i, wave in enumerate(songs):
        fresh = _stft(env, p, wave)
        t, f0 = fresh.T, st.region[i]
        full = fresh.mag[0].cpu().numpy().astype(np.float64)
        res = st.s_mag[f0:f0 + t].cpu().numpy()
        stems = st.stems[:, f0:f0 + t].cpu().numpy()
        assert np.all(stems >= 0) and np.all(res >= 0)
        gap = np.abs(full - (res.astype(np.float64) + stems.astype(np.float64).sum(axis=0)))
        bound = identity_bound(full, max_notes)
        ratio = float((gap / np.maximum(bound, 1e-300)).max())
        print('song %d: %d frames, identity gap at most %.3f of the bound (largest gap %.3e)' % (i, t, ratio, gap.max()))
        assert np.all(gap <= bound), ('identity', i, ratio)
        cov = _covered(ev[:, i, :], t, tf, table, G)
        for g in range(G):
            assert not stems[g][~cov[g]].any(), ('stem %d outside its records' % g, i)
            assert (per_group[g] == 0) <= (not stems[g].any())
        assert torch.equal(st.s_ph[f0:f0 + t], fresh.ph[0]), ('phases', i)
        y = st.stem_audio[i]
        assert y.dtype == torch.float32 and tuple(y.shape) == (G, p.H * (t - 1))
        whole = _istft_one(env, fresh.plan, fresh.mag, fresh.ph, t, p.H, fresh.ldf).cpu().numpy().astype(np.float64)
        parts = st.residual[i].cpu().numpy().astype(np.float64) + y.cpu().numpy().astype(np.float64).sum(axis=0)
        werr = np.abs(parts - whole).max() / np.abs(whole).max()
        worst = max(worst, werr)
        print('song %d: residual wave + stem waves against the song\'s own iSTFT %.2e of the maximum' % (i, werr))
        assert werr < REL, ('waveforms', i, werr)
    assert bool((st.stems[:, st.region[0]:st.region[0] + 1 + len(songs[0]) // p.H] > 0).any())
    # opt-in: events unchanged, and nothing allocated without it
    ev0, st0 = lp.run_songs(songs, max_notes=max_notes, silence=1e-4, poll=4)
    ev1, st1 = lp.run_songs(songs, max_notes=max_notes, silence=1e-4, poll=4, stems=True)
    assert torch.equal(ev0, events) and torch.equal(ev1, events)
    assert st0.stems is None and st0.stem_audio is None and not st0.keep_stems
    assert st1.keep_stems and not st1.keep_residual and st1.residual is None
    assert torch.equal(st1.stems, st.stems)                        # independent of keep_residual
    assert torch.equal(st0.batch.mag, st.batch.mag) and torch.equal(st0.batch.ref_max, st.batch.ref_max)
    for i in range(B):
        assert torch.equal(st1.stem_audio[i], st.stem_audio[i])
    with pytest.raises(ValueError, match='keep_stems'):
        st0.stem_waves([0])
    with pytest.raises(ValueError, match='keep_stems'):
        lp.walk_songs(lp.prepare_songs(songs[:1]), stems=True)
    # only the span subtraction keeps stems
    lp.span_subtract = False
    try:
        with pytest.raises(ValueError, match='AMT_SUBTRACT_SPAN'):
            lp.run_songs(songs[:1], stems=True)
    finally:
        lp.span_subtract = True
    b = st.batch
    b._fmax = None                                                 # no per-frame maxima: no silent whole-window fall-back
    with pytest.raises(RuntimeError, match='per-frame maxima'):
        b.subtract(lp.bank_mag, lp.bank_max, torch.zeros(B, dtype=torch.int32, device='cuda'), 0,
                   torch.zeros(B, dtype=torch.int32, device='cuda'), span=True, stems=env['_lib'].StemArgs())


# ---- 3. the live walk against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['bank2048', 'plain_slides'])
def test_walk_stems_vs_cpu_restatement(env, case):
    """run_songs(stems=True) on the screened seeds of song_oracle.WALK_CASES (no instrument head: one stem): each
    song's region of stem 0 against the stems assembled from the restatement's windows, to 1e-4 of the song's
    spectrogram maximum, the bar test_gpu_song_residual applies to the residual."""
    nfft, wsec, guess, seed, lengths, max_notes, silence, silent, shift = so.WALK_CASES[case]
    torch = env['torch']
    p, lp = _make_loop(env, nfft, wsec, guess, shift)
    songs = so.make_songs(p, seed, lengths, silent)
    events, st = lp.run_songs(songs, max_notes=max_notes, silence=silence, poll=4, song0=3, stems=True)
    torch.cuda.synchronize()
    ev = events.cpu().numpy()
    B = len(songs)
    assert st.finished.cpu().tolist() == [1] * B and tuple(st.stems.shape)[0] == 1
    bank = osynth.guess_bank_waves((0,), p.pitch_low, p.pitch_high, sr=p.sr)
    orc = so.SongOracle(p, so.HEADS, {k: n.weights for k, n in lp.nets.items()}, bank_waves=bank)
    bands = bands_for(p)
    refs = {k: v.cpu().numpy() for k, v in st.refs.items()}
    F, half = p.N // 2 + 1, p.timing_frames // 2
    removed = 0
    for i, wave in enumerate(songs):
        t = 1 + len(wave) // p.H
        f0 = st.region[i]
        wins = []
        ev_ref, _ = orc.run_song(wave, {k: float(v[i]) for k, v in refs.items()}, max_notes, silence, song_id=3 + i,
                                 force=(ev[:, i, :], bands), windows=wins)
        assert np.array_equal(ev[:, i, :], so.pad_finished(ev_ref, ev.shape[0], 3 + i, half)), ('events', i)
        song = oa.AudioCompleteOracle(np.asarray(wave, np.float32), p.N, p.H)
        want, _ = sso.assemble_stems(song, ev_ref, wins, p.timing_frames, None, 1)
        got = st.stems[0, f0:f0 + t].cpu().numpy()
        scale = float(np.asarray(song.mag, np.float32).max())
        err = np.abs(got[:, :F].T - want[0]).max() / scale
        print('%s song %d: %d frames, stem 0 product-oracle %.2e of the maximum' % (case, i, t, err))
        assert err < 1e-4, ('stem 0', i, err)
        assert np.all(got[:, F:] == 0)
        removed += int(want[0].any())
    if not shift:
        assert removed > 0                                         # the case detects: something was taken out


# ---- 4. the queue -----------------------------------------------------------------------------------------------------------
def test_queue_stems_equal_run_songs(env, grouped2048):
    """Five songs of different lengths through 2 slots and a pool small enough that regions are handed out again: every
    yielded stem tensor is run_songs([song], stems=True)'s, bit for bit (a region whose stems were not zeroed at the
    admission would still hold the earlier song's), and so are the records; the optional items come in the order
    residual, stems; a cut walk has None for its unfinished song."""
    torch = env['torch']
    p, lp = grouped2048
    songs = so.make_songs(p, 29, (3.1, 1.4, 4.0, 0.7, 2.6))
    frames = [1 + len(s) // p.H for s in songs]
    pool = 2 * max(frames) + 40
    assert pool < sum(sorted(frames)[-3:])
    alone = []
    for s in songs:
        ev, st = lp.run_songs([s], max_notes=2, silence=1e-4, poll=16, residual=True, stems=True)
        e = ev.cpu().numpy()[:, 0, :]
        alone.append((e[e[:, 2] != so.FINISHED], st.stem_audio[0].clone(), st.residual[0].clone()))
    assert any(bool((a[1] != 0).any()) for a in alone)
    regions, got = [], {}
    for idx, evs, stems in lp.iter_song_queue(iter(songs), 2, max_notes=2, silence=1e-4, poll=4, pool_frames=pool,
                                              on_finish=lambda i, slot, st: regions.append(st.region[slot]), stems=True):
        got[idx] = (evs, stems.clone())
    assert sorted(got) == list(range(5)) and len(set(regions)) < 5          # a region was used twice
    for i, (e, stems, _) in enumerate(alone):
        assert np.array_equal(got[i][0][:, 2:], e[:, 2:]), i
        assert tuple(stems.shape) == (3, p.H * (frames[i] - 1))
        assert torch.equal(got[i][1], stems), ('stems of song %d' % i)
    both = lp.run_song_queue(iter(songs), 2, max_notes=2, silence=1e-4, poll=4, pool_frames=pool, residual=True, stems=True)
    assert len(both) == 5 and all(len(item) == 3 for item in both)
    for i, (e, res, stems) in enumerate(both):
        assert torch.equal(res, alone[i][2]) and torch.equal(stems, alone[i][1]), i
    plain = lp.run_song_queue(iter(songs), 2, max_notes=2, silence=1e-4, poll=4, pool_frames=pool)
    assert all(np.array_equal(a, b[0]) for a, b in zip(plain, both))
    st = lp.prepare_songs([songs[3], songs[2]], keep_stems=True)
    lp.walk_songs(st, max_notes=2, silence=1e9, poll=1, max_steps=2, stems=True)
    assert st.finished.cpu().tolist() == [1, 0]
    assert st.stem_audio[1] is None and not bool(st.stem_audio[0].any())    # nothing detected: silence
    with pytest.raises(ValueError, match='not finished'):
        st.stem_waves([0, 1])
    with pytest.raises(ValueError):
        st.stem_waves([2])


# ---- 5. transcribe and the command line ----------------------------------------------------------------------------------
def test_transcribe_stems_and_command_line(env, tmp_path):
    """transcribe(traversal='song', stems=True) appends the stems [G, samples] to what it returns (after the residual);
    the command line writes them through flac.save_float, <input stem>.group<g>.flac per reference group id: each file
    decodes with CRC and MD5 verified, holds hop * (T - 1) samples at the model's rate and equals the returned stem after
    the writer's 24-bit quantisation.  --songs --stems-dir writes G files per song."""
    from amt_saga import flac, transcribe as tr
    p = env['hp'].Hyperparams(N=2048, sr=44100)                   # the command line's model: 516-frame windows
    n = int(1.3 * p.H * (p.timing_frames - 1))
    notes_in = [(0, 60, 100, 0.2, 0.5), (0, 64, 90, 0.9, 0.4), (1, 67, 80, 2.6, 0.6), (2, 72, 110, 5.4, 0.3)]
    wf = osynth.render_window(notes_in, n, p.sr).numpy()
    src = str(tmp_path / 'clip.flac')
    flac.save_float(wf, src, p.sr)
    wf24 = flac.load_float(src)[0]                                 # what the command line reads
    lp = tr._make_loop(p, 1, ALL_HEADS, (0, 1, 2), None, 'bank')   # transcribe()'s own
    notes, evs, res, stems = tr.transcribe(wf24, p, iters=1, traversal='song', residual=True, stems=True, loop=lp)
    only = tr.transcribe(wf24, p, iters=1, traversal='song', stems=True, loop=lp)
    plain = tr.transcribe(wf24, p, iters=1, traversal='song', loop=lp)
    assert len(plain) == 2 and len(only) == 3 and np.array_equal(plain[1], evs) and plain[0] == notes == only[0]
    T = 1 + n // p.H
    assert stems.is_cuda and tuple(stems.shape) == (3, p.H * (T - 1)) and tuple(res.shape) == (p.H * (T - 1),)
    assert env['torch'].equal(only[2], stems)
    with pytest.raises(ValueError, match='stems'):
        tr.transcribe(wf24, p, iters=1, stems=True, loop=lp)
    sdir, out = str(tmp_path / 'stems'), str(tmp_path / 'left.flac')
    tr.main([src, str(tmp_path / 'cli.mid'), '--iters', '1', '--traversal', 'song', '--residual', out, '--stems-dir', sdir])
    assert sorted(os.listdir(sdir)) == ['clip.group0.flac', 'clip.group1.flac', 'clip.group2.flac']
    y = stems.cpu().numpy().astype(np.float64)
    want = np.clip(np.rint(y * 8388608.0), -8388608, 8388607).astype(np.int64)
    assert np.any(want != 0)
    for g in range(3):
        pcm, sr, bps = flac.decode(os.path.join(sdir, 'clip.group%d.flac' % g), verify=True)
        assert (sr, bps) == (p.sr, 24) and pcm.shape == (p.H * (T - 1), 1)
        assert np.array_equal(pcm[:, 0], want[g]), g
    assert flac.decode(out, verify=True)[0].shape == (p.H * (T - 1), 1)
    with pytest.raises(SystemExit, match='--traversal song'):
        tr.main([src, str(tmp_path / 'x.mid'), '--iters', '1', '--stems-dir', str(tmp_path / 'x')])
    other = str(tmp_path / 'other.flac')
    flac.save_float(wf[:n // 2], other, p.sr)
    qdir = str(tmp_path / 'qstems')
    tr.main(['--songs', src, other, '--out-dir', str(tmp_path / 'mid'), '--slots', '2', '--iters', '1', '--stems-dir', qdir])
    assert sorted(os.listdir(qdir)) == ['%s.group%d.flac' % (s, g) for s in ('clip', 'other') for g in range(3)]
    for g in range(3):
        pcm2, sr2, _ = flac.decode(os.path.join(qdir, 'clip.group%d.flac' % g), verify=True)
        assert sr2 == p.sr and np.array_equal(pcm2[:, 0], want[g])  # the queue's stems are run_songs' for the song alone
        pcm3, sr3, _ = flac.decode(os.path.join(qdir, 'other.group%d.flac' % g), verify=True)
        assert sr3 == p.sr and pcm3.shape == (p.H * (n // 2 // p.H), 1)
    assert sorted(os.listdir(str(tmp_path / 'mid'))) == ['clip.mid', 'other.mid']
