"""GPU: the song queue (TranscriptionLoop.run_song_queue / iter_song_queue, amt_stft_mag_ragged, amt_song_admit): the
ragged STFT bit for bit against amt_stft_mag per signal, the admit kernel against numpy, and the queue against run_songs
on every song alone -- integers exact, the residual of the last window bit-identical -- for every slots / poll / pool."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import song_oracle as so                                        # noqa: E402
from oracle import synth as osynth                              # noqa: E402

pytestmark = pytest.mark.gpu


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


def _alone(env, lp, songs, max_notes, silence):
    """run_songs on every song by itself: (live records [k, 9], last window magnitudes, phases) per song."""
    out = []
    for s in songs:
        ev, st = lp.run_songs([s], max_notes=max_notes, silence=silence, poll=16)
        e = ev.cpu().numpy()[:, 0, :]
        out.append((e[e[:, 2] != so.FINISHED], st.batch.mag[0].clone(), st.batch.ph[0].clone()))
    return out


def _queue(lp, songs, slots, poll, max_notes, silence, pool_frames=None):
    last = {}

    def keep(idx, slot, st):
        last[idx] = (st.batch.mag[slot].clone(), st.batch.ph[slot].clone())
    evs = lp.run_song_queue(iter(songs), slots, max_notes=max_notes, silence=silence, poll=poll,
                            pool_frames=pool_frames, on_finish=keep)
    return evs, last


def _same(env, alone, evs, last, tag):
    torch = env['torch']
    assert len(evs) == len(alone) == len(last), tag
    for i, (e, mag, ph) in enumerate(alone):
        q = evs[i]
        assert q.dtype == np.int32 and q.shape == e.shape, (tag, i, q.shape, e.shape)
        assert np.all(q[:, 0] == i) and q[:, 1].tolist() == list(range(len(q))), (tag, i)
        assert np.array_equal(q[:, 2:], e[:, 2:]), (tag, i, q.tolist(), e.tolist())
        assert np.array_equal(e[:, 1], q[:, 1])                     # alone, the walk's steps are the song's own
        assert torch.equal(last[i][0], mag) and torch.equal(last[i][1], ph), (tag, i, 'residual window')


def test_company_does_not_matter(env):
    """The premise of the queue tests (holds without the queue): a song walked alone by run_songs and the same song among
    seven others give the same records and bit-identical last windows -- the networks choose their tiles from the layer
    shape and scale per window, nothing in the step mixes songs."""
    torch = env['torch']
    p, lp = _make_loop(env, 2048, 1, 'bank')
    songs = so.make_songs(p, 41, (3.1, 2.2, 4.0, 1.4, 2.8, 3.6, 0.7, 4.4))
    ev8, st8 = lp.run_songs(songs, max_notes=2, silence=1e-4, poll=1)
    e8 = ev8.cpu().numpy()
    detects = 0
    for i, s in enumerate(songs):
        ev1, st1 = lp.run_songs([s], max_notes=2, silence=1e-4, poll=1)
        e1 = ev1.cpu().numpy()[:, 0, :]
        a, b = e1[e1[:, 2] != so.FINISHED], e8[:, i, :][e8[:, i, 2] != so.FINISHED]
        assert np.array_equal(a[:, 1:], b[:, 1:]), (i, a.tolist(), b.tolist())
        assert torch.equal(st1.batch.mag[0], st8.batch.mag[i]) and torch.equal(st1.batch.ph[0], st8.batch.ph[i]), i
        assert torch.equal(st1.refs['ref_mag'][0], st8.refs['ref_mag'][i])
        detects += int((a[:, 2] == so.DETECT).sum())
    assert detects > 8


@pytest.mark.parametrize('nfft', [2048, 4096])
def test_ragged_stft_bit_identical(env, nfft):
    """amt_stft_mag_ragged against amt_stft_mag on each signal alone: magnitudes, unit phases and maxima bit for bit, with
    and without phases.  Lengths: the shortest the reflect padding allows (n_fft / 2 + 1; a signal of ONE hop = n_fft / 4
    samples is rejected by amt_stft_mag itself, so both entries must refuse it), one hop more, a non-multiple of the
    hop, exactly one window, one frame pair more / less than 16 and than 32 pairs, a long one (> 1300 hops), then 33
    signals of mixed lengths in one launch.  These launches are small -- one frame pair per workgroup; workgroups of
    several pairs are test_ragged_stft_multi_pair_workgroups."""
    torch, lib, _lib, audio = env['torch'], env['lib'], env['_lib'], env['audio']
    hop, ldf = nfft // 4, audio.ldf_of(nfft)
    rng = np.random.default_rng(nfft)
    special = [nfft // 2 + 1, nfft // 2 + hop, 5 * hop + 37, nfft, 30 * hop, 34 * hop + 3, 31 * hop + hop - 1,
               62 * hop, 66 * hop + 1, 1311 * hop + 5]
    mixed = [int(v) for v in rng.integers(nfft // 2 + 1, 90 * hop, 33)]
    plan = audio._plan(nfft, hop, True)
    for lens in ([special[0]], [special[-1]], special, mixed):
        n = len(lens)
        t = [1 + L // hop for L in lens]
        # regions in shuffled order with gaps, as a free list would hand them out
        order = rng.permutation(n)
        fb, sb, f_at, s_at = np.zeros(n, np.int64), np.zeros(n, np.int64), 3, 5
        for i in order:
            fb[i], sb[i] = f_at, s_at
            f_at += t[i] + int(rng.integers(0, 3))
            s_at += lens[i] + int(rng.integers(0, 7))
        pool_frames, n_samples = f_at + 2, s_at + 3
        samples = torch.zeros(n_samples, device='cuda')
        waves = [torch.from_numpy(rng.standard_normal(L).astype(np.float32)).cuda() for L in lens]
        for i, w in enumerate(waves):
            samples[sb[i]:sb[i] + lens[i]] = w
        d_sb, d_fb = torch.from_numpy(sb).cuda(), torch.from_numpy(fb).cuda()
        d_len = torch.from_numpy(np.asarray(lens, np.int32)).cuda()
        for with_phase in (True, False):
            mag = torch.full((pool_frames, ldf), -7.0, device='cuda')
            ph = torch.full((pool_frames, ldf, 2), -7.0, device='cuda') if with_phase else None
            ref = torch.empty(n, device='cuda')
            st = lib.amt_stft_mag_ragged(plan, samples.data_ptr(), d_sb.data_ptr(), d_len.data_ptr(), n, max(lens),
                                         n_samples, sum(lens), mag.data_ptr(), ph.data_ptr() if with_phase else None,
                                         ref.data_ptr(), d_fb.data_ptr(), pool_frames, ldf, None)
            assert st == _lib.AMT_OK
            torch.cuda.synchronize()
            written = torch.zeros(pool_frames, dtype=torch.bool, device='cuda')
            for i, w in enumerate(waves):
                one = audio.AudioBatch(w[None, :], nfft, hop).stft(with_phase=with_phase)
                assert one.T == t[i]
                assert torch.equal(mag[fb[i]:fb[i] + t[i]], one.mag[0]), (lens[i], 'mag', with_phase)
                if with_phase:
                    assert torch.equal(ph[fb[i]:fb[i] + t[i]], one.ph[0]), (lens[i], 'phase')
                assert torch.equal(ref[i], one.ref_max[0]), (lens[i], 'ref_max')
                written[fb[i]:fb[i] + t[i]] = True
            assert bool((mag[~written] == -7.0).all())              # nothing outside the signals' regions
    # one hop: too short for the reflect padding -- refused by both entries, nothing launched
    w = torch.zeros(1, hop, device='cuda')
    with pytest.raises(ValueError, match='Invalid Input shape'):
        audio.AudioBatch(w, nfft, hop).stft()
    z = torch.zeros(1, dtype=torch.int64, device='cuda')
    one = torch.full((1,), hop, dtype=torch.int32, device='cuda')
    out = torch.zeros(4, ldf, device='cuda')
    assert lib.amt_stft_mag_ragged(plan, w.data_ptr(), z.data_ptr(), one.data_ptr(), 1, hop, hop, hop, out.data_ptr(),
                                   None, None, z.data_ptr(), 4, ldf, None) == _lib.AMT_E_SHAPE


@pytest.mark.parametrize('want_ppb', [4, 16])
def test_ragged_stft_multi_pair_workgroups(env, want_ppb):
    """The launches above are small: both launchers give every workgroup ONE frame pair there, so no workgroup carries
    samples from a pair to the next.  Here a magnitude-only launch (N = 2048: the form that keeps ten samples of a pair
    in registers for the next one) is large enough for `want_ppb` pairs per workgroup -- the launchers halve 16 while
    fewer than 16384 workgroups would result; the test restates that rule and asserts the value -- with signals whose
    pair counts sit one below, on and one above a multiple of want_ppb, odd frame counts and lengths off the hop grid.
    Every signal bit for bit against amt_stft_mag on the signal alone (one pair per workgroup, nothing carried); the
    boundary signals also against amt_stft_mag on a batch large enough that it, too, runs want_ppb pairs per workgroup
    and carries.  The carry must end at a signal's own end: neighbours are packed without a gap."""
    torch, lib, _lib, audio = env['torch'], env['lib'], env['_lib'], env['audio']
    nfft, hop = 2048, 512
    ldf = audio.ldf_of(nfft)

    def ppb_of(pairs_all):
        ppb = 16
        while ppb > 1 and (pairs_all + ppb - 1) // ppb < 16384:
            ppb >>= 1
        return ppb
    rng = np.random.default_rng(want_ppb)
    base_pairs = 16384 * want_ppb // 32                             # 33 signals of about this many pairs each
    pairs = [base_pairs + d for d in (-1, 0, 1, want_ppb - 1, want_ppb, want_ppb + 1)] + \
        [int(v) for v in rng.integers(base_pairs - 40, base_pairs + 40, 27)]
    # pairs = (T + 1) // 2: T = 2 pairs (even) or 2 pairs - 1 (odd: the last pair has one frame)
    t = [2 * q - (i % 2) for i, q in enumerate(pairs)]
    lens = [hop * (T - 1) + int(rng.integers(0, hop)) for T in t]
    n = len(lens)
    assert [1 + L // hop for L in lens] == t and n == 33
    assert ppb_of((sum(lens) // hop + 2 * n + 1) // 2) == want_ppb
    assert {q % want_ppb for q in pairs[:6]} >= {want_ppb - 1, 0, 1}
    fb = np.concatenate(([0], np.cumsum(t)))
    sb = np.concatenate(([0], np.cumsum(lens)))
    samples = torch.randn(int(sb[-1]), device='cuda', generator=torch.Generator('cuda').manual_seed(want_ppb))
    pool_frames = int(fb[-1])
    mag = torch.full((pool_frames, ldf), -7.0, device='cuda')
    ref = torch.empty(n, device='cuda')
    d_sb, d_fb = torch.from_numpy(sb[:-1].astype(np.int64)).cuda(), torch.from_numpy(fb[:-1].astype(np.int64)).cuda()
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    plan = audio._plan(nfft, hop, True)
    assert lib.amt_stft_mag_ragged(plan, samples.data_ptr(), d_sb.data_ptr(), d_len.data_ptr(), n, max(lens),
                                   samples.numel(), sum(lens), mag.data_ptr(), None, ref.data_ptr(), d_fb.data_ptr(),
                                   pool_frames, ldf, None) == _lib.AMT_OK
    torch.cuda.synchronize()
    assert not bool((mag == -7.0).any())                            # the regions tile the pool: everything written
    for i in range(n):
        w = samples[sb[i]:sb[i + 1]]
        one = audio.AudioBatch(w[None, :], nfft, hop).stft(with_phase=False)
        assert ppb_of((t[i] + 1) // 2) == 1
        assert torch.equal(mag[fb[i]:fb[i + 1]], one.mag[0]), (i, lens[i], 'alone')
        assert torch.equal(ref[i], one.ref_max[0]), (i, 'ref_max')
        del one
    for i in range(6):                                              # the boundary signals against a batch that carries
        rows = -(-16384 * want_ppb // ((t[i] + 1) // 2))
        assert ppb_of(((t[i] + 1) // 2) * rows) >= want_ppb         # launch_stft: (pairs / ppb) x B workgroups
        batch = samples[sb[i]:sb[i + 1]][None, :].repeat(rows, 1)
        many = audio.AudioBatch(batch, nfft, hop).stft(with_phase=False)
        assert torch.equal(mag[fb[i]:fb[i + 1]], many.mag[0]) and torch.equal(mag[fb[i]:fb[i + 1]], many.mag[rows - 1]), i
        assert torch.equal(ref[i], many.ref_max[0])
        del many, batch


def test_admit_kernel_vs_numpy(env):
    """amt_song_admit on a random pool: admitted slots hold S[0:T) with zero rows past short songs, state reset, tables
    replaced; every other slot -- window, state, tables -- byte-identical to before."""
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    rng = np.random.default_rng(9)
    B, T, ldf, K, S = 11, 86, 1028, 5, 2
    t_new = [30, 86, 200, 1, 85, 87]                                # shorter than a window, exact, longer, one frame
    slots = [9, 0, 4, 10, 2, 6]                                     # admission order != slot order
    n = len(t_new)
    pool_frames = sum(t_new) + 40
    fb_new = np.zeros(n, np.int64)
    at = 7
    for j in rng.permutation(n):
        fb_new[j] = at
        at += t_new[j] + 3
    s_mag = rng.standard_normal((pool_frames, ldf)).astype(np.float32)
    s_ph = rng.standard_normal((pool_frames, ldf, 2)).astype(np.float32)
    host = dict(w_mag=rng.standard_normal((B, T, ldf)).astype(np.float32),
                w_ph=rng.standard_normal((B, T, ldf, 2)).astype(np.float32),
                frame_base=rng.integers(0, 99, B).astype(np.int64), t_song=rng.integers(1, 99, B).astype(np.int32),
                sample_base=rng.integers(0, 99, B).astype(np.int64), slot_song=rng.integers(0, 99, B).astype(np.int32),
                seg=rng.integers(0, 99, (B, K, S, 3)).astype(np.int32), offset=rng.integers(0, 99, B).astype(np.int32),
                count=rng.integers(0, 5, B).astype(np.int32), finished=rng.integers(0, 2, B).astype(np.int32),
                clean=rng.integers(0, 2, B).astype(np.int32))
    for k in range(4):
        host['ref%d' % k] = rng.random(B).astype(np.float32)
    new = dict(new_t_song=np.asarray(t_new, np.int32), new_frame_base=fb_new,
               new_sample_base=rng.integers(100, 999, n).astype(np.int64), new_song=np.arange(50, 50 + n).astype(np.int32),
               new_seg=rng.integers(100, 999, (n, K, S, 3)).astype(np.int32))
    for k in range(4):
        new['new_ref%d' % k] = (rng.random(n) + 2).astype(np.float32)
    admit = np.zeros(B, np.int32)
    for j, b in enumerate(slots):
        admit[b] = 1 + j
    d = {k: torch.from_numpy(v).cuda() for k, v in list(host.items()) + list(new.items())}
    d.update(s_mag=torch.from_numpy(s_mag).cuda(), s_ph=torch.from_numpy(s_ph).cuda(), admit=torch.from_numpy(admit).cuda())
    names = ('w_mag', 'w_ph', 's_mag', 's_ph', 'admit', 'new_frame_base', 'new_t_song', 'new_sample_base', 'new_song',
             'new_seg', 'frame_base', 't_song', 'sample_base', 'slot_song', 'seg', 'offset', 'count', 'finished', 'clean')
    a = _lib.song_admit_args(w_stride=T * ldf, B=B, n_new=n, T=T, ldf=ldf, K=K, S=S,
                             new_ref=[d['new_ref%d' % k] for k in range(3)],       # the fourth constant is unused
                             ref=[d['ref%d' % k] for k in range(3)],               # (NULL): left alone
                             **{f: d[f] for f in names})
    with pytest.raises(ValueError):
        _lib.song_admit_args(nope=1)
    a.ldf = ldf + 1
    assert lib.amt_song_admit(ctypes.byref(a), None) == _lib.AMT_E_SHAPE      # rows must be whole float4
    a.ldf = ldf
    assert lib.amt_song_admit(None, None) == _lib.AMT_E_INVALID
    assert lib.amt_song_admit(ctypes.byref(a), None) == _lib.AMT_OK
    torch.cuda.synchronize()
    got = {k: d[k].cpu().numpy() for k in host}
    for b in range(B):
        if admit[b] == 0:
            for k in host:
                assert np.array_equal(got[k][b], host[k][b]), (b, k)
            continue
        j = admit[b] - 1
        rows = min(T, t_new[j])
        for name, s in (('w_mag', s_mag), ('w_ph', s_ph)):
            want = np.zeros_like(host[name][b])
            want[:rows] = s[fb_new[j]:fb_new[j] + rows]
            assert np.array_equal(got[name][b], want), (b, name)
        assert got['frame_base'][b] == fb_new[j] and got['t_song'][b] == t_new[j]
        assert got['sample_base'][b] == new['new_sample_base'][j] and got['slot_song'][b] == 50 + j
        assert np.array_equal(got['seg'][b], new['new_seg'][j])
        for k in range(3):
            assert got['ref%d' % k][b] == new['new_ref%d' % k][j]
        assert got['ref3'][b] == host['ref3'][b]
        assert (got['offset'][b], got['count'][b], got['finished'][b], got['clean'][b]) == (0, 0, 0, 1)
    # the event packer with per-slot song indices
    i32 = lambda v: torch.from_numpy(np.asarray(v, np.int32)).cuda()
    kind, pit, on, en, off = i32([0, 1, 3, 2]), i32([60, 61, 62, 63]), i32([5, 50, 7, 9]), i32([9, 60, 8, 20]), i32([43, 0, 86, 129])
    song, ev = i32([7, 3, -1, 12]), torch.zeros(4, 9, dtype=torch.int32, device='cuda')
    assert lib.amt_song_pack_events_slots(4, song.data_ptr(), 21, kind.data_ptr(), pit.data_ptr(), None, None,
                                          on.data_ptr(), en.data_ptr(), off.data_ptr(), ev.data_ptr(), None) == _lib.AMT_OK
    assert ev.cpu().tolist() == [[7, 21, 0, 60, -1, -1, 48, 52, 43], [3, 21, 1, -1, -1, -1, 50, 60, 0],
                                 [-1, 21, 3, -1, -1, -1, -1, -1, 86], [12, 21, 2, -1, -1, -1, 138, 149, 129]]
    # ... and with song0 + slot: one kernel behind both entries, so song0 = 7 and slot_song = 7 .. 10 write the same
    ev0, ev1 = (torch.full((4, 9), -5, dtype=torch.int32, device='cuda') for _ in range(2))
    assert lib.amt_song_pack_events(4, 7, 21, kind.data_ptr(), pit.data_ptr(), None, None, on.data_ptr(), en.data_ptr(),
                                    off.data_ptr(), ev0.data_ptr(), None) == _lib.AMT_OK
    assert lib.amt_song_pack_events_slots(4, i32([7, 8, 9, 10]).data_ptr(), 21, kind.data_ptr(), pit.data_ptr(), None,
                                          None, on.data_ptr(), en.data_ptr(), off.data_ptr(), ev1.data_ptr(),
                                          None) == _lib.AMT_OK
    assert torch.equal(ev0, ev1)
    assert ev0.cpu().tolist() == [[7, 21, 0, 60, -1, -1, 48, 52, 43], [8, 21, 1, -1, -1, -1, 50, 60, 0],
                                  [9, 21, 3, -1, -1, -1, -1, -1, 86], [10, 21, 2, -1, -1, -1, 138, 149, 129]]


@pytest.mark.parametrize('case', list(so.WALK_CASES))
def test_queue_vs_run_songs_walk_cases(env, case):
    """The screened seeds of song_oracle.WALK_CASES: every song's records from the queue equal run_songs([song]) for the
    song alone, the residual of its last window bit for bit, for slots 2, 4, 8 and poll 1, 16."""
    nfft, wsec, guess, seed, lengths, max_notes, silence, silent, shift = so.WALK_CASES[case]
    p, lp = _make_loop(env, nfft, wsec, guess, shift)
    songs = so.make_songs(p, seed, lengths, silent)
    alone = _alone(env, lp, songs, max_notes, silence)
    assert sum(int((e[:, 2] == so.DETECT).sum()) for e, _, _ in alone) > 0 or shift
    for slots in (2, 4, 8):
        for poll in (1, 16):
            evs, last = _queue(lp, songs, slots, poll, max_notes, silence)
            _same(env, alone, evs, last, (case, slots, poll))
            assert lp.queue_stats['songs'] == len(songs)


@pytest.mark.parametrize('guess', ['bank', 'render'])
def test_queue_of_many_songs_vs_run_songs(env, guess):
    """24 songs of mixed lengths (0.4 ... 6 half windows) through 2, 4 and 8 slots, poll 1 and 16: the records do not
    depend on slots or poll and equal run_songs on each song alone; then a pool sized for two songs under eight slots
    (songs wait for a region): same records, the walk ends."""
    p, lp = _make_loop(env, 2048, 1, guess)
    rng = np.random.default_rng(77)
    hw = [float(v) for v in np.round(rng.uniform(0.4, 6.0, 24), 2)]
    songs = so.make_songs(p, 51, hw)
    alone = _alone(env, lp, songs, 2, 1e-4)
    assert len({len(e) for e, _, _ in alone}) >= 6
    for slots in (2, 4, 8):
        for poll in (1, 16):
            evs, last = _queue(lp, songs, slots, poll, 2, 1e-4)
            _same(env, alone, evs, last, (guess, slots, poll))
            st = lp.queue_stats
            assert st['songs'] == 24 and st['admissions'] > 1 and sum(st['slot_steps']) == st['steps'] * slots
    longest = max(1 + len(s) // p.H for s in songs)
    evs, last = _queue(lp, songs, 8, 4, 2, 1e-4, pool_frames=2 * longest)
    _same(env, alone, evs, last, (guess, 'small pool'))
    assert lp.queue_stats['waits'] > 0
    with pytest.raises(ValueError, match='longer than the pool'):
        lp.run_song_queue(songs, 4, max_notes=2, pool_frames=longest - 1)
    # the generator form yields each song as it finishes: short songs overtake long ones
    order = [i for i, _ in lp.iter_song_queue(songs, 4, max_notes=2, silence=1e-4, poll=4)]
    assert sorted(order) == list(range(24)) and order != sorted(order)


def test_transcribe_songs_and_cli(env, tmp_path):
    """transcribe_songs on three synthetic songs equals three transcribe(traversal='song') calls; the many-files mode
    of the command line writes three parseable MIDI files; the one-file invocation is untouched."""
    from amt_saga import events, flac, transcribe as tr
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    L = p.H * (p.timing_frames - 1)
    heads = ('timing', 'pitch', 'instrument', 'velocity')
    wfs = []
    for k, frac in enumerate((3.2, 1.4, 2.1)):
        n = int(frac * L)
        notes_in = [(k % 3, 60 + 2 * j + k, 100, 0.2 + 0.7 * j, 0.4) for j in range(int(n / p.sr / 0.7))]
        wfs.append(osynth.render_window(notes_in, n, p.sr).numpy())
    got = tr.transcribe_songs(wfs, p, slots=2, iters=2, heads=heads)
    assert len(got) == 3
    for i, wf in enumerate(wfs):
        notes, evs = tr.transcribe(wf, p, iters=2, heads=heads, traversal='song')
        live = evs[evs[:, 0, 2] != so.FINISHED, 0, :]
        q_notes, q_evs = got[i]
        assert np.array_equal(q_evs[:, 1:], live[:, 1:]) and np.all(q_evs[:, 0] == i)
        assert [dict(n, song=0) for n in q_notes] == notes and all(n['song'] == i for n in q_notes)
    assert sum(len(n) for n, _ in got) > 0
    paths = []
    for i, wf in enumerate(wfs):
        paths.append(str(tmp_path / ('clip%d.flac' % i)))
        flac.save_float(wf, paths[-1], p.sr)
    out_dir = str(tmp_path / 'mid')
    tr.main(['--songs'] + paths + ['--out-dir', out_dir, '--slots', '2', '--iters', '2'])
    for i in range(3):
        rd = events.read_midi(os.path.join(out_dir, 'clip%d.mid' % i))
        cli_p = env['hp'].Hyperparams(N=2048, sr=p.sr)              # the command line's own parameters: 6-s windows
        cli_notes, _ = tr.transcribe(flac.load_float(paths[i])[0], cli_p, iters=2, traversal='song')
        assert len(rd) == len(cli_notes)
    other = str(tmp_path / 'rate.flac')
    flac.save_float(wfs[1], other, 22050)
    with pytest.raises(SystemExit, match='sample rate'):
        tr.main(['--songs', paths[0], other, '--out-dir', out_dir])
    tr.main([paths[1], str(tmp_path / 'one.mid'), '--iters', '1', '--traversal', 'song'])
    assert os.path.getsize(str(tmp_path / 'one.mid')) > 20


def test_every_optional_output_at_once_keeps_the_documented_order(env):
    """transcribe(traversal='song') asked for residual, stems, percussive and beats together returns six items in the
    documented order, each the item of the run that asks for it alone; transcribe_songs with the same flags returns the
    same six for song 0 (notes up to `song`)."""
    torch = env['torch']
    from amt_saga import transcribe as tr
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    lp = tr._make_loop(p, 1, ('timing', 'pitch', 'instrument', 'velocity'), (0, 1, 2), None, 'bank')
    n = int(2.4 * p.H * (p.timing_frames - 1))
    notes_in = [(j % 3, 60 + 2 * j, 100, 0.2 + 0.7 * j, 0.4) for j in range(int(n / p.sr / 0.7))]
    wf = osynth.render_window(notes_in, n, p.sr).numpy().astype(np.float32)
    rng = np.random.default_rng(6)
    for s in range(3000, n - 64, 11000):                            # drum-like bursts: a percussive part that is not 0
        wf[s:s + 64] += (0.5 * (2 * rng.random(64) - 1)).astype(np.float32)

    def run(**kw):
        return tr.transcribe(wf, p, iters=1, loop=lp, traversal='song', hpss=True, **kw)
    everything = dict(residual=True, stems=True, percussive=True, beats=True)
    got = run(**everything)
    assert len(got) == 6
    notes, evs, residual, stems, percussive, beats = got
    assert residual.ndim == 1 and stems.ndim == 2 and stems.shape[0] == 3 and percussive.ndim == 1
    assert float(percussive.abs().max()) > 0 and set(beats) == {'period', 'tempo', 'beats', 'frames'}
    for k, flag in enumerate(('residual', 'stems', 'percussive', 'beats')):
        alone = run(**{flag: True})
        assert len(alone) == 3 and alone[0] == notes and np.array_equal(alone[1], evs), flag
        if flag == 'beats':
            assert alone[2] == got[2 + k]
        else:
            assert alone[2].shape == got[2 + k].shape and torch.equal(alone[2], got[2 + k]), flag
    plain = run()
    assert len(plain) == 2 and plain[0] == notes and np.array_equal(plain[1], evs)
    queue = tr.transcribe_songs([wf, wf[:n // 2]], p, slots=2, iters=1, loop=lp, hpss=True, **everything)
    assert [len(q) for q in queue] == [6, 6]
    q_notes, q_evs, q_residual, q_stems, q_percussive, q_beats = queue[0]
    assert [dict(nt, song=0) for nt in q_notes] == notes and all(nt['song'] == 0 for nt in q_notes)
    live = evs[evs[:, 0, 2] != so.FINISHED, 0, :]
    assert np.array_equal(q_evs[:, 1:], live[:, 1:]) and np.all(q_evs[:, 0] == 0)
    assert torch.equal(q_residual, residual) and torch.equal(q_stems, stems) and torch.equal(q_percussive, percussive)
    assert q_beats == beats
    assert all(nt['song'] == 1 for nt in queue[1][0]) and queue[1][2].shape[0] < residual.shape[0]


def test_song_queue_argument_checks(env):
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    lp = env['loop'].TranscriptionLoop(p, heads=('timing', 'pitch')).setup_device()
    song = np.zeros(p.H * 50, np.float32)
    with pytest.raises(ValueError, match='slots must be at least 1'):
        lp.run_song_queue([song], 0)
    with pytest.raises(ValueError, match='run_songs: no songs given'):
        lp.run_song_queue([], 4)
    with pytest.raises(ValueError, match='run_songs: no songs given'):
        lp.iter_song_queue(iter(()), 4)                             # raised at the call, not at the first next()
    with pytest.raises(ValueError, match='Invalid Input shape. Expected: a song of at least one hop'):
        lp.run_song_queue([song, song[:p.H - 1]], 4)
    with pytest.raises(ValueError, match='Invalid Input shape'):
        lp.run_song_queue([song, song[:p.H]], 1)                    # met later in the queue: raised when it is pulled
    with pytest.raises(ValueError, match='run_songs: max_notes must be at least 1'):
        lp.run_song_queue([song], 2, max_notes=0)
    odd = env['loop'].TranscriptionLoop(env['hp'].Hyperparams(N=4096, window_size_note_time=1), heads=('timing',))
    with pytest.raises(ValueError, match='Invalid Input shape. run_songs needs an even timing_frames'):
        odd.run_song_queue([song], 2)                              # 43 frames: checked before any device set-up
    with pytest.raises(ValueError, match='run_songs: the walk needs the timing heads'):
        env['loop'].TranscriptionLoop(p, heads=('pitch',)).setup_device().run_song_queue([song], 2)
    evs = lp.run_song_queue([song], 3, max_notes=1)                 # a silent song: forced slides only, the walk ends
    assert len(evs) == 1 and set(evs[0][:, 2].tolist()) <= {so.SLIDE, so.FORCED_SLIDE}


SYNTHETIC = ('timing', 'pitch', 'velocity')


def test_fixed_batch_is_one_admission(env):
    """prepare_songs is a state of one slot per song and one admission of song i into slot i: for a song shorter than
    the first window (zero rows after its end), one of exactly hop x (timing_frames - 1) samples and one of 2.3 windows
    off the hop grid, its state and a queue's state after the first admission (3 slots, the queue's default pool) hold
    bit-identical windows, equal integers and normalisers and the same raw samples for the CQT heads; the queue's own
    state, seen in on_finish, has the same song lengths and normalisers.  Then run_songs against run_song_queue: equal
    live records, and run_songs' song column is song0 + slot in every row, FINISHED ones included."""
    torch, lib, _lib, loop = env['torch'], env['lib'], env['_lib'], env['loop']
    p, lp = _make_loop(env, 2048, 1, 'bank', heads=SYNTHETIC)
    tf, half = p.timing_frames, p.timing_frames // 2
    L = p.H * (tf - 1)
    n = [int(0.7 * L), L, int(2.3 * L)]
    assert 1 + n[0] // p.H < tf and n[2] % p.H and (tf, half) == (86, 43)
    songs = [s[:k].copy() for s, k in zip(so.make_songs(p, 61, (1.5, 2.1, 4.7)), n)]
    assert [len(s) for s in songs] == n
    fixed = lp.prepare_songs(songs)
    queue = loop.SongState(lp, 3, 3 * max(1 + k // p.H for k in n))
    assert len(queue.admit([(i, i, torch.from_numpy(s).cuda()) for i, s in enumerate(songs)])) == 3
    assert torch.equal(fixed.batch.mag, queue.batch.mag) and torch.equal(fixed.batch.ph, queue.batch.ph)
    assert bool((fixed.batch.mag[0, 1 + n[0] // p.H:] == 0).all()) and bool((fixed.batch.mag[0, n[0] // p.H] != 0).any())
    for name in ('t_song', 'offset', 'count', 'finished', 'clean', 'slot_song'):
        assert torch.equal(getattr(fixed, name), getattr(queue, name)), name
    assert fixed.t_song.tolist() == [1 + k // p.H for k in n] and fixed.finished.tolist() == [0, 0, 0]
    assert set(fixed.refs) == set(queue.refs) == {'ref_mag', 'ref_C_1', 'ref_C_foc'}
    for k in fixed.refs:
        assert torch.equal(fixed.refs[k], queue.refs[k]), k
    assert fixed.l_row == queue.l_row
    rows = []
    for st in (fixed, queue):
        out = torch.zeros((3, st.l_row), device='cuda')
        assert lib.amt_song_wave(st.samples.data_ptr(), st.sample_base.data_ptr(), st.seg.data_ptr(), 3,
                                 int(st.seg.shape[1]), int(st.seg.shape[2]), st.offset.data_ptr(), half,
                                 st.clean.data_ptr(), st.finished.data_ptr(), out.data_ptr(), st.l_row, st.l_row, L,
                                 None) == _lib.AMT_OK
        rows.append(out)
    assert torch.equal(rows[0], rows[1]) and bool((rows[0] != 0).any(dim=1).all())
    seen = []

    def look(idx, slot, st):
        seen.append(idx)
        assert torch.equal(st.t_song, fixed.t_song) and st.pool.frames == queue.pool.frames
        for k in fixed.refs:
            assert torch.equal(st.refs[k], fixed.refs[k]), k
    ev, st = lp.run_songs(songs, max_notes=2, silence=1e-4, poll=1, song0=5)
    evs = lp.run_song_queue(songs, 3, max_notes=2, silence=1e-4, poll=1, on_finish=look)
    assert sorted(seen) == [0, 1, 2] and st.slot_song.tolist() == [5, 6, 7]
    e = ev.cpu().numpy()
    assert bool((e[:, 0, 2] == so.FINISHED).any()) and bool((e[:, :, 2] == so.DETECT).any())
    for i in range(3):
        assert np.all(e[:, i, 0] == 5 + i), i
        live = e[:, i][e[:, i, 2] != so.FINISHED]
        assert np.array_equal(live[:, 2:], evs[i][:, 2:]), (i, live.tolist(), evs[i].tolist())


def test_one_refusal_for_short_songs(env):
    """A song of one hop and a song of n_fft / 2 samples (too short for the reflect padding) are refused by run_songs and
    by the queue with one and the same text; n_fft / 2 + 1 samples are walked to the end by both, with equal records."""
    p, lp = _make_loop(env, 2048, 1, 'bank', heads=SYNTHETIC)
    rng = np.random.default_rng(5)
    for n in (p.H, p.N // 2):
        s = rng.standard_normal(n).astype(np.float32)
        with pytest.raises(ValueError, match='Invalid Input shape') as fixed:
            lp.run_songs([s])
        with pytest.raises(ValueError, match='Invalid Input shape') as queue:
            lp.run_song_queue([s], 2)
        assert str(fixed.value) == str(queue.value) and str(n) in str(fixed.value)
    s = (0.1 * rng.standard_normal(p.N // 2 + 1)).astype(np.float32)
    ev, st = lp.run_songs([s], max_notes=2, silence=1e-4, poll=1)
    e = ev.cpu().numpy()[:, 0, :]
    evs = lp.run_song_queue([s], 2, max_notes=2, silence=1e-4, poll=1)
    assert st.finished.tolist() == [1] and len(evs) == 1
    assert len(evs[0]) >= 1 and np.array_equal(e[e[:, 2] != so.FINISHED], evs[0])
