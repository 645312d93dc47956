"""GPU: the device FLAC encoder (amt_flac.hip) against the numpy restatement of its format rule
(tests/flac_encode_reference.py), byte for byte -- the format is all integer, so there are no tolerances -- and through
the product's own reader, the song walk and the command line."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_encode_reference as R                               # noqa: E402
import song_oracle as so                                        # noqa: E402
from oracle import synth as osynth                              # noqa: E402

pytestmark = pytest.mark.gpu
ALL_HEADS = ('timing', 'pitch', 'instrument', 'velocity')
# signal of flac_encode_reference.signals() -> its length in the batch: 1, 3, 5 and the block size +- 1 are all there
LENGTHS = {'zeros': 4097, 'dc': 1, 'impulse': 8229, 'noise_full': 4095, 'square': 4096, 'tone': 8229,
           'tone_noise': 4097, 'loud_quiet': 8229, 'walk': 4096, 'walk2': 5, 'walk3': 8229, 'tiny': 3, 'sparse': 4095,
           'ramp': 8229}
SENTINEL_OUT, SENTINEL_SCRATCH, MARGIN = 0x5A, 0xA5, 64


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import audio, _lib, hyperparams, loop
    return dict(torch=torch, audio=audio, _lib=_lib, lib=_lib.load(), hp=hyperparams, loop=loop)


def _batch(cap=None):
    sig = R.signals()
    waves = []
    for name, n in LENGTHS.items():
        y = sig[name][:n].copy()
        if name == 'ramp':
            y[10], y[11], y[12] = np.nan, np.inf, -np.inf          # NaN -> 0, infinities clip (restatement only)
        waves.append(y if cap is None else y[:cap])
    return waves


_REF = {}


def _reference(bps, blocksize, cap, first_frame=0):
    """Per signal ([frames], md5) of the restatement, computed once per configuration."""
    key = (bps, blocksize, cap, first_frame)
    if key not in _REF:
        out = []
        for y in _batch(cap):
            q = R.quantise(y, bps)
            out.append((R.encode_frames(q, bps, blocksize, first_frame)[0], R.pcm_md5(q, bps)))
        _REF[key] = out
    return _REF[key]


def _encode_raw(env, waves, bps, blocksize, first_frame=0):
    """amt_flac_encode_ragged on a pool with odd, non-adjacent bases and sentinel bytes around every output region.
    Returns per signal (stream bytes, frame sizes, (min, max), md5) after checking the sentinels."""
    torch, lib = env['torch'], env['lib']
    n = len(waves)
    lens = [len(w) for w in waves]
    base, at = [], 3
    for l in lens:
        at |= 1
        base.append(at)
        at += l + 7
    pool = np.full(at + 8, 0.123, np.float32)
    for w, b in zip(waves, base):
        pool[b:b + len(w)] = w
    max_len = max(lens)
    frames = [-(-l // blocksize) for l in lens]
    fmax = max(frames)
    bound = lib.amt_flac_frame_bound(blocksize, bps)
    assert bound == 13 + (8 + blocksize * bps + 7) // 8 + 2
    need = lib.amt_flac_scratch_bytes(n, max_len, blocksize, bps)
    out_bytes = sum(frames) * bound
    dev = torch.device('cuda')
    d_pool = torch.from_numpy(pool).to(dev)
    meta = torch.tensor([base, lens], dtype=torch.int64).to(dev)
    scratch = torch.full((need + MARGIN,), SENTINEL_SCRATCH, dtype=torch.uint8, device=dev)
    out = torch.full((MARGIN + out_bytes + MARGIN,), SENTINEL_OUT, dtype=torch.uint8, device=dev)
    fb = torch.full((n, fmax), -7, dtype=torch.int64, device=dev)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    mm = torch.full((n, 2), -7, dtype=torch.int32, device=dev)
    md5 = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    st = lib.amt_flac_encode_ragged(vp(d_pool.data_ptr()), vp(meta[0].data_ptr()), vp(meta[1].data_ptr()), n, max_len,
                                    blocksize, bps, first_frame, vp(scratch.data_ptr()), need,
                                    vp(out.data_ptr() + MARGIN), out_bytes, vp(fb.data_ptr()), vp(off.data_ptr()),
                                    vp(mm.data_ptr()), vp(md5.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
    assert st == 0, st
    torch.cuda.synchronize()
    out_h, scr_h = out.cpu().numpy(), scratch.cpu().numpy()
    off_h, fb_h, mm_h, md5_h = off.cpu().numpy(), fb.cpu().numpy(), mm.cpu().numpy(), md5.cpu().numpy()
    assert off_h[0] == 0 and np.all(np.diff(off_h) >= 0) and off_h[-1] <= out_bytes
    assert np.all(out_h[:MARGIN] == SENTINEL_OUT), 'bytes before out were written'
    assert np.all(out_h[MARGIN + off_h[-1]:] == SENTINEL_OUT), 'bytes after the last stream were written'
    assert np.all(scr_h[need:] == SENTINEL_SCRATCH), 'bytes past the scratch were written'
    slots = scr_h[:n * fmax * bound].reshape(n, fmax, bound)
    for i in range(n):
        for f in range(fmax):
            assert np.all(slots[i, f, fb_h[i, f]:] == SENTINEL_SCRATCH), ('slot tail', i, f)
    body = out_h[MARGIN:]
    return [(body[off_h[i]:off_h[i + 1]].tobytes(), fb_h[i, :frames[i]].tolist(), fb_h[i, frames[i]:].tolist(),
             tuple(mm_h[i].tolist()), md5_h[i].tobytes()) for i in range(n)]


def _compare(got, ref, tag):
    for i, ((stream, sizes, past, mm, md5), (frames, md5_ref)) in enumerate(zip(got, ref)):
        assert sizes == [len(f) for f in frames], (tag, i, 'frame sizes')
        assert all(p == 0 for p in past), (tag, i, 'sizes past the last frame')
        want = b''.join(frames)
        if stream != want:
            first = next(k for k in range(min(len(stream), len(want))) if stream[k] != want[k]) \
                if stream[:len(want)] != want[:len(stream)] else min(len(stream), len(want))
            raise AssertionError((tag, i, 'bytes differ first at', first, 'of', len(want)))
        assert mm == ((min(sizes), max(sizes)) if sizes else (0, 0)), (tag, i, 'min / max frame')
        assert md5 == md5_ref, (tag, i, 'md5')


@pytest.mark.parametrize('bps,blocksize,cap', [(24, 4096, None), (16, 4096, None), (24, 16, 600), (24, 192, 600),
                                               (16, 192, 600)])
def test_bytes_against_restatement(env, bps, blocksize, cap):
    """One ragged launch of the 14 committed signals (lengths 1, 3, 5, 4095, 4096, 4097, 8229; zeros, DC, impulse,
    full-scale noise, a clipping square, tones, loud and quiet halves, integrated noise, ...), odd non-adjacent bases:
    frames, sizes, min / max, stream offsets and MD5 equal the restatement's; every sentinel byte is untouched."""
    got = _encode_raw(env, _batch(cap), bps, blocksize)
    _compare(got, _reference(bps, blocksize, cap), (bps, blocksize))


def _many_short(count, n):
    """`count` signals of n samples: windows of the committed signals, a different signal and start for neighbours."""
    sig = R.signals()
    names = sorted(LENGTHS)
    return [sig[names[i % len(names)]][7 * i:7 * i + n].copy() for i in range(count)]


@pytest.mark.parametrize('tag', ['301_frames', '300_signals'])
def test_offset_scans_carry_past_one_pass(env, tag):
    """The two offset scans walk their items 256 at a time and carry the running sum on: one signal of 16 * 300 + 5
    samples at block size 16 is 301 frames (the frame-offset scan carries once), 300 signals of 40 samples in one call
    make the stream-offset scan carry.  Bytes, sizes, min / max, offsets and MD5 against the restatement."""
    sig = R.signals()
    waves = [sig['tone_noise'][:16 * 300 + 5].copy()] if tag == '301_frames' else _many_short(300, 40)
    got = _encode_raw(env, waves, 24, 16)
    assert sum(len(sizes) for _, sizes, _, _, _ in got) == (301 if tag == '301_frames' else 900)
    assert len({len(stream) for stream, _, _, _, _ in got}) > (0 if tag == '301_frames' else 10)
    ref = []
    for y in waves:
        q = R.quantise(y, 24)
        ref.append((R.encode_frames(q, 24, 16, 0)[0], R.pcm_md5(q, 24)))
    _compare(got, ref, tag)


@pytest.mark.parametrize('first_frame', [126, 2046, 65534, (1 << 21) - 2, (1 << 26) - 2])
def test_frame_numbers(env, first_frame):
    """Two- and three-block signals at block size 16: the frame numbers first_frame .. first_frame + 2 cross into the
    2-, 3-, 4-, 5- and 6-byte codings."""
    sig = R.signals()
    waves = [sig['tone_noise'][:40], sig['walk'][100:121], sig['zeros'][:17]]
    got = _encode_raw(env, waves, 24, 16, first_frame)
    ref = []
    for y in waves:
        q = R.quantise(y, 24)
        ref.append((R.encode_frames(q, 24, 16, first_frame)[0], R.pcm_md5(q, 24)))
    _compare(got, ref, first_frame)
    assert len(R.utf8_num(first_frame + 1)) + 1 == len(R.utf8_num(first_frame + 2))


def test_frame_number_limit_is_invalid(env):
    """first_frame + frames >= 2^31 is AMT_E_INVALID, returned before any pointer is looked at."""
    lib, _lib = env['lib'], env['_lib']
    one = ctypes.c_void_p(8)
    args = lambda ff, n_len: (one, one, one, 1, n_len, 16, 24, ff, one, 1 << 30, one, 1 << 30, one, one, one, one, None)
    assert lib.amt_flac_encode_ragged(*args((1 << 31) - 1, 32)) == _lib.AMT_E_INVALID
    assert lib.amt_flac_encode_ragged(*args((1 << 31) - 2, 32)) == _lib.AMT_E_INVALID      # first_frame + 2 frames = 2^31


def test_independence_and_repeat(env):
    """Every signal's stream from the batch equals its stream encoded alone (another base, another grid), and the same
    launch twice gives the same bytes."""
    waves = _batch()
    a = _encode_raw(env, waves, 24, 4096)
    b = _encode_raw(env, waves, 24, 4096)
    assert a == b
    torch, audio = env['torch'], env['audio']
    for i, w in enumerate(waves):
        t = torch.from_numpy(w).cuda()
        out, off, mm, md5, fb = audio.flac_encode_streams([t], bps=24, blocksize=4096)
        total = int(off[1])
        assert out[:total].cpu().numpy().tobytes() == a[i][0], i
        assert md5[0].cpu().numpy().tobytes() == a[i][4] and tuple(mm[0].tolist()) == a[i][3], i


def test_save_flac_through_the_reader(env, tmp_path):
    """audio.save_flac files decode with CRC-8, CRC-16 and MD5 verified to exactly clip(rint(y 2^(bps-1))) of the host
    copy; a 0-sample signal is a valid file of 42 bytes; a [3, n] tensor gives three files whose rows were not copied."""
    from amt_saga import flac
    torch, audio = env['torch'], env['audio']
    sig = R.signals()
    rows = torch.from_numpy(np.stack([sig['tone'][:4500], sig['loud_quiet'][:4500], sig['zeros'][:4500]])).cuda()
    single = torch.from_numpy(sig['tone_noise'][:5000]).cuda()
    empty = torch.zeros((0,), dtype=torch.float32, device='cuda')
    for bps in (24, 16):
        paths = [str(tmp_path / ('f%d_%d.flac' % (bps, i))) for i in range(5)]
        audio.save_flac([single, empty, rows], paths, 44100, bps=bps)
        hosts = [single.cpu().numpy(), np.zeros(0, np.float32)] + list(rows.cpu().numpy())
        for path, y in zip(paths, hosts):
            if len(y) == 0:
                assert os.path.getsize(path) == 42
            pcm, sr, b = flac.decode(path, verify=True)
            lim = float(1 << (bps - 1))
            want = np.clip(np.rint(y.astype(np.float64) * lim), -lim, lim - 1).astype(np.int64)
            assert (sr, b) == (44100, bps) and np.array_equal(pcm[:, 0] if len(y) else pcm.reshape(-1), want), path
    sigs = audio._device_signals(rows)
    assert [s.data_ptr() for s in sigs] == [rows[g].data_ptr() for g in range(3)]
    files = audio.flac_encode(rows, 44100)
    assert len(files) == 3 and files[0] == open(str(tmp_path / 'f24_2.flac'), 'rb').read()
    with pytest.raises(ValueError):
        audio.save_flac([single], paths[:2], 44100)
    with pytest.raises(ValueError):
        audio.flac_encode([single.double()], 44100)


def _make_loop(env, shift=0, heads=ALL_HEADS, groups=(0, 1, 2)):
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)     # 86-frame windows: the smallest live walk
    lp = env['loop'].TranscriptionLoop(p, heads=heads, guess='bank', groups=groups)
    if shift:
        w = {k: v.copy() for k, v in lp.nets['timing_start'].weights.items()}
        w['dense2/bias'] = w['dense2/bias'] + np.float32(shift)
        lp.nets['timing_start'].set_weights(w)
    return p, lp.setup_device()


def test_walk_audio_host_and_device_writers(env, tmp_path):
    """transcribe(traversal='song', residual=True, stems=True) on the smallest live walk, written once by the host
    writer and once by save_flac: the decoded PCM is equal file for file and no device file is larger.  The stems of
    the plain_slides song, where nothing is detected, are CONSTANT frames only."""
    from amt_saga import flac, transcribe as tr
    torch, audio = env['torch'], env['audio']
    p, lp = _make_loop(env)
    for song in so.make_songs(p, 29, (3.1, 1.4, 4.0, 0.7, 2.6)):   # the first song whose walk takes something out
        notes, evs, res, stems = tr.transcribe(song, p, iters=2, traversal='song', residual=True, stems=True, loop=lp,
                                               silence=1e-4)
        if bool((stems != 0).any()):
            break
    assert bool((stems != 0).any()) and bool((res != 0).any())
    for writer in tr.FLAC_WRITERS:
        d = tmp_path / writer
        os.makedirs(str(d))
        tr.write_song_audio(p.sr, residual=res, residual_path=str(d / 'res.flac'), stems=stems, stems_dir=str(d),
                            name='s', flac=writer)
    names = sorted(os.listdir(str(tmp_path / 'host')))
    assert names == sorted(os.listdir(str(tmp_path / 'device'))) == ['res.flac', 's.group0.flac', 's.group1.flac',
                                                                     's.group2.flac']
    for name in names:
        h, dv = str(tmp_path / 'host' / name), str(tmp_path / 'device' / name)
        a, b = flac.decode(h, verify=True), flac.decode(dv, verify=True)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], name
        assert os.path.getsize(dv) <= os.path.getsize(h), name
        print('%s: host %d bytes, device %d' % (name, os.path.getsize(h), os.path.getsize(dv)))
    with pytest.raises(ValueError):
        tr.write_song_audio(p.sr, residual=res, residual_path=str(tmp_path / 'x.flac'), flac='gpu')
    # nothing detected: every stem frame is a CONSTANT subframe (header, 0x00, the 24-bit sample, CRC-16)
    nfft, wsec, guess, seed, lengths, max_notes, silence, silent, shift = so.WALK_CASES['plain_slides']
    p2, lp2 = _make_loop(env, shift, heads=so.HEADS, groups=(0,))
    songs = so.make_songs(p2, seed, lengths[:1], silent)
    _, st = lp2.run_songs(songs, max_notes=max_notes, silence=silence, poll=4, stems=True)
    out, off, mm, md5, fb = audio.flac_encode_streams(st.stem_audio[0])
    sizes = fb.cpu().numpy()
    assert sizes.shape[0] == 1 and sizes.shape[1] >= 2
    assert np.all(sizes == 4 + 1 + 2 + 1 + 4 + 2), sizes                      # all below frame 128: one-byte numbers
    body = out[:int(off[-1])].cpu().numpy().reshape(-1, 14)
    assert np.all(body[:, 8] == 0x00) and np.all(body[:, 9:12] == 0)


def test_command_line_flac_device(env, tmp_path, monkeypatch):
    """--flac device in --traversal song mode and in --songs mode (the model set-up of the command line, 516-frame
    windows, is paid once, about 11 s as in test_gpu_song_stems): the files decode with CRC and MD5 verified and hold
    the PCM of the --flac host files."""
    from amt_saga import flac, transcribe as tr
    loops, make = {}, tr._make_loop

    def make_once(p, iters, heads, groups, weights_dir, guess):      # the three runs below share one model set-up
        key = (p.N, p.sr, p.timing_frames, iters, tuple(heads), tuple(groups), weights_dir, guess)
        if key not in loops:
            loops[key] = make(p, iters, heads, groups, weights_dir, guess)
        return loops[key]
    monkeypatch.setattr(tr, '_make_loop', make_once)
    p = env['hp'].Hyperparams(N=2048, sr=44100)
    n = int(1.3 * p.H * (p.timing_frames - 1))
    notes_in = [(0, 60, 100, 0.2, 0.5), (0, 64, 90, 0.9, 0.4), (1, 67, 80, 2.6, 0.6), (2, 72, 110, 5.4, 0.3)]
    wf = osynth.render_window(notes_in, n, p.sr).numpy()
    src, other = str(tmp_path / 'clip.flac'), str(tmp_path / 'other.flac')
    flac.save_float(wf, src, p.sr)
    flac.save_float(wf[:n // 2], other, p.sr)
    dirs = {}
    for writer in ('host', 'device'):
        d = tmp_path / writer
        os.makedirs(str(d))
        tr.main([src, str(d / 'cli.mid'), '--iters', '1', '--traversal', 'song', '--residual', str(d / 'left.flac'),
                 '--stems-dir', str(d / 'stems'), '--flac', writer])
        dirs[writer] = d
    tr.main(['--songs', src, other, '--out-dir', str(tmp_path / 'mid'), '--slots', '2', '--iters', '1', '--stems-dir',
             str(tmp_path / 'qstems'), '--residual-dir', str(tmp_path / 'qres'), '--flac', 'device'])
    stem_names = ['clip.group%d.flac' % g for g in range(3)]
    assert sorted(os.listdir(str(dirs['device'] / 'stems'))) == stem_names
    pairs = [(dirs['host'] / 'left.flac', dirs['device'] / 'left.flac')]
    pairs += [(dirs['host'] / 'stems' / s, dirs['device'] / 'stems' / s) for s in stem_names]
    pairs += [(dirs['host'] / 'stems' / s, tmp_path / 'qstems' / s) for s in stem_names]     # the queue = the song alone
    pairs += [(dirs['host'] / 'left.flac', tmp_path / 'qres' / 'clip.residual.flac')]
    host = {}
    for h, dv in pairs:
        if h not in host:
            host[h] = flac.decode(str(h), verify=True)
        got = flac.decode(str(dv), verify=True)
        assert np.array_equal(host[h][0], got[0]) and host[h][1:] == got[1:], dv
        assert os.path.getsize(str(dv)) <= os.path.getsize(str(h)), dv
    assert flac.decode(str(tmp_path / 'qres' / 'other.residual.flac'), verify=True)[0].shape[0] == p.H * (n // 2 // p.H)
