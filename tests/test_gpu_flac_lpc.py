"""GPU: the device FLAC encoder with linear prediction (amt_flac_encode_lpc_ragged, predictor='lpc') against the numpy
restatement of its rule (tests/flac_lpc_reference.py), byte for byte -- no tolerances -- and through the product's own
readers, the device decoder, the song walk and the command line."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_encode_reference as R                               # noqa: E402
import flac_lpc_reference as L                                  # noqa: E402
import song_oracle as so                                        # noqa: E402
from oracle import synth as osynth                              # noqa: E402

pytestmark = pytest.mark.gpu
ALL_HEADS = ('timing', 'pitch', 'instrument', 'velocity')
# signal -> its length in the batch: 1, 3, 5, 13 and the block size +- 1 are all there; the last five are
# flac_lpc_reference.more_signals()
LENGTHS = {'zeros': 4097, 'dc': 1, 'impulse': 8229, 'noise_full': 4095, 'square': 4096, 'tone': 8229,
           'tone_noise': 4097, 'loud_quiet': 8229, 'walk': 4096, 'walk2': 5, 'walk3': 8229, 'tiny': 3, 'sparse': 4095,
           'ramp': 8229, 'harmonics': 8229, 'harmonics_quiet': 4097, 'lowpass': 4095, 'alternating': 8229,
           'slow_sine': 13}
SENTINEL_OUT, SENTINEL_SCRATCH, MARGIN = 0x5A, 0xA5, 64


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import audio, _lib, hyperparams, loop
    return dict(torch=torch, audio=audio, _lib=_lib, lib=_lib.load(), hp=hyperparams, loop=loop)


def _batch(cap=None, names=None):
    sig = dict(R.signals())
    sig.update(L.more_signals())
    waves = []
    for name, n in LENGTHS.items():
        if names is not None and name not in names:
            continue
        y = sig[name][:n].copy()
        if name == 'ramp':
            y[10], y[11], y[12] = np.nan, np.inf, -np.inf          # NaN -> 0, infinities clip
        waves.append(y if cap is None else y[:cap])
    return waves


_REF = {}


def _reference(bps, blocksize, cap, first_frame=0, order=12, names=None):
    """Per signal ([frames], md5, [choices]) of the restatement, computed once per configuration."""
    key = (bps, blocksize, cap, first_frame, order, names)
    if key not in _REF:
        out = []
        for y in _batch(cap, names):
            q = R.quantise(y, bps)
            frames, choices = L.encode_frames(q, bps, blocksize, first_frame, order)
            out.append((frames, R.pcm_md5(q, bps), choices))
        _REF[key] = out
    return _REF[key]


def _encode_raw(env, waves, bps, blocksize, first_frame=0, order=12):
    """amt_flac_encode_lpc_ragged on a pool with odd, non-adjacent bases and sentinel bytes around every output region.
    Returns per signal (stream bytes, frame sizes, sizes past the last frame, (min, max), md5) after checking the
    sentinels."""
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
    st = lib.amt_flac_encode_lpc_ragged(vp(d_pool.data_ptr()), vp(meta[0].data_ptr()), vp(meta[1].data_ptr()), n,
                                        max_len, blocksize, bps, first_frame, order, vp(scratch.data_ptr()), need,
                                        vp(out.data_ptr() + MARGIN), out_bytes, vp(fb.data_ptr()), vp(off.data_ptr()),
                                        vp(mm.data_ptr()), vp(md5.data_ptr()),
                                        vp(torch.cuda.current_stream().cuda_stream))
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
    for i, ((stream, sizes, past, mm, md5), (frames, md5_ref, choices)) in enumerate(zip(got, ref)):
        want = b''.join(frames)
        if stream != want or sizes != [len(f) for f in frames]:
            at, f = 0, 0
            for f, fr in enumerate(frames):                        # the first frame that differs, and what it should be
                if stream[at:at + len(fr)] != fr:
                    break
                at += len(fr)
            raise AssertionError((tag, i, 'frame', f, 'differs; the rule chooses', choices[f][:3],
                                  'sizes', sizes, [len(x) for x in frames]))
        assert all(p == 0 for p in past), (tag, i, 'sizes past the last frame')
        assert mm == ((min(sizes), max(sizes)) if sizes else (0, 0)), (tag, i, 'min / max frame')
        assert md5 == md5_ref, (tag, i, 'md5')


@pytest.mark.parametrize('bps,blocksize,cap', [(24, 4096, None), (16, 4096, None), (24, 16, 600), (24, 192, 600),
                                               (16, 192, 600), (16, 16, 600)])
def test_bytes_against_restatement(env, bps, blocksize, cap):
    """One ragged launch of the 19 signals (lengths 1, 3, 5, 13, 4095, 4096, 4097, 8229; NaN and infinities in one), odd
    non-adjacent bases: frames, sizes, min / max, stream offsets and MD5 equal the restatement's; every sentinel byte is
    untouched.  The restatement's choices for these very inputs include LPC subframes."""
    ref = _reference(bps, blocksize, cap)
    got = _encode_raw(env, _batch(cap), bps, blocksize)
    _compare(got, ref, (bps, blocksize))
    kinds = [c[0] for r in ref for c in r[2]]
    assert 'LPC' in kinds and 'FIXED' in kinds and 'CONSTANT' in kinds and 'VERBATIM' in kinds, set(kinds)
    if cap is None:
        assert len({c[1] for r in ref for c in r[2] if c[0] == 'LPC'}) >= 5


SUBSET = ('tone', 'tone_noise', 'ramp', 'harmonics', 'alternating', 'square', 'zeros', 'walk2')


@pytest.mark.parametrize('order', [1, 5])
def test_orders(env, order):
    """lpc_order 1 and 5 on a subset at 24 bit: no LPC subframe above the order, bytes equal."""
    ref = _reference(24, 4096, None, 0, order, SUBSET)
    assert {c[1] for r in ref for c in r[2] if c[0] == 'LPC'} <= set(range(1, order + 1))
    assert any(c[0] == 'LPC' for r in ref for c in r[2])
    _compare(_encode_raw(env, _batch(None, SUBSET), 24, 4096, 0, order), ref, order)


@pytest.mark.parametrize('first_frame', [126, 65534])
def test_frame_numbers(env, first_frame):
    """Three-block signals at block size 16 whose frame numbers cross into the 2- and the 4-byte coding."""
    more = L.more_signals()
    waves = [more['alternating'][:40], R.signals()['tone_noise'][:40], more['harmonics'][100:121]]
    ref = []
    for y in waves:
        q = R.quantise(y, 24)
        frames, choices = L.encode_frames(q, 24, 16, first_frame)
        ref.append((frames, R.pcm_md5(q, 24), choices))
    assert any(c[0] == 'LPC' for r in ref for c in r[2])
    _compare(_encode_raw(env, waves, 24, 16, first_frame), ref, first_frame)


def test_independence_repeat_and_fixed_keyword(env):
    """Every signal's stream from the batch equals its stream encoded alone (another base, another grid); the same
    launch twice gives the same bytes; predictor='fixed' through the new keyword gives the bytes of a plain call, and
    the LPC files are never larger."""
    torch, audio = env['torch'], env['audio']
    waves = _batch()
    a = _encode_raw(env, waves, 24, 4096)
    assert a == _encode_raw(env, waves, 24, 4096)
    dev = [torch.from_numpy(w).cuda() for w in waves]
    for i, t in enumerate(dev):
        out, off, mm, md5, fb = audio.flac_encode_streams([t], bps=24, blocksize=4096, predictor='lpc')
        assert out[:int(off[1])].cpu().numpy().tobytes() == a[i][0], i
        assert md5[0].cpu().numpy().tobytes() == a[i][4] and tuple(mm[0].tolist()) == a[i][3], i
    plain = audio.flac_encode(dev, 44100)
    assert audio.flac_encode(dev, 44100, predictor='fixed') == plain
    assert audio.flac_encode(dev, 44100, predictor='fixed', lpc_order=3) == plain
    lpc = audio.flac_encode(dev, 44100, predictor='lpc')
    assert all(len(x) <= len(y) for x, y in zip(lpc, plain)) and sum(map(len, lpc)) < sum(map(len, plain))
    assert [x[42:] for x in lpc] == [s[0] for s in a]
    with pytest.raises(ValueError):
        audio.flac_encode(dev, 44100, predictor='lpc', lpc_order=13)


def test_device_decoder_and_save_flac(env, tmp_path):
    """The encoder's LPC output through the device decoder's LPC path (CRC-16 and MD5 verified) and through the host
    reader: the quantised samples; a [3, n] tensor gives three files."""
    from amt_saga import flac
    torch, audio = env['torch'], env['audio']
    for bps in (24, 16):
        waves = [w for w in _batch() if len(w)]
        dev = [torch.from_numpy(w).cuda() for w in waves]
        files = audio.flac_encode(dev, 44100, bps=bps, predictor='lpc')
        orders = {c[1] for r in _reference(bps, 4096, None) for c in r[2] if c[0] == 'LPC'}
        assert len(orders) >= 3, orders                            # the decoder's LPC path gets several orders
        res = audio.flac_decode(files, verify=True, pcm=True)
        for i, (w, r) in enumerate(zip(waves, res)):
            assert np.array_equal(r[-1].cpu().numpy().reshape(-1), R.quantise(w, bps)), (bps, i)
    more = L.more_signals()
    rows = torch.from_numpy(np.stack([more['harmonics'][:4500], R.signals()['tone_noise'][:4500],
                                      more['alternating'][:4500]])).cuda()
    paths = [str(tmp_path / ('g%d.flac' % g)) for g in range(3)]
    audio.save_flac(rows, paths, 44100, predictor='lpc')
    fixed = audio.flac_encode(rows, 44100)
    for g, path in enumerate(paths):
        pcm, sr, b = flac.decode(path, verify=True)
        assert (sr, b) == (44100, 24) and np.array_equal(pcm[:, 0], R.quantise(rows[g].cpu().numpy(), 24)), g
        assert os.path.getsize(path) < len(fixed[g]), g
        assert open(path, 'rb').read() == L.encode_file(rows[g].cpu().numpy(), 44100, 24, 4096)[0], g


def _make_loop(env, heads=ALL_HEADS, groups=(0, 1, 2)):
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)     # 86-frame windows: the smallest live walk
    lp = env['loop'].TranscriptionLoop(p, heads=heads, guess='bank', groups=groups)
    return p, lp.setup_device()


def test_walk_audio_lpc_against_fixed(env, tmp_path):
    """transcribe(traversal='song', residual=True, stems=True) on the smallest live walk, written by the device encoder
    with the fixed predictors and with LPC: the decoded PCM is equal file for file and no LPC file is larger."""
    from amt_saga import flac, transcribe as tr
    p, lp = _make_loop(env)
    for song in so.make_songs(p, 29, (3.1, 1.4, 4.0, 0.7, 2.6)):   # the first song whose walk takes something out
        notes, evs, res, stems = tr.transcribe(song, p, iters=2, traversal='song', residual=True, stems=True, loop=lp,
                                               silence=1e-4)
        if bool((stems != 0).any()):
            break
    assert bool((stems != 0).any()) and bool((res != 0).any())
    for predictor in ('fixed', 'lpc'):
        d = tmp_path / predictor
        os.makedirs(str(d))
        tr.write_song_audio(p.sr, residual=res, residual_path=str(d / 'res.flac'), stems=stems, stems_dir=str(d),
                            name='s', flac='device', predictor=predictor)
    names = sorted(os.listdir(str(tmp_path / 'fixed')))
    assert names == sorted(os.listdir(str(tmp_path / 'lpc'))) == ['res.flac', 's.group0.flac', 's.group1.flac',
                                                                  's.group2.flac']
    for name in names:
        f, l = str(tmp_path / 'fixed' / name), str(tmp_path / 'lpc' / name)
        a, b = flac.decode(f, verify=True), flac.decode(l, verify=True)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], name
        assert os.path.getsize(l) <= os.path.getsize(f), name
        print('%s: fixed %d bytes, lpc %d' % (name, os.path.getsize(f), os.path.getsize(l)))
    with pytest.raises(ValueError):
        tr.write_song_audio(p.sr, residual=res, residual_path=str(tmp_path / 'x.flac'), flac='host', predictor='lpc')
    assert not os.path.exists(str(tmp_path / 'x.flac'))


def test_command_line_flac_predictor_lpc(env, tmp_path, monkeypatch):
    """--flac device --flac-predictor lpc in --traversal song mode and in --songs mode against --flac host (one model
    set-up for the three runs, as test_gpu_flac_encode does it): the files decode with CRC and MD5 verified and hold the
    PCM of the host files, none larger."""
    from amt_saga import flac, transcribe as tr
    loops, make = {}, tr._make_loop

    def make_once(p, iters, heads, groups, weights_dir, guess):
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
    for writer, extra in (('host', []), ('device', ['--flac-predictor', 'lpc'])):
        d = tmp_path / writer
        os.makedirs(str(d))
        tr.main([src, str(d / 'cli.mid'), '--iters', '1', '--traversal', 'song', '--residual', str(d / 'left.flac'),
                 '--stems-dir', str(d / 'stems'), '--flac', writer] + extra)
        dirs[writer] = d
    tr.main(['--songs', src, other, '--out-dir', str(tmp_path / 'mid'), '--slots', '2', '--iters', '1', '--stems-dir',
             str(tmp_path / 'qstems'), '--residual-dir', str(tmp_path / 'qres'), '--flac', 'device', '--flac-predictor',
             'lpc'])
    stem_names = ['clip.group%d.flac' % g for g in range(3)]
    assert sorted(os.listdir(str(dirs['device'] / 'stems'))) == stem_names
    pairs = [(dirs['host'] / 'left.flac', dirs['device'] / 'left.flac')]
    pairs += [(dirs['host'] / 'stems' / s, dirs['device'] / 'stems' / s) for s in stem_names]
    pairs += [(dirs['host'] / 'stems' / s, tmp_path / 'qstems' / s) for s in stem_names]
    pairs += [(dirs['host'] / 'left.flac', tmp_path / 'qres' / 'clip.residual.flac')]
    host, lpc_subframes = {}, 0
    for h, dv in pairs:
        if h not in host:
            host[h] = flac.decode(str(h), verify=True)
        got = flac.decode(str(dv), verify=True)
        assert np.array_equal(host[h][0], got[0]) and host[h][1:] == got[1:], dv
        assert os.path.getsize(str(dv)) <= os.path.getsize(str(h)), dv
        # the restatement of the LPC rule on the decoded PCM gives the file's frames 3 .. 5 (the first note sounds
        # there): the command line did ask for LPC
        q = got[0][3 * 4096:6 * 4096, 0].astype(np.int64)
        frames, choices = L.encode_frames(q, 24, 4096, first_frame=3)
        assert b''.join(frames) in open(str(dv), 'rb').read(), dv
        lpc_subframes += sum(c[0] == 'LPC' for c in choices)
    assert lpc_subframes > 0
