"""GPU: the device resampler (amt_resample_ragged, amt_saga.audio.Resampler / resample, transcribe(sr=...), --sr)
against the float64 definition of tests/resample_reference.py.

Bar of every comparison, per output sample (u = 2^-24):

    |y_gpu - y_f64| <= (taps_n + C + 2) u sum_m |h| mean_c |x[m][c]|      over that sample's own taps

(resample_reference.bar: the forward bound of a float32 dot product of that length plus the coefficient rounding and
the channel mean).  The largest ratio error / bar of every case is printed and, when the environment variable
AMT_RECORD_DIR names a directory, written there as resample_error_vs_f64.json.  The assertions are the bar; the ratio
is a record."""
import json
import os

import numpy as np
import pytest

import resample_reference as rr      # tests/resample_reference.py

pytestmark = pytest.mark.gpu

SENT = -7.0
RECORD = {}


def _note(kind, sr_in, sr_out, ratio):
    key = (kind, sr_in, sr_out)
    RECORD[key] = max(RECORD.get(key, 0.0), float(ratio))


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    rows = [dict(kind=k[0], sr_in=k[1], sr_out=k[2], max_error_over_bar=RECORD[k]) for k in sorted(RECORD)]
    out = os.environ.get('AMT_RECORD_DIR')
    if out:
        try:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, 'resample_error_vs_f64.json'), 'w') as f:
                json.dump(rows, f, indent=1)
        except OSError:
            pass
    for r in rows:
        print('error / bar  %-10s %6d -> %6d  %.4f' % (r['kind'], r['sr_in'], r['sr_out'], r['max_error_over_bar']))


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import audio, _lib
    return dict(torch=torch, lib=_lib.load(), _lib=_lib, audio=audio)


def _noise(n, seed, channels=None):
    """Seeded N(0, 1) noise with the first and the last sample at 8.0: the zero extension at both ends carries weight."""
    x = np.random.default_rng(seed).standard_normal(n if channels is None else (n, channels)).astype(np.float32)
    x[0] = x[-1] = 8.0
    return x


def _check(kind, x, y_gpu, sr_in, sr_out, ns=None):
    """y_gpu (numpy, the outputs ns or all of them) against the definition at the bar; returns the largest ratio."""
    y, scale, taps = rr.resample_at(x, sr_in, sr_out, ns)
    assert y_gpu.shape == y.shape
    channels = 1 if np.ndim(x) == 1 else np.shape(x)[1]
    b = rr.bar(scale, taps, channels)
    err = np.abs(y_gpu.astype(np.float64) - y)
    ratio = float(np.max(err / np.maximum(b, 1e-300)))
    print('%s %d -> %d, %d in, %d out: error / bar %.4f' % (kind, sr_in, sr_out, len(x), len(y), ratio))
    _note(kind, sr_in, sr_out, ratio)
    worst = int(np.argmax(err - b))
    assert np.all(err <= b), (kind, sr_in, sr_out, len(x), worst, err[worst], b[worst])
    return ratio


def _lengths(sr_in, sr_out):
    """1, 2, 37, 1000, 4097 and the first length whose output count reaches 3 tiles + 5 (exactly 3 * tile + 5 when
    decimating; an interpolator cannot hit every count)."""
    L, M, _ = rr.ratio(sr_in, sr_out)
    big = -((-(3 * rr.TILE + 5) * M) // L)
    while rr.out_len(big - 1, sr_in, sr_out) >= 3 * rr.TILE + 5:
        big -= 1
    n_out = rr.out_len(big, sr_in, sr_out)
    assert 3 * rr.TILE + 5 <= n_out < 4 * rr.TILE and (L > M or n_out == 3 * rr.TILE + 5)
    return [1, 2, 37, 1000, 4097, big]


@pytest.mark.parametrize('sr_in,sr_out', rr.PAIRS + [rr.STEEP], ids=lambda v: str(v))
def test_every_rate_pair_and_length(env, sr_in, sr_out):
    """Every output of every length against the definition.  The last pair (44100 -> 4000, 11 input samples per output
    and 706 taps) is the one whose tiles need more input than one LDS piece holds: the kernel's several-piece walk."""
    rs = env['audio'].Resampler(sr_in, sr_out)
    L, M, _ = rr.ratio(sr_in, sr_out)
    if (sr_in, sr_out) == rr.STEEP:
        assert rr.TILE * M // L + rs.taps > 8192                   # more than one piece of AMT_RS_CHUNK samples
    for i, n_in in enumerate(_lengths(sr_in, sr_out)):
        x = _noise(n_in, 100 + i)
        y = rs(x)
        assert y.is_cuda and y.dtype == env['torch'].float32 and y.shape == (rr.out_len(n_in, sr_in, sr_out),)
        assert env['lib'].amt_resample_length(rs._handle(), n_in) == y.shape[0] == rs.out_len(n_in)
        _check('noise', x, y.cpu().numpy(), sr_in, sr_out)


def test_ragged_batch_bit_identical_and_in_bounds(env):
    """Three signals at bases that are no multiple of 16 bytes, through the C ABI: each equals the single-signal call
    bit for bit, nothing outside the three output regions is written, and a signal whose region leaves a buffer is left
    unwritten."""
    torch, lib = env['torch'], env['lib']
    for sr_in, sr_out in ((48000, 44100), (44100, 48000), rr.STEEP):
        rs = env['audio'].Resampler(sr_in, sr_out)
        lens, in_base = [4097, 1, 1500], [3, 4103, 4111]
        xs = [_noise(n, 7 + k) for k, n in enumerate(lens)]
        olens = [rs.out_len(n) for n in lens]
        out_base = [5, 5 + olens[0] + 7, 5 + olens[0] + 7 + olens[1] + 7]
        buf = torch.full((in_base[2] + lens[2] + 9,), float('nan'), device='cuda')
        for x, b in zip(xs, in_base):
            buf[b:b + len(x)] = torch.from_numpy(x).cuda()
        out = torch.full((out_base[2] + olens[2] + 11,), SENT, device='cuda')
        meta = torch.tensor([in_base, lens, out_base], dtype=torch.int64, device='cuda')
        st = lib.amt_resample_ragged(rs._handle(), buf.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), 3, 1,
                                     buf.numel(), max(olens), out.data_ptr(), meta[2].data_ptr(), out.numel(), None)
        assert st == 0
        got = out.cpu().numpy()
        keep = np.ones(len(got), bool)
        for x, b, n in zip(xs, out_base, olens):
            alone = rs(x).cpu().numpy()
            assert np.array_equal(got[b:b + n], alone)
            keep[b:b + n] = False
        assert np.all(got[keep] == SENT)
        _check('ragged', xs[0], got[out_base[0]:out_base[0] + olens[0]], sr_in, sr_out)
        # the same call with buffers declared one float too short for the last signal: that signal stays unwritten
        for short_in, short_out in ((1, 0), (0, 1)):
            out2 = torch.full_like(out, SENT)
            st = lib.amt_resample_ragged(rs._handle(), buf.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), 3, 1,
                                         in_base[2] + lens[2] - short_in, max(olens), out2.data_ptr(),
                                         meta[2].data_ptr(), out_base[2] + olens[2] - short_out, None)
            assert st == 0
            got2 = out2.cpu().numpy()
            assert np.array_equal(got2[:out_base[2]], got[:out_base[2]]) and np.all(got2[out_base[2]:] == SENT)
    # the list form of the Python object packs the same way
    rs = env['audio'].Resampler(48000, 44100)
    ys = rs(xs)
    assert [tuple(y.shape) for y in ys] == [(rs.out_len(n),) for n in lens]
    assert all(np.array_equal(y.cpu().numpy(), rs(x).cpu().numpy()) for x, y in zip(xs, ys))
    assert ys[1].data_ptr() == ys[0].data_ptr() + 4 * ys[0].numel()            # views of one packed buffer


def test_c_abi_argument_checks(env):
    lib, _lib = env['lib'], env['_lib']
    import ctypes
    h = ctypes.c_void_p()
    for bad in ((0, 44100), (44100, -1), (44100, 44100), (44100, 48001)):
        assert lib.amt_resampler_create(ctypes.byref(h), *bad) == _lib.AMT_E_INVALID
    rs = env['audio'].Resampler(48000, 44100)
    t = env['torch'].zeros(64, device='cuda')
    m = env['torch'].zeros(3, 1, dtype=env['torch'].int64, device='cuda')
    p, q = t.data_ptr(), m.data_ptr()
    assert lib.amt_resample_ragged(None, p, q, q, 1, 1, 64, 8, p, q, 64, None) == _lib.AMT_E_INVALID
    assert lib.amt_resample_ragged(rs._handle(), p, q, q, 1, 9, 64, 8, p, q, 64, None) == _lib.AMT_E_INVALID
    assert lib.amt_resample_ragged(rs._handle(), p, q, q, 1, 0, 64, 8, p, q, 64, None) == _lib.AMT_E_INVALID
    assert lib.amt_resample_ragged(rs._handle(), p, q, q, 0, 1, 64, 8, p, q, 64, None) == _lib.AMT_E_INVALID
    assert lib.amt_resample_ragged(rs._handle(), p, q, q, 1, 1, 64, 65, p, q, 64, None) == _lib.AMT_E_SHAPE
    assert lib.amt_resample_length(None, 5) < 0


@pytest.mark.parametrize('channels', (2, 3))
def test_channels(env, channels):
    """Interleaved channels against the definition on the float64 mean; with three channels the second cancels the
    first exactly, so the mean is a third of the last."""
    for sr_in, sr_out in ((48000, 44100), (16000, 44100)):
        x = _noise(2500, 40 + channels, channels)
        if channels == 3:
            x[:, 1] = -x[:, 0]
        y = env['audio'].Resampler(sr_in, sr_out)(x)
        _check('channels%d' % channels, x, y.cpu().numpy(), sr_in, sr_out)
        yt = env['audio'].Resampler(sr_in, sr_out)(env['torch'].from_numpy(x).cuda())
        assert np.array_equal(yt.cpu().numpy(), y.cpu().numpy())


def test_64_bit_indices(env):
    """192000 -> 44100 (M = 640) on 15,000,000 samples: n M passes 2^31 from output 3,355,444 of 3,445,313."""
    torch = env['torch']
    sr_in, sr_out, n_in = 192000, 44100, 15_000_000
    g = torch.Generator(device='cuda')
    g.manual_seed(1234)
    x = torch.randn(n_in, generator=g, device='cuda')
    rs = env['audio'].Resampler(sr_in, sr_out)
    y = rs(x)
    n_out = rs.out_len(n_in)
    assert (rs.M, n_out) == (640, 3_445_313) and y.shape == (n_out,)
    assert 3_355_443 * 640 < 2 ** 31 <= 3_355_444 * 640
    rng = np.random.default_rng(99)
    ns = np.sort(np.concatenate([rng.integers(0, n_out - 50_000, 1000), rng.integers(n_out - 50_000, n_out, 999),
                                 [n_out - 1]]))
    assert np.sum(ns >= 3_355_444) >= 1000
    y_ns = y[torch.from_numpy(ns).cuda()].cpu().numpy()
    _check('int64', x.cpu().numpy(), y_ns, sr_in, sr_out, ns)


def test_quality_on_the_device(env):
    """48000 -> 44100: a 1 kHz tone keeps its RMS within 0.05 dB, a 23 kHz tone comes out at or below -90 dB."""
    rs = env['audio'].Resampler(48000, 44100)
    x1, x23 = rr.tone(1000.0, 48000, 0.25), rr.tone(23000.0, 48000, 0.25)
    y1, y23 = (y.cpu().numpy() for y in rs([x1, x23]))
    gain = rr.db(rr.middle_rms(y1) / rr.middle_rms(x1))
    stop = rr.db(rr.middle_rms(y23) / rr.middle_rms(x23))
    print('device 48000 -> 44100: 1 kHz %+.4f dB, 23 kHz %.1f dB' % (gain, stop))
    assert abs(gain) <= 0.05
    assert stop <= -90.0


def test_python_surface(env):
    torch, audio = env['torch'], env['audio']
    from amt_saga.hyperparams import Hyperparams
    from amt_saga.loop import TranscriptionLoop
    rs = audio.Resampler(22050, 44100)
    assert (rs.L, rs.M, rs.taps) == (2, 1, 65) and rs.out_len(1001) == 2002
    x = _noise(30000, 3)
    host, dev = rs(x), rs(torch.from_numpy(x).cuda())
    f64 = rs(x.astype(np.float64))
    assert host.is_cuda and host.dtype == torch.float32 and host.shape == (60000,)
    assert torch.equal(host, dev) and torch.equal(host, f64)
    as_list = rs([x, torch.from_numpy(x[:777]).cuda()])
    assert isinstance(as_list, list) and torch.equal(as_list[0], host) and torch.equal(as_list[1], rs(x[:777]))
    out = torch.full((60000 + 5,), SENT, device='cuda')
    y = rs(x, out=out)
    assert y.data_ptr() == out.data_ptr() and torch.equal(y, host) and bool((out[60000:] == SENT).all())
    with pytest.raises(ValueError):
        rs(x, out=torch.empty(59999, device='cuda'))
    with pytest.raises(ValueError):
        rs(x, out=np.empty(60000, np.float32))
    # the module function: cached per rate pair, the input itself at equal rates (channels averaged)
    assert torch.equal(audio.resample(x, 22050, 44100), host)
    assert audio._RESAMPLERS[(22050, 44100)] is not rs and audio.resample(x[:10], 22050, 44100).shape == (20,)
    n_cached = len(audio._RESAMPLERS)
    xd = torch.from_numpy(x).cuda()
    same = audio.resample(xd, 44100, 44100)
    assert same.data_ptr() == xd.data_ptr() and torch.equal(same, xd)
    assert np.array_equal(audio.resample(x, 44100, 44100).cpu().numpy(), x)
    st = np.stack([x, -0.5 * x], axis=1)
    assert np.array_equal(audio.resample(st, 44100, 44100).cpu().numpy(), (0.25 * x).astype(np.float32))
    assert len(audio._RESAMPLERS) == n_cached
    # a result is a song as the walk takes it
    p = Hyperparams(N=2048, window_size_note_time=1)
    lp = TranscriptionLoop(p, heads=('timing', 'pitch')).setup_device()
    ev_dev, _ = lp.run_songs([host], max_notes=1)
    ev_host, _ = lp.run_songs([host.cpu().numpy()], max_notes=1)
    assert ev_dev.shape[0] > 0 and torch.equal(ev_dev, ev_host)


@pytest.fixture(scope='module')
def clip48(tmp_path_factory):
    """A 3-window synthetic clip (1-s windows at 44.1 kHz) rendered at 48 kHz, two channels, as a FLAC file: (path,
    the [n, 2] waveform read back from it, its resampled mono signal on the host)."""
    from oracle import synth as osynth
    from amt_saga import audio, flac
    from amt_saga.hyperparams import Hyperparams
    p44 = Hyperparams(N=2048, window_size_note_time=1)
    assert p44.sr == 44100
    n48 = int(3.2 * p44.H * (p44.timing_frames - 1) * 160 / 147)
    notes_in = [(0, 60, 100, 0.2, 0.5), (0, 64, 90, 0.9, 0.4), (1, 67, 80, 1.6, 0.6), (2, 72, 110, 2.4, 0.3)]
    mono48 = osynth.render_window(notes_in, n48, 48000).numpy()
    path48 = str(tmp_path_factory.mktemp('clip48') / 'clip48.flac')
    flac.save_float(np.stack([mono48, 0.5 * mono48], axis=1), path48, 48000)
    wf48, sr = flac.load_float(path48)
    assert sr == 48000 and wf48.shape == (n48, 2)
    wf44 = audio.resample(wf48, 48000, 44100).cpu().numpy()
    assert wf44.shape == (rr.out_len(n48, 48000, 44100),)
    return path48, wf48, wf44


def test_transcription_at_the_model_rate(env, clip48):
    """A 48 kHz stereo file through transcribe(sr=48000) is the transcription of its resampled signal, in both
    traversals and as a (waveform, sr) item of the song queue."""
    from amt_saga import transcribe as tr
    from amt_saga.hyperparams import Hyperparams
    _, wf48, wf44 = clip48
    p44 = Hyperparams(N=2048, window_size_note_time=1)
    loop = tr._make_loop(p44, 2, ('timing', 'pitch', 'instrument', 'velocity'), (0, 1, 2), None, 'bank')
    notes_a, evs_a = tr.transcribe(wf48, p44, sr=48000, traversal='song', iters=2, loop=loop)
    notes_b, evs_b = tr.transcribe(wf44, p44, traversal='song', iters=2, loop=loop)
    assert evs_a.shape[0] > 0 and np.array_equal(evs_a, evs_b) and notes_a == notes_b
    notes_w, evs_w = tr.transcribe(wf48, p44, sr=48000, iters=2, loop=loop)
    notes_v, evs_v = tr.transcribe(wf44, p44, iters=2, loop=loop)
    assert np.array_equal(evs_w, evs_v) and notes_w == notes_v
    (q_notes, q_evs), (r_notes, r_evs) = tr.transcribe_songs([(wf48, 48000), wf44], p44, slots=2, iters=2, loop=loop)
    assert np.array_equal(q_evs[:, 1:], r_evs[:, 1:]) and len(q_notes) == len(r_notes) == len(notes_a)


def test_command_line_sr(env, clip48, tmp_path):
    """--sr in both modes of the command line; without it mixed rates are still refused."""
    from amt_saga import events, flac, transcribe as tr
    path48, _, wf44 = clip48
    mid = str(tmp_path / 'one.mid')
    tr.main([path48, mid, '--sr', '44100', '--iters', '1', '--traversal', 'song'])
    events.read_midi(mid)
    assert os.path.getsize(mid) > 20
    a44, b22 = str(tmp_path / 'a44.flac'), str(tmp_path / 'b22.flac')
    flac.save_float(wf44, a44, 44100)
    flac.save_float(wf44[:len(wf44) // 2], b22, 22050)
    out_dir = str(tmp_path / 'mid')
    tr.main(['--songs', a44, b22, '--out-dir', out_dir, '--sr', '44100', '--iters', '1'])
    for stem in ('a44', 'b22'):
        events.read_midi(os.path.join(out_dir, stem + '.mid'))
    with pytest.raises(SystemExit, match='sample rate'):
        tr.main(['--songs', a44, b22, '--out-dir', str(tmp_path / 'mid2')])
