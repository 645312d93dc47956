"""GPU: the WAV kernels (amt_pcm.hip) against the value rule restated in tests/wav_stream_writer.py, the writer against
wav.encode's bytes, and the command line on WAV input and output.  Bits and bytes only: nothing here has a tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wav_stream_writer as W                                      # noqa: E402
from oracle import synth as osynth                                 # noqa: E402

pytestmark = pytest.mark.gpu

SENT_OUT, SENT_PCM, SENT_BYTE = 0xDEADBEEF, 0x5EADBEEF, 0xAB
KINDS = {'int': 0, 'float': 1}


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import audio, wav, _lib
    return dict(torch=torch, audio=audio, wav=wav, _lib=_lib, lib=_lib.load())


@pytest.fixture(scope='module')
def corpus():
    return W.corpus()


def _bits(t):
    return t.contiguous().cpu().numpy().reshape(-1).view(np.uint32)


def _unpack(env, blob, rows, out_values, pcm=True):
    """amt_pcm_unpack_ragged called directly on `blob` and the table `rows`, both outputs prefilled with sentinels and
    followed by guard words.  Returns (out bits, pcm) on the host; the guards are asserted."""
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    guard = 64
    data = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    assert data.numel() == len(blob)
    sm = torch.tensor(rows, dtype=torch.int64).reshape(-1, 8).cuda()
    out = torch.full((out_values + guard,), SENT_OUT - (1 << 32), dtype=torch.int32).cuda()
    out_i = torch.full((out_values + guard,), SENT_PCM, dtype=torch.int32).cuda()
    from amt_saga.device import ptr, stream_ptr
    rc = lib.amt_pcm_unpack_ragged(ptr(data), data.numel(), ptr(sm), len(rows), min(max(max(r[1] for r in rows), 1), 4096),
                                   ptr(out), ptr(out_i) if pcm else None, out_values, stream_ptr())
    assert rc == _lib.AMT_OK
    torch.cuda.synchronize()
    o, p = out.cpu().numpy().view(np.uint32), out_i.cpu().numpy()
    assert np.all(o[out_values:] == SENT_OUT) and np.all(p[out_values:] == SENT_PCM)
    return o[:out_values], p[:out_values]


def _tables(files, lead=0, out_pad=1):
    """The files back to back after `lead` filler bytes: (blob, rows, out_values, expected out bits, expected pcm)."""
    blob, rows, out, pcm = bytearray(b'\xee' * lead), [], [], []
    base = 0
    for name, d, wv, q, (kind, c, b) in files:
        n, ch = wv.shape
        rows.append([len(blob) + W.data_offset(d), n, ch, KINDS[kind], c, b, base, 0])
        pad = -(n * ch) % out_pad
        out += [wv.reshape(-1).view(np.uint32), np.full(pad, SENT_OUT, np.uint32)]
        pcm += [q.reshape(-1) if q is not None else np.full(n * ch, SENT_PCM, np.int32), np.full(pad, SENT_PCM, np.int32)]
        base += n * ch + pad
        blob += d
    return bytes(blob), rows, base, np.concatenate(out), np.concatenate(pcm).astype(np.int32)


@pytest.mark.parametrize('lead', [0, 1, 2, 3])
def test_unpack_every_form_at_every_alignment(env, corpus, lead):
    """Every kind / container / valid-bits form with 1, 2, 3 and 8 channels and frame counts from 1 to past two tiles,
    all files in ONE launch, the whole buffer shifted by 0 .. 3 bytes; the last file's last sample ends on the buffer's
    last byte.  wave and pcm bit for bit; outputs laid both on 16-byte boundaries and back to back."""
    last = [e for e in corpus if W.data_offset(e[1]) + e[2].size * e[4][1] == len(e[1]) and e[4][1] > 1][-1]
    order = [e for e in corpus if e is not last] + [last]
    for out_pad in (4, 1):
        blob, rows, n_out, out, pcm = _tables(order, lead=lead, out_pad=out_pad)
        assert rows[-1][0] + rows[-1][1] * rows[-1][2] * rows[-1][4] == len(blob)
        got, got_pcm = _unpack(env, blob, rows, n_out)
        assert np.array_equal(got_pcm, pcm)
        bad = np.flatnonzero(got != out)
        assert bad.size == 0, (bad[:5], [r for r in rows if r[6] <= bad[0]][-1])
    # without out_pcm the waveform is the same
    got, got_pcm = _unpack(env, blob, rows, n_out, pcm=False)
    assert np.array_equal(got, out) and np.all(got_pcm == SENT_PCM)


def test_ragged_batch_of_seven_with_a_one_frame_file_in_the_middle(env, corpus):
    audio = env['audio']
    nm = len(W.FORMS) * len(W.CHANNELS)
    one = next(e for e in corpus[nm:] if e[2].shape[0] == 1 and e[4] == ('int', 3, 24))
    pick = [corpus[2], corpus[13], corpus[nm + 19], one, corpus[37], corpus[nm + 88], corpus[7]]
    assert len({e[4] for e in pick}) >= 5 and {e[2].shape[1] for e in pick} >= {1, 2, 3, 8}
    res = audio.wav_decode([e[1] for e in pick])
    assert len(res) == 7 and len({r[0].untyped_storage().data_ptr() for r in res}) == 1       # views of one buffer
    for (name, d, wv, q, (kind, c, b)), (wave, sr, bits) in zip(pick, res):
        n, ch = wv.shape
        assert tuple(wave.shape) == ((n,) if ch == 1 else (n, ch)) and bits == b and wave.is_cuda, name
        assert sr == env['wav'].read_header(d)[0]
        assert np.array_equal(_bits(wave), wv.reshape(-1).view(np.uint32)), name
    ints = [e for e in pick if e[3] is not None]
    for e, (wave, sr, bits, pcm) in zip(ints, audio.wav_decode([e[1] for e in ints], pcm=True)):
        assert pcm.dtype == env['torch'].int32 and np.array_equal(pcm.cpu().numpy().reshape(e[3].shape), e[3]), e[0]
        assert np.array_equal(_bits(wave), e[2].reshape(-1).view(np.uint32))
    # alone and inside the batch: the same bits
    alone = audio.wav_decode([pick[4][1]])[0][0]
    assert np.array_equal(_bits(alone), _bits(res[4][0]))


def test_a_table_row_that_points_outside_costs_only_its_own_output(env, corpus):
    nm = len(W.FORMS) * len(W.CHANNELS)
    few = [corpus[1], corpus[nm + 3], corpus[9]]
    blob, rows, n_out, out, pcm = _tables(few, lead=1, out_pad=4)
    nb, big = len(blob), 1 << 62
    bad = [[-1, 4, 1, 0, 2, 16, 0, 0], [nb - 7, 4, 1, 0, 2, 16, 0, 0], [nb, 1, 1, 0, 1, 8, 0, 0],
           [nb + 100, 4, 2, 0, 2, 16, 0, 0], [0, big, 1, 0, 1, 8, 0, 0], [0, big, 8, 1, 8, 64, 0, 0],
           [big, 4, 1, 0, 2, 16, 0, 0], [-big, 4, 1, 0, 2, 16, 0, 0], [0, 4, 1, 0, 2, 16, -1, 0],
           [0, 4, 1, 0, 2, 16, n_out - 3, 0], [0, 4, 1, 0, 2, 16, big, 0], [0, 4, 0, 0, 2, 16, 0, 0],
           [0, 4, 9, 0, 2, 16, 0, 0], [0, 4, 1, 0, 5, 16, 0, 0], [0, 4, 1, 0, 0, 16, 0, 0], [0, 4, 1, 0, 2, 17, 0, 0],
           [0, 4, 1, 0, 2, 0, 0, 0], [0, 4, 1, 1, 2, 16, 0, 0], [0, 4, 1, 7, 4, 32, 0, 0], [0, -4, 1, 0, 2, 16, 0, 0],
           [0, 0, 1, 0, 2, 16, 0, 0], [0, (1 << 61) + 1, 8, 0, 1, 8, 0, 0]]
    mixed = bad[:8] + rows[:1] + bad[8:15] + rows[1:2] + bad[15:] + rows[2:]
    got, got_pcm = _unpack(env, blob, mixed, n_out)
    assert np.array_equal(got, out) and np.array_equal(got_pcm, pcm)
    got, got_pcm = _unpack(env, blob, bad, n_out)
    assert np.all(got == SENT_OUT) and np.all(got_pcm == SENT_PCM)


def test_pack_bytes_equal_the_host_writer(env):
    """wav_encode == wav.encode == the stated layout for all three formats, with and without norm, over lengths 1, odd,
    even and past a tile, all signals in one call; inputs hold NaN, infinities, +-1 and beyond, half-way cases."""
    torch, audio, wav = env['torch'], env['audio'], env['wav']
    sigs = W.pack_signals()
    dev = [torch.from_numpy(s).cuda() for s in sigs]
    for fmt in wav.FORMATS:
        for norm in (False, True):
            files = audio.wav_encode(dev, 48000, fmt=fmt, norm=norm)
            assert len(files) == len(sigs)
            for y, data in zip(sigs, files):
                assert data == W.expect_file(y, 48000, fmt, norm), (fmt, norm, len(y))
                assert data == wav.encode(wav.normalise(y) if norm else y, 48000, fmt)
    # rows of a [G, n] tensor are signals; a signal alone gives the same bytes as inside the batch
    grid = torch.from_numpy(np.stack([sigs[5], sigs[5][::-1].copy()])).cuda()
    two = audio.wav_encode(grid, 8000)
    assert two[0] == W.expect_file(sigs[5], 8000, 'pcm24') and two[1] == W.expect_file(sigs[5][::-1], 8000, 'pcm24')
    assert audio.wav_encode([dev[6]], 48000, 'pcm16', norm=True)[0] == W.expect_file(sigs[6], 48000, 'pcm16', True)


def test_peak_and_pack_called_directly_keep_inside_their_buffers(env):
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    from amt_saga.device import ptr, stream_ptr
    sigs = W.pack_signals()
    lens = [len(s) for s in sigs]
    wave = torch.from_numpy(np.concatenate(sigs)).cuda()
    base = np.concatenate([[0], np.cumsum(lens)[:-1]])
    n = len(sigs)
    meta = torch.tensor(np.stack([base, lens]), dtype=torch.int64).cuda()
    peaks = torch.full((n + 4,), -7.0).cuda()
    assert lib.amt_pcm_peak_ragged(ptr(wave), ptr(meta[0]), ptr(meta[1]), n, max(lens), ptr(peaks), stream_ptr()) == 0
    want = []
    for s in sigs:
        a = np.abs(s)[~np.isnan(s)]
        want.append(np.float32(a.max() if a.size else 0))
    got = peaks.cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint32), np.array(want, np.float32).view(np.uint32)) and np.all(got[n:] == -7.0)
    # pack at odd output bases; a signal whose bytes would pass the buffer, and one at a negative base, write nothing
    for fmt_id, fmt in enumerate(env['wav'].FORMATS):
        c = env['wav'].FORMAT_BYTES[fmt]
        ob, total = [], 1
        for l in lens:
            ob.append(total)
            total += l * c + 3
        size = ob[-1] + lens[-1] * c - 1                                    # the last signal passes the end by one byte
        ob2 = list(ob)
        ob2[0] = -1
        out = torch.full((size + 64,), SENT_BYTE, dtype=torch.uint8).cuda()
        obd = torch.tensor(ob2, dtype=torch.int64).cuda()
        assert lib.amt_pcm_pack_ragged(ptr(wave), ptr(meta[0]), ptr(meta[1]), n, max(lens), fmt_id, None, ptr(out), ptr(obd),
                                       size, stream_ptr()) == 0
        got = out.cpu().numpy()
        want = np.full(size + 64, SENT_BYTE, np.uint8)
        for i in range(1, n - 1):
            body = W.expect_file(sigs[i], 8000, fmt)[58 if fmt == 'float32' else 44:][:lens[i] * c]
            want[ob[i]:ob[i] + len(body)] = np.frombuffer(body, np.uint8)
        assert np.array_equal(got, want), fmt


def test_cross_container_and_load_audio(env, tmp_path):
    """One signal through flac_encode -> flac_decode and through wav_encode('pcm24') -> wav_decode: the same tensor, bit
    for bit.  load_audio of a mixed list (FLAC, WAV, FLAC) returns input order and equals the separate calls."""
    torch, audio = env['torch'], env['audio']
    rng = np.random.default_rng(11)
    y = (rng.standard_normal(5000) * 0.3).astype(np.float32)
    y[:6] = [1.0, -1.0, 2.0, np.nan, 0.5 * 2.0 ** -23, 1.5 * 2.0 ** -23]
    yd = torch.from_numpy(y).cuda()
    f = audio.flac_encode([yd], 44100)[0]
    w = audio.wav_encode([yd], 44100, 'pcm24')[0]
    (fw, fsr, fb), (ww, wsr, wb) = audio.flac_decode([f])[0], audio.wav_decode([w])[0]
    assert (fsr, fb) == (wsr, wb) == (44100, 24) and np.array_equal(_bits(fw), _bits(ww))
    assert np.array_equal(ww.cpu().numpy(), W.quantise(y, 24).astype(np.float32) * np.float32(2.0 ** -23))
    y2 = (rng.standard_normal(777) * 0.2).astype(np.float32)
    f2 = audio.flac_encode([torch.from_numpy(y2).cuda()], 22050, bps=16)[0]
    st = W.write(W.values('int', 2, 16, 301, 2, 5), c=2, sr=48000)
    paths = [str(tmp_path / n) for n in ('a.flac', 'b.wav', 'c.flac', 'd.wav')]
    for p, d in zip(paths, (f, w, f2, st)):
        open(p, 'wb').write(d)
    got = audio.load_audio(paths[:3])
    fl, wv = audio.load_flac([paths[0], paths[2]]), audio.load_wav(paths[1])
    for g, want in zip(got, (fl[0], wv, fl[1])):
        assert g[1:] == want[1:] and np.array_equal(_bits(g[0]), _bits(want[0]))
    assert [g[1] for g in got] == [44100, 44100, 22050]
    one = audio.load_audio(paths[3])
    assert tuple(one[0].shape) == (301, 2) and one[1:] == (48000, 16)
    assert np.array_equal(_bits(one[0]), _bits(audio.load_wav([paths[3]])[0][0]))


def test_audio_complete_save_writes_a_peak_normalised_float_wav(env, tmp_path):
    audio, wav = env['audio'], env['wav']
    rng = np.random.default_rng(2)
    y = (rng.standard_normal(3000) * 0.2).astype(np.float32)
    ac = audio.audio_complete(y, 1024, sample_rate=22050)
    p = str(tmp_path / 'ac.wav')
    ac.save(p, flac=False)
    data = open(p, 'rb').read()
    sr, ch, kind, bits, c, off, n = wav.read_header(data)
    assert (sr, ch, kind, bits, n) == (22050, 1, 'float', 32, len(y)) and off == 58
    wf = np.asarray(ac.wf, dtype=np.float32)
    x = wav.decode(data)[0][:, 0]
    assert np.array_equal(x, wf / np.abs(wf).max()) and np.abs(x).max() == 1.0
    assert data == W.expect_file(wf, 22050, 'float32', norm=True)
    pf = str(tmp_path / 'ac.flac')
    ac.save(pf)                                                           # flac=True is untouched
    assert open(pf, 'rb').read(4) == b'fLaC'


@pytest.mark.parametrize('cli', ['one_file', 'songs'])
def test_command_line_reads_wav_as_it_reads_flac_and_writes_wav(env, tmp_path, monkeypatch, cli):
    """A short mono song saved as FLAC and as PCM-24 WAV gives byte-identical .mid files in the one-file mode (both files
    through both readers) and with --songs (one group that mixes the two) for --decode host and --decode device;
    --format wav with --residual-dir and --stems-dir writes files that wav.decode reads back to the tensors the walk
    kept, quantised to 24 bits."""
    from amt_saga import flac, transcribe as tr, wav
    from amt_saga.hyperparams import Hyperparams
    p = Hyperparams(N=2048, window_size_note_time=1)
    n = int(1.4 * p.H * (p.timing_frames - 1))
    notes_in = [(j % 3, 60 + 2 * j, 100, 0.2 + 0.7 * j, 0.4) for j in range(int(n / p.sr / 0.7))]
    y = osynth.render_window(notes_in, n, p.sr).numpy()
    pf, pw = str(tmp_path / 'song_f.flac'), str(tmp_path / 'song_w.wav')
    flac.save_float(y, pf, p.sr)
    wav.save_float(y, pw, p.sr, fmt='pcm24')
    assert np.array_equal(flac.load_float(pf)[0], wav.load_float(pw)[0])
    if cli == 'one_file':
        mids = []
        for k, (path, mode) in enumerate(((pf, 'host'), (pw, 'host'), (pf, 'device'), (pw, 'device'))):
            one = str(tmp_path / ('one_%d.mid' % k))
            tr.main([path, one, '--iters', '1', '--decode', mode])
            mids.append(open(one, 'rb').read())
        assert len(mids[0]) > 20 and all(m == mids[0] for m in mids)
        return
    kept = []
    real = tr.write_song_audio

    def spy(rate, **kw):
        kept.append((rate, kw))
        return real(rate, **kw)
    monkeypatch.setattr(tr, 'write_song_audio', spy)
    song_mids = []
    for mode in tr.DECODERS:
        out_dir = str(tmp_path / ('mid_' + mode))
        extra = ['--format', 'wav', '--residual-dir', str(tmp_path / 'res'), '--stems-dir', str(tmp_path / 'stems'),
                 '--flac', 'device'] if mode == 'device' else []
        kept.clear()
        tr.main(['--songs', pf, pw, '--out-dir', out_dir, '--slots', '2', '--iters', '1', '--decode', mode] + extra)
        song_mids += [open(os.path.join(out_dir, s + '.mid'), 'rb').read() for s in ('song_f', 'song_w')]
    assert len(song_mids[0]) > 20 and all(m == song_mids[0] for m in song_mids)
    assert len(kept) == 2
    for rate, kw in kept:
        name = kw['name']
        assert rate == p.sr and kw['format'] == 'wav' and kw['residual_path'].endswith(name + '.residual.wav')
        files = [(kw['residual_path'], kw['residual'])]
        files += [(os.path.join(str(tmp_path / 'stems'), '%s.group%d.wav' % (name, g)), row)
                  for g, row in zip(tr.CLI_GROUPS, kw['stems'])]
        for path, t in files:
            data = open(path, 'rb').read()
            x, sr, bits = wav.decode(data)
            assert (sr, bits) == (p.sr, 24) and wav.read_header(data)[4] == 3
            assert np.array_equal(x[:, 0], W.quantise(t.cpu().numpy(), 24)), path
    assert sorted(os.listdir(str(tmp_path / 'stems'))) == sorted('%s.group%d.wav' % (s, g) for s in ('song_f', 'song_w')
                                                                 for g in tr.CLI_GROUPS)
