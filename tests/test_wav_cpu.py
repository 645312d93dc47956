"""CPU: WAV input and output without a GPU.  The chunk walk accepts the whole matrix of the test writer and refuses every
unsupported or damaged file with a ValueError; the numpy reader follows the value rule (and agrees with the standard
library's `wave` where that reads the file); the writer's bytes are the stated layout; the core the kernels compile
(csrc/amt_pcm_core.h) reproduces every bit and touches nothing outside its buffers in a stand-alone program built with
the address and undefined-behaviour sanitizers; the ABI, the Python entry points and the command line refuse bad
arguments before a GPU is touched."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import wave

import numpy as np
import pytest

import wav_stream_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def corpus():
    return W.corpus()


def test_header_over_the_writer_matrix(corpus):
    from amt_saga import audio, wav
    assert wav.MAX_CHANNELS == audio.Resampler.MAX_CHANNELS and audio.PCM_TILE == W.TILE
    assert len(corpus) == len(W.FORMS) * (len(W.CHANNELS) + len(W.FRAMES))
    for name, data, wv, pcm, (kind, c, b) in corpus:
        sr, ch, k, bits, cb, off, n = wav.read_header(data)
        assert (ch, k, bits, cb, n) == (wv.shape[1], kind, b, c, wv.shape[0]), name
        assert off == W.data_offset(data) and sr in (8000, 44100, 48000, 96000), name
    x = np.arange(-6, 6).reshape(6, 2)
    # streaming writers' placeholders and a truncated file: the size is clamped to what is there, then to whole frames
    for size in (0, 0xFFFFFFFF, 24 + 7):
        assert wav.read_header(W.write(x, c=2, data_size=size))[6] == 6
    assert wav.read_header(W.write(x, c=2)[:-5])[6] == 4
    assert wav.read_header(W.write(x, c=2, data_size=9))[6] == 2
    # EXTENSIBLE with wValidBitsPerSample 0 means the container's width
    assert wav.read_header(W.write(x, c=3, b=24, fmt_size=40, valid_field=0))[3] == 24


def test_header_refusals_are_value_errors_with_their_reason():
    from amt_saga import wav
    x = np.arange(-6, 6).reshape(6, 2)
    good = W.write(x, c=2)
    cases = [(W.write(x, magic=b'RIFX'), 'RIFX'), (W.write(x, magic=b'RF64'), 'RF64'),
             (W.write(x, tag=6, c=1), r'0x0006 \(A-law\)'), (W.write(x, tag=7, c=1), r'0x0007 \(mu-law\)'),
             (W.write(x, tag=2, c=1), 'MS ADPCM'), (W.write(x, tag=0x55, c=1, fmt_size=40), '0x0055'),
             (W.write(x, c=2, block_align=5), 'block align 5 does not divide'),
             (W.write(x, c=2, block_align=0), 'block align 0'),
             (W.write(np.zeros((4, 9), int), c=2), '9 channels'),
             (W.write(np.zeros((0, 2), int), c=2), 'without a whole sample frame'),
             (W.write(x, c=2)[:W.data_offset(good) + 3], 'without a whole sample frame'),
             (W.write(x, c=2, fmt=False), 'without a fmt chunk'),
             (W.write(x, c=2, block_align=10), 'samples of 5 bytes'),
             (W.write(x, kind='float', c=4, block_align=4), 'float samples of 2 bytes'),
             (W.write(x, c=2, b=17), '17 valid bits'), (W.write(x, c=2, b=16, fmt_size=40, valid_field=20), '20 valid bits'),
             (W.write(x, form=b'AVI '), 'not WAVE'), (b'fLaC' + bytes(60), 'not a WAV file'), (b'', 'not a WAV file'),
             (good[:12] + W.chunk(b'fmt ', bytes(14)) + good[36:], 'fmt chunk of 14 bytes'),
             (W.write(x, c=2, sr=0), 'sample rate 0')]
    for data, reason in cases:
        with pytest.raises(ValueError, match=reason):
            wav.read_header(data)
    # truncations at every byte of a 60-byte file, and of one with junk chunks and an EXTENSIBLE fmt: ValueError or a
    # header that stays inside what is left -- never another exception
    small = W.write(np.arange(8), c=2)
    assert len(small) == 60
    big = W.write(np.arange(5), c=3, b=20, fmt_size=40, before=[(b'LIST', b'abc')], between=[(b'fact', bytes(4))])
    for data in (small, big):
        for cut in range(len(data)):
            try:
                sr, ch, kind, bits, c, off, n = wav.read_header(data[:cut])
            except ValueError:
                continue
            assert n >= 1 and off + n * ch * c <= cut, cut
    # random damage: any byte string is refused with ValueError or described inside its bounds
    rng = np.random.default_rng(3)
    for _ in range(300):
        d = bytearray(big)
        for p in rng.integers(0, len(d), 3):
            d[p] = rng.integers(0, 256)
        try:
            sr, ch, kind, bits, c, off, n = wav.read_header(bytes(d))
        except ValueError:
            continue
        assert off + n * ch * c <= len(d)


def test_reader_follows_the_value_rule_and_agrees_with_the_wave_module(corpus):
    from amt_saga import wav
    seen = set()
    for name, data, wv, pcm, (kind, c, b) in corpus:
        x, sr, bits = wav.decode(data)
        assert bits == b and x.shape == wv.shape, name
        got = wav.to_wave(x, kind, bits)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), wv.view(np.uint32)), name
        if kind == 'int':
            assert x.dtype == np.int32 and np.array_equal(x, pcm), name
        if kind == 'int' and b == 8 * c:                                  # plain PCM: the standard library reads it
            w = wave.open(io.BytesIO(data))
            assert (w.getnchannels(), w.getsampwidth(), w.getnframes()) == (wv.shape[1], c, wv.shape[0]), name
            raw = np.frombuffer(w.readframes(w.getnframes()), np.uint8).reshape(-1, c).astype(np.int64)
            v = sum(raw[:, i] << (8 * i) for i in range(c))
            v = v - 128 if c == 1 else (v ^ (1 << (8 * c - 1))) - (1 << (8 * c - 1))
            assert np.array_equal(v.reshape(wv.shape), pcm), name
            seen.add(c)
    assert seen == {1, 2, 3, 4}
    # the extremes by hand: 0 / 255, +-full scale, int32 values that round in float32, 24-in-32 and 20-in-24, low bits
    assert wav.decode(W.write(np.array([-128, 127]), c=1))[0][:, 0].tolist() == [-128, 127]
    assert W.containers(np.array([[-128], [127]]), 'int', 1, 8) == b'\x00\xff'
    y = wav.to_wave(wav.decode(W.write(np.array([-(1 << 31), (1 << 31) - 1, (1 << 24) + 1, (1 << 24) + 3]), c=4))[0], 'int', 32)
    assert y[:, 0].tolist() == [-1.0, 1.0, 2.0 ** -7, 2.0 ** -7 + 2.0 ** -29]  # to even: 2^24 + 1 down, 2^24 + 3 up
    for c, b in ((4, 24), (3, 20)):
        q = np.array([-(1 << (b - 1)), (1 << (b - 1)) - 1, -1, 5])
        x, _, bits = wav.decode(W.write(q, c=c, b=b, fmt_size=40, low=0xffffffff))
        assert bits == b and x[:, 0].tolist() == q.tolist()
    f = np.array([0x7fc12345, 0x80000000, 0xff800001], np.uint32).view(np.float32)
    x, _, bits = wav.decode(W.write(f, kind='float', c=4))
    assert bits == 32 and x.view(np.uint32)[:, 0].tolist() == [0x7fc12345, 0x80000000, 0xff800001]
    x, _, bits = wav.decode(W.write(np.array([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -0.0]), kind='float', c=8))
    assert bits == 64 and x[:, 0].tolist() == [1.0, 1.0 + 2.0 ** -22, 0.0] and np.signbit(x[2, 0])


def test_load_float_has_the_shape_and_meaning_of_the_flac_reader(tmp_path):
    from amt_saga import flac, wav
    rng = np.random.default_rng(0)
    q = rng.integers(-(1 << 23), 1 << 23, (50, 2))
    for x in (q, q[:, 0]):
        pw, pf = str(tmp_path / 'a.wav'), str(tmp_path / 'a.flac')
        with open(pw, 'wb') as f:
            f.write(W.write(x, c=3, sr=22050))
        flac.encode(x, pf, sr=22050, bps=24)
        (yw, srw), (yf, srf) = wav.load_float(pw), flac.load_float(pf)
        assert srw == srf == 22050 and yw.dtype == yf.dtype == np.float64 and yw.shape == yf.shape == x.shape
        assert np.array_equal(yw, yf)
        assert wav.is_wav(pw) and not wav.is_wav(pf)


def test_writer_bytes_are_the_stated_layout_and_read_back():
    from amt_saga import wav
    sigs = W.pack_signals()
    assert {len(s) & 1 for s in sigs} == {0, 1}
    for y in sigs:
        for fmt in wav.FORMATS:
            data = wav.encode(y, 48000, fmt)
            assert data == W.expect_file(y, 48000, fmt), (len(y), fmt)
            assert len(data) % 2 == 0 and len(data) == (58 if fmt == 'float32' else 44) + -(-len(y) * wav.FORMAT_BYTES[fmt] // 2) * 2
            x, sr, bits = wav.decode(data)
            assert sr == 48000 and x.shape == (len(y), 1)
            if fmt == 'float32':
                assert np.array_equal(x[:, 0].view(np.uint32), y.view(np.uint32))
                continue
            q = W.quantise(y, bits)
            assert np.array_equal(x[:, 0], q)
            w = wave.open(io.BytesIO(data))                               # the standard library reads the same samples
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, bits // 8, 48000, len(y))
            raw = np.frombuffer(w.readframes(len(y)), np.uint8).reshape(-1, bits // 8).astype(np.int64)
            v = sum(raw[:, i] << (8 * i) for i in range(bits // 8))
            assert np.array_equal((v ^ (1 << (bits - 1))) - (1 << (bits - 1)), q)
            assert wav.encode(x[:, 0], 48000, fmt) == data                # encode . decode = identity on quantised input
            assert wav.encode(wav.to_wave(x[:, 0], 'int', bits), 48000, fmt) == data
    assert wav.quantise([0.5 * 2.0 ** -15, 1.5 * 2.0 ** -15, -2.5 * 2.0 ** -15, 1.0, -2.0, np.nan, np.inf], 16).tolist() == \
        [0, 2, -2, 32767, -32768, 0, 32767]
    for y, want in ((np.array([0.25, -0.5], np.float32), [0.5, -1.0]), (np.array([np.nan, 0.0], np.float32), None),
                    (np.array([np.inf, 1.0], np.float32), None)):
        got = wav.normalise(y)
        assert np.array_equal(got.view(np.uint32), (y if want is None else np.array(want, np.float32)).view(np.uint32))
        assert wav.encode(wav.normalise(y), 8000, 'float32') == W.expect_file(y, 8000, 'float32', norm=True)
    with pytest.raises(ValueError, match='2\\^32 - 64'):
        wav.header((1 << 32) // 3, 44100, 'pcm24')
    assert len(wav.header(((1 << 32) - 64) // 3 - 1, 44100, 'pcm24')) == 44
    with pytest.raises(ValueError, match='fmt must be one of'):
        wav.encode(sigs[0], 44100, 'pcm8')
    with pytest.raises(ValueError, match='sample rate'):
        wav.encode(sigs[0], 0, 'pcm16')
    with pytest.raises(ValueError, match='a mono signal'):
        wav.encode(np.zeros((4, 2), np.float32), 44100, 'pcm16')


def test_save_float_writes_what_encode_returns(tmp_path):
    from amt_saga import wav
    y = W.pack_signals()[3]
    p = str(tmp_path / 'y.wav')
    wav.save_float(y.astype(np.float64), p, sr=32000)
    assert open(p, 'rb').read() == W.expect_file(y, 32000, 'pcm24')
    got, sr = wav.load_float(p)
    assert sr == 32000 and np.array_equal(got, W.quantise(y, 24) / 2.0 ** 23)
    # the drop-in audio_from_file reads it as it reads a FLAC file: float32, mono (a stereo file is mixed down)
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'amt-saga_amd', 'dropin'))
    import util_audio as ua
    back, sr = ua.audio_from_file(p)
    assert sr == 32000 and back.dtype == np.float32 and np.array_equal(back, got.astype(np.float32))
    q = np.arange(-20, 20).reshape(20, 2) << 8
    with open(p, 'wb') as f:
        f.write(W.write(q, c=3, sr=8000))
    back, sr = ua.audio_from_file(p)
    assert sr == 8000 and back.shape == (20,) and np.array_equal(back, (q.mean(axis=1) / 2.0 ** 23).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------
# the core of the kernels in a sanitised stand-alone program
# ---------------------------------------------------------------------------------------------------------------
SENT_OUT, SENT_PCM, SENT_BYTE = 0xDEADBEEF, 0x5EADBEEF, 0xAB
KINDS = {'int': 0, 'float': 1}


def row_values(row, data_bytes, out_values):
    """The clamp restated: frames * channels if the row is a known geometry and lies inside both buffers, else 0."""
    off, frames, ch, kind, c, bits, ob = row[:7]
    ok = frames > 0 and 1 <= ch <= 8 and ((kind == 0 and 1 <= c <= 4 and 1 <= bits <= 8 * c) or (kind == 1 and c in (4, 8)))
    if not ok:
        return 0
    v = frames * ch
    return v if off >= 0 and off + v * c <= data_bytes and ob >= 0 and ob + v <= out_values else 0


def batch_tables(files, out_pad=0):
    """(data, rows, out_values, expected out bits, expected pcm) for corpus entries laid back to back."""
    data, rows, out, pcm = b'', [], [], []
    base = 0
    for name, d, wv, q, (kind, c, b) in files:
        n, ch = wv.shape
        rows.append([len(data) + W.data_offset(d), n, ch, KINDS[kind], c, b, base, 0])
        out.append(wv.reshape(-1).view(np.uint32))
        pcm.append(q.reshape(-1) if q is not None else np.full(n * ch, SENT_PCM, np.int32))
        pad = out_pad and -(n * ch) % out_pad
        if pad:
            out.append(np.full(pad, SENT_OUT, np.uint32))
            pcm.append(np.full(pad, SENT_PCM, np.int32))
        base += n * ch + pad
        data += d
    return data, rows, base, np.concatenate(out), np.concatenate(pcm).astype(np.int32)


def bad_rows(data_bytes, out_values):
    """Table rows that point before, across and past either buffer, or describe no known geometry."""
    big = 1 << 62
    return [[-1, 4, 1, 0, 2, 16, 0, 0], [data_bytes - 7, 4, 1, 0, 2, 16, 0, 0], [data_bytes, 1, 1, 0, 1, 8, 0, 0],
            [data_bytes + 100, 4, 2, 0, 2, 16, 0, 0], [0, big, 1, 0, 1, 8, 0, 0], [0, big, 8, 1, 8, 64, 0, 0],
            [big, 4, 1, 0, 2, 16, 0, 0], [-big, 4, 1, 0, 2, 16, 0, 0], [0, 4, 1, 0, 2, 16, -1, 0],
            [0, 4, 1, 0, 2, 16, out_values - 3, 0], [0, 4, 1, 0, 2, 16, big, 0], [0, 4, 0, 0, 2, 16, 0, 0],
            [0, 4, 9, 0, 2, 16, 0, 0], [0, 4, 1, 0, 5, 16, 0, 0], [0, 4, 1, 0, 0, 16, 0, 0], [0, 4, 1, 0, 2, 17, 0, 0],
            [0, 4, 1, 0, 2, 0, 0, 0], [0, 4, 1, 1, 2, 16, 0, 0], [0, 4, 1, 7, 4, 32, 0, 0], [0, -4, 1, 0, 2, 16, 0, 0],
            [0, 0, 1, 0, 2, 16, 0, 0], [0, (1 << 61) + 1, 8, 0, 1, 8, 0, 0]]


def test_core_in_a_sanitised_stand_alone_program(corpus, tmp_path):
    """amt_pcm_core.h, host only, under the address and undefined-behaviour sanitizers: every file of the corpus bit for
    bit at all four alignments with the buffer ending on its allocation's last byte, tables that point outside costing
    only their own output, the writer's bytes for all three formats -- and no sanitizer report (a report aborts the
    program: a nonzero exit)."""
    from amt_saga import wav
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'pcm_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'pcm_host_main.cpp'), '-o', exe], check=True)
    cases = []

    def unpack_case(data, rows, out_values, out, pcm, with_pcm=1):
        assert len(out) == len(pcm) == out_values
        return (struct.pack('<iq', 0, len(data)) + data + struct.pack('<i', len(rows))
                + np.asarray(rows, '<i8').tobytes() + struct.pack('<qi', out_values, with_pcm)
                + out.astype('<u4').tobytes() + pcm.astype('<i4').tobytes())
    # the whole corpus in one table (the last file ends on the buffer's last byte), and file by file
    last = [e for e in corpus if W.data_offset(e[1]) + e[2].size * e[4][1] == len(e[1]) and e[4][1] > 1][-1]
    order = [e for e in corpus if e is not last] + [last]
    data, rows, n_out, out, pcm = batch_tables(order, out_pad=4)
    assert rows[-1][0] + rows[-1][1] * rows[-1][2] * rows[-1][4] == len(data)
    cases.append(unpack_case(data, rows, n_out, out, pcm))
    assert {r[0] % 4 for r in rows if r[4] in (2, 3, 4, 8)} == {0, 1, 2, 3}
    for e in corpus[::7]:
        cases.append(unpack_case(*batch_tables([e])))
    # tables that point outside: the rows around them stay exact, everything else keeps the sentinel
    few = [corpus[1], corpus[len(W.FORMS) * len(W.CHANNELS) + 3], corpus[9]]
    data, rows, n_out, out, pcm = batch_tables(few, out_pad=4)
    bad = bad_rows(len(data), n_out)
    assert all(row_values(r, len(data), n_out) == 0 for r in bad)
    assert all(row_values(r, len(data), n_out) == r[1] * r[2] for r in rows)
    mixed = bad[:8] + rows[:1] + bad[8:15] + rows[1:2] + bad[15:] + rows[2:]
    cases.append(unpack_case(data, mixed, n_out, out, pcm))
    cases.append(unpack_case(data, bad, n_out, np.full(n_out, SENT_OUT, np.uint32), np.full(n_out, SENT_PCM, np.int32)))
    cases.append(unpack_case(b'', rows, 0, np.zeros(0, np.uint32), np.zeros(0, np.int32)))
    n_unpack = len(cases)
    # the writer: every signal in every format with and without a peak, into a buffer it exactly fills, one it would
    # pass by a byte, and at a negative base
    for y in W.pack_signals():
        for fmt_id, fmt in enumerate(wav.FORMATS):
            for norm in (False, True):
                c = wav.FORMAT_BYTES[fmt]
                body = W.expect_file(y, 8000, fmt, norm)[58 if fmt == 'float32' else 44:][:len(y) * c]
                a = np.abs(y)[~np.isnan(y)]
                peak = np.float32(a.max() if a.size else 0)
                for base, size in ((3, 3 + len(body)), (3, 2 + len(body)), (-1, len(body) + 8)):
                    want = bytearray([SENT_BYTE]) * size
                    if base >= 0 and base + len(body) <= size:
                        want[base:base + len(body)] = body
                    cases.append(struct.pack('<iq', 1, len(y)) + y.astype('<f4').tobytes()
                                 + struct.pack('<iiIqq', fmt_id, int(norm), int(peak.view(np.uint32)), base, size)
                                 + bytes(want))
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        f.write(b'PCMC' + struct.pack('<i', len(cases)) + b''.join(cases))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('-> ok') == len(cases) and 'runtime error' not in r.stderr
    assert r.stdout.count(' unpack ') == n_unpack


# ---------------------------------------------------------------------------------------------------------------
# ABI, Python entry points, command line
# ---------------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_arguments_before_any_hip_call():
    from amt_saga import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                                        # never dereferenced: checks come first

    def unpack(**kw):
        a = dict(data=p, data_bytes=10, sm=p, n=1, max_frames=4, out=p, pcm=None, out_values=16)
        a.update(kw)
        return lib.amt_pcm_unpack_ragged(a['data'], a['data_bytes'], a['sm'], a['n'], a['max_frames'], a['out'], a['pcm'],
                                         a['out_values'], None)

    def peak(**kw):
        a = dict(wave=p, base=p, len=p, n=1, max_len=4, out=p)
        a.update(kw)
        return lib.amt_pcm_peak_ragged(a['wave'], a['base'], a['len'], a['n'], a['max_len'], a['out'], None)

    def pack(**kw):
        a = dict(wave=p, base=p, len=p, n=1, max_len=4, fmt=1, peak=None, out=p, out_base=p, out_bytes=16)
        a.update(kw)
        return lib.amt_pcm_pack_ragged(a['wave'], a['base'], a['len'], a['n'], a['max_len'], a['fmt'], a['peak'], a['out'],
                                       a['out_base'], a['out_bytes'], None)
    for k in ('data', 'sm', 'out'):
        assert unpack(**{k: None}) == _lib.AMT_E_INVALID, k
    for k in ('wave', 'base', 'len', 'out'):
        assert peak(**{k: None}) == _lib.AMT_E_INVALID, k
    for k in ('wave', 'base', 'len', 'out', 'out_base'):
        assert pack(**{k: None}) == _lib.AMT_E_INVALID, k
    for n in (0, -1, 65536):
        assert unpack(n=n) == peak(n=n) == pack(n=n) == _lib.AMT_E_INVALID, n
    for kw in (dict(data_bytes=-1), dict(max_frames=-1), dict(out_values=-1)):
        assert unpack(**kw) == _lib.AMT_E_INVALID, kw
    assert peak(max_len=-1) == _lib.AMT_E_INVALID
    for kw in (dict(max_len=-1), dict(out_bytes=-1), dict(fmt=3), dict(fmt=-1)):
        assert pack(**kw) == _lib.AMT_E_INVALID, kw
    assert lib.amt_version() == 1


def test_python_refuses_bad_arguments_before_the_gpu(tmp_path):
    from amt_saga import audio
    good = W.write(np.arange(8), c=2)
    with pytest.raises(ValueError, match='a list of bytes'):
        audio.wav_decode(good)
    with pytest.raises(ValueError, match='a list of bytes'):
        audio.wav_decode(['name.wav'])
    with pytest.raises(ValueError, match='at least one file'):
        audio.wav_decode([])
    with pytest.raises(ValueError, match='RIFX'):
        audio.wav_decode([good, W.write(np.arange(8), magic=b'RIFX')])
    with pytest.raises(ValueError, match='A-law'):
        audio.wav_decode([W.write(np.arange(8), tag=6, c=1)])
    with pytest.raises(ValueError, match='invalid argument'):                      # AMT_E_INVALID: pcm of a float file
        audio.wav_decode([good, W.write(np.zeros(4, np.float32), kind='float', c=4)], pcm=True)
    with pytest.raises(FileNotFoundError):
        audio.load_wav([str(tmp_path / 'missing.wav')])
    with pytest.raises(FileNotFoundError):
        audio.load_audio(str(tmp_path / 'missing.wav'))
    p = str(tmp_path / 'x.ogg')
    with open(p, 'wb') as f:
        f.write(b'OggS' + bytes(100))
    with pytest.raises(ValueError, match='not a FLAC file'):
        audio.load_audio([p])
    with pytest.raises(ValueError, match='fmt must be one of'):
        audio.wav_encode([], 44100, fmt='pcm32')
    with pytest.raises(ValueError, match='float32 device tensors'):
        audio.wav_encode([np.zeros(4, np.float32)], 44100)


def test_format_option_parses_and_riff_files_reach_the_wav_reader(tmp_path, capsys, monkeypatch):
    from amt_saga import transcribe as tr, wav
    assert tr.FORMATS == ('flac', 'wav') and tr.DECODERS == ('host', 'device') and tr.FLAC_WRITERS == ('host', 'device')
    missing = str(tmp_path / 'missing.wav')
    for fmt in tr.FORMATS:                                                         # accepted: the file is what fails
        with pytest.raises(FileNotFoundError):
            tr.main([missing, str(tmp_path / 'o.mid'), '--format', fmt])
        with pytest.raises(FileNotFoundError):
            tr.main(['--songs', missing, '--out-dir', str(tmp_path / 'o'), '--format', fmt])
    for argv in ([missing, str(tmp_path / 'o.mid'), '--format', 'mp3'],
                 ['--songs', missing, '--out-dir', str(tmp_path / 'o'), '--format', 'mp3']):
        with pytest.raises(SystemExit):
            tr.main(argv)
    assert 'invalid choice' in capsys.readouterr().err
    with pytest.raises(ValueError, match='Requested attribute does not exist'):
        tr.write_song_audio(44100, residual=None, format='ogg')
    # a RIFF file goes to the WAV reader in both --decode modes and both command-line modes
    song = str(tmp_path / 'song.wav')
    y = (np.sin(np.arange(4000) * 0.05) * 0.3).astype(np.float32)
    wav.save_float(y, song, sr=16000)
    calls = []
    real = wav.load_float

    def load_float(path):
        calls.append(path)
        return real(path)
    monkeypatch.setattr(wav, 'load_float', load_float)
    import torch
    if not torch.cuda.is_available():
        # without a GPU the host mode gets as far as the model (RuntimeError), not a FLAC error
        for argv in ([song, str(tmp_path / 'o.mid')], ['--songs', song, '--out-dir', str(tmp_path / 'o')]):
            with pytest.raises(RuntimeError):
                tr.main(argv)
        assert calls == [song, song]

    class Reached(Exception):
        pass

    def load_audio(paths, verify=True):
        raise Reached(paths)
    from amt_saga import audio
    monkeypatch.setattr(audio, 'load_audio', load_audio)
    with pytest.raises(Reached):
        tr.main([song, str(tmp_path / 'o.mid'), '--decode', 'device'])
    with pytest.raises(Reached):
        list(tr._read_inputs([song], 'device', 2))


def test_device_reader_pulls_groups_lazily_and_opens_no_file(tmp_path, monkeypatch):
    """--decode device reads every group through audio.load_audio, whatever the files are: no probe opens them, and a
    group is requested only when the queue pulls past the one before."""
    from amt_saga import audio, transcribe as tr
    paths = [str(tmp_path / ('missing_%d.flac' % k)) for k in range(5)]
    groups = []

    def load_audio(group, verify=True):
        groups.append(list(group))
        return [('wave of ' + f, 44100 + paths.index(f), 24) for f in group]
    monkeypatch.setattr(audio, 'load_audio', load_audio)
    reader = tr._read_inputs(paths, 'device', 2)
    assert groups == []                                                            # nothing before the first pull
    want = [paths[0:2], paths[2:4], paths[4:5]]
    for k, f in enumerate(paths):
        assert next(reader) == ('wave of ' + f, 44100 + k)
        assert groups == want[:k // 2 + 1]                                         # the next group: not before its turn
    with pytest.raises(StopIteration):
        next(reader)
    assert groups == want


def test_ragged_layout_of_host_tensors():
    """The input layout of the three ragged encoder calls, stated once (audio._ragged_layout), on host tensors: base is
    every pointer minus the lowest in floats, an empty signal gets 0, lens are the lengths; no signal with samples gives
    no anchor."""
    import torch
    from amt_saga import audio
    (r0, r1, r2), lone, none = torch.zeros((3, 7)).unbind(0), torch.zeros(5), torch.zeros(0)
    for sigs in ([r0, r1, none, r2, lone], [lone, r2, none, r0, r1]):
        anchor, base, lens = audio._ragged_layout(sigs)
        assert anchor == min(s.data_ptr() for s in sigs if s.numel())
        assert lens == [int(s.numel()) for s in sigs] and sorted(lens) == [0, 5, 7, 7, 7]
        for s, b in zip(sigs, base):
            assert b == ((s.data_ptr() - anchor) // 4 if s.numel() else 0) and b >= 0
        assert base[2] == 0 and min(base) == 0
        at = dict(zip(map(id, sigs), base))
        assert at[id(r1)] - at[id(r0)] == 7 and at[id(r2)] - at[id(r0)] == 14
    assert audio._ragged_layout([none, torch.zeros(0)]) == (None, [0, 0], [0, 0])
