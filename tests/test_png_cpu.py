"""CPU: spectrogram images without a GPU.  The writer of tests/png_reference.py reads back through an independent reader
(and through PIL where it is installed); the core the kernels compile (csrc/amt_png_core.h) writes the same bytes and
the same levels in a stand-alone program built with the address and undefined-behaviour sanitizers; the host tables of
amt_saga.png have their known answers; the rule's files stay within 0.02 of zlib's Z_RLE strategy on spectrograms of the
reference's recordings; the ABI, the Python entry points and the command line refuse bad arguments before a GPU is
touched."""
import ctypes
import io
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def corpus():
    return R.corpus()


@pytest.fixture(scope='module')
def files(corpus):
    from amt_saga import png
    pal = png.palette('cubehelix')
    out = []
    for k, (name, img) in enumerate(corpus):
        info = {}
        p = pal if k % 2 == 0 else None
        out.append((name, img, p, R.encode(img, p, info), info))
    return out


def test_writer_reads_back_through_the_independent_reader(files):
    kinds, filters = set(), set()
    for name, img, pal, data, info in files:
        got, got_pal, names = R.decode(data)
        assert np.array_equal(got, img), name
        assert (got_pal is None) == (pal is None) and (pal is None or np.array_equal(got_pal, pal)), name
        assert names == [b'IHDR'] + ([b'PLTE'] if pal is not None else []) + [b'IDAT'] * len(info['kinds']) + [b'IEND'], name
        assert len(info['kinds']) == -(-img.shape[0] // R.piece_rows(img.shape[1])), name
        kinds |= set(info['kinds'])
        filters |= set(info['filters'])
        # no piece beyond its stored size: the payload is at most the stored form of every piece, the header and Adler-32
        assert info['payload'] <= len(info['filtered']) + 5 * len(info['kinds']) + 6, name
    assert kinds == set(R.KINDS) and filters == {0, 1, 2, 3, 4}
    by = {name: info for name, _, _, _, info in files}
    assert by['noise255']['kinds'] == ['stored'] and by['noise15']['kinds'] == ['dynamic'] and by['small']['kinds'] == ['fixed']
    for f in range(5):                                                 # built so that the filter is chosen
        assert by['filter%d' % f]['filters'].count(f) >= 7, (f, by['filter%d' % f]['filters'])
    assert [len(by['rows%d' % h]['kinds']) for h in (7, 8, 9, 17)] == [1, 1, 2, 3]
    assert len(by['widest']['kinds']) == 3


def test_writer_reads_back_through_pil(files):
    Image = pytest.importorskip('PIL.Image')
    for name, img, pal, data, info in files:
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (img.shape[1], img.shape[0]) and im.mode == ('P' if pal is not None else 'L'), name
        assert np.array_equal(np.asarray(im), img), name
        if pal is not None:
            assert np.array_equal(np.asarray(im.getpalette(), np.uint8).reshape(-1, 3)[:256], pal), name


def test_token_and_code_rules_by_hand():
    assert [R.length_symbol(n) for n in (3, 10, 11, 12, 13, 18, 19, 227, 257, 258)] == \
        [(257, 0, 0), (264, 0, 0), (265, 1, 0), (265, 1, 1), (266, 1, 0), (268, 1, 1), (269, 2, 0), (284, 5, 0),
         (284, 5, 30), (285, 0, 0)]
    lit = (9, 0, 0)
    assert R.run_tokens(bytes([9] * 1)) == [lit]
    assert R.run_tokens(bytes([9] * 3)) == [lit] * 3                       # 2 left: literals
    assert R.run_tokens(bytes([9] * 4)) == [lit, (257, 0, 0)]
    assert R.run_tokens(bytes([9] * 259)) == [lit, (285, 0, 0)]
    assert R.run_tokens(bytes([9] * 260)) == [lit, (285, 0, 0), lit]
    assert R.run_tokens(bytes([9] * 261)) == [lit, (285, 0, 0), lit, lit]
    assert R.run_tokens(bytes([9] * 262)) == [lit, (285, 0, 0), (257, 0, 0)]
    assert R.run_tokens(bytes([1, 1, 2])) == [(1, 0, 0), (1, 0, 0), (2, 0, 0)]
    # code lengths: complete (Kraft sum 1) within the limit, shorter for the more frequent; the limit bites on a
    # Fibonacci-like histogram
    rng = np.random.default_rng(0)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for freq, limit in ((fib, 15), (fib[:19], 7), (list(rng.integers(0, 50, 286)), 15), ([0, 5, 0, 0], 7), ([0] * 19, 7),
                        ([3, 3, 3, 3], 15)):
        lens = R.code_lengths(freq, limit)
        used = [l for l in lens if l]
        assert len(used) >= 2 and max(used) <= limit and sum(2 ** (limit - l) for l in used) == 2 ** limit, freq
        pairs = [(f, -m) for f, m in sorted((int(f), -l) for f, l in zip(freq, lens) if f)]
        assert all(a[1] >= b[1] for a, b in zip(pairs, pairs[1:])), freq
    assert R.code_lengths([3, 3, 3, 3], 15) == [2, 2, 2, 2] and R.code_lengths([0, 5, 0, 0], 7) == [1, 1, 0, 0]
    assert max(R.code_lengths(fib, 15)) == 15 and max(R.code_lengths(fib[:12], 15)) == 11
    assert R.cl_tokens([0] * 150 + [5] * 9 + [0, 0, 3]) == [(18, 7, 127), (18, 7, 1), (5, 0, 0), (16, 2, 3), (5, 0, 0),
                                                           (5, 0, 0), (0, 0, 0), (0, 0, 0), (3, 0, 0)]


def test_host_tables_have_their_known_answers():
    from amt_saga import png
    thr = png.thresholds()
    assert thr.dtype == np.float32 and thr.shape == (255,) and np.all(np.diff(thr) > 0)
    assert np.array_equal(thr, R.thresholds())
    assert thr[0] == np.float32(10.0 ** (-4.0 * (1 - 0.5 / 255))) and thr[-1] == np.float32(10.0 ** (-4.0 * 0.5 / 255))
    assert 1e-4 < thr[0] < 1.04e-4 and 0.98 < thr[-1] < 1.0
    assert np.array_equal(png.thresholds(40.0), R.thresholds(40.0))
    for bad in (0, -3, float('inf'), 1e-9):
        with pytest.raises(ValueError):
            png.thresholds(bad)
    for T, W in ((70, 33), (70, 70), (33, 70), (1, 5), (1000, 1)):
        c = png.axis_cols(T, W)
        assert c.dtype == np.int32 and c.tolist() == [list(p) for p in R.cols(T, W)]
        assert c[0, 0] == 0 and c[-1, 1] == T and np.all(c[:, 1] > c[:, 0]) and np.all(np.diff(c[:, 0]) >= 0)
        if W <= T:                                                     # every frame exactly once
            assert np.array_equal(np.concatenate([np.arange(a, b) for a, b in c]), np.arange(T))
    assert png.axis_cols(3, 6)[:, 0].tolist() == [0, 0, 1, 1, 2, 2]
    for F, H, sr, n_fft in ((33, 20, 16000, 64), (33, 64, 16000, 64), (1025, 500, 44100, 2048), (1025, 3, 44100, 2048)):
        for axis in png.AXES:
            r = png.axis_rows(F, H, sr, n_fft, axis)
            assert r.dtype == np.int32 and r.shape == (H, 2)
            up = r[::-1]                                               # from the lowest frequency
            assert up[-1, 1] == F and np.all(up[:, 1] > up[:, 0]) and np.all(up >= 0) and np.all(up <= F)
            assert np.all(np.diff(up[:, 0]) >= 0) and np.all(np.diff(up[:, 1]) >= 0)
        lin = png.axis_rows(F, H, sr, n_fft, 'linear')[::-1]
        assert lin.tolist() == [[j * F // H, max(j * F // H + 1, (j + 1) * F // H)] for j in range(H)]
    # log: equal ratios from 27.5 Hz to sr / 2; a row with bin centres in its interval takes exactly those
    F, H, sr, n_fft = 1025, 500, 44100, 2048
    up = png.axis_rows(F, H, sr, n_fft, 'log')[::-1]
    edge = 27.5 * (sr / 2 / 27.5) ** (np.arange(H + 1) / H)
    centre = np.arange(F) * sr / n_fft
    for j in (H - 1, H - 2, 400, 300):
        inside = np.flatnonzero((centre >= edge[j]) & ((centre < edge[j + 1]) | (j == H - 1)))
        assert inside.size and up[j].tolist() == [inside[0], inside[-1] + 1], j
    assert up[0].tolist() == [1, 2]                                     # 27.5 Hz .. : the nearest bin is 21.5 Hz
    assert up[-1, 1] - up[-1, 0] > 5
    with pytest.raises(ValueError, match='axis must be one of'):
        png.axis_rows(33, 5, 16000, 64, 'mel')
    for bad in (0, 16385, 2.5, True):
        with pytest.raises(ValueError):
            png.axis_rows(33, bad, 16000, 64)
        with pytest.raises(ValueError):
            png.axis_cols(10, bad)
    pal = png.palette('cubehelix')
    assert pal.dtype == np.uint8 and pal.shape == (256, 3) and png.palette('gray') is None
    assert pal[0].tolist() == [0, 0, 0] and pal[255].tolist() == [255, 255, 255]
    lum = pal.astype(np.float64) @ np.array([0.30, 0.59, 0.11])
    assert np.all(np.diff(lum) > 0) and np.max(np.abs(lum - np.arange(256))) < 2.0
    # the closed form at one level by hand: x = 0.5 -> phi = 2 pi (1/6 - 0.75), a = 0.125
    phi = 2 * np.pi * (0.5 / 3 - 1.5 * 0.5)
    x = 127.5 / 255
    want = [x + 0.125 * (-0.14861 * np.cos(phi) + 1.78277 * np.sin(phi)), x + 0.125 * (-0.29227 * np.cos(phi) - 0.90649 * np.sin(phi)),
            x + 0.125 * 1.97294 * np.cos(phi)]
    mid = (pal[127].astype(int) + pal[128].astype(int)) / 2
    assert np.max(np.abs(mid - 255 * np.array(want))) < 1.5
    with pytest.raises(ValueError, match='palette must be one of'):
        png.palette('viridis')
    assert png.parse_size('1200x500') == (1200, 500) and png.parse_size('1X1') == (1, 1)
    for bad in ('1200', '0x5', '5x16385', 'axb', '3x4x5', ''):
        with pytest.raises(ValueError):
            png.parse_size(bad)


def level_cases():
    """[(name, mag [T, ldf], F, ref, rows, cols, thr)]: F = 33, T up to 70."""
    from amt_saga import png
    rng = np.random.default_rng(7)
    F, ldf, thr = 33, 40, png.thresholds()
    out = []
    ref = np.float32(3.7)
    prod = thr * ref
    edge = np.concatenate([prod, np.nextafter(prod, np.float32(0)), [0, np.nan, np.inf, -1.0, 1e-30, 3.7, 4.0]]).astype(np.float32)
    T = -(-edge.size // F)
    mag = np.zeros((T, ldf), np.float32)
    mag[:, :F] = np.resize(edge, T * F).reshape(T, F)
    mag[:, F:] = 99.0                                                   # the padding of a frame is never read
    one = lambda n: np.stack([np.arange(n), np.arange(n) + 1], 1).astype(np.int32)
    out.append(('thresholds', mag, F, ref, one(F)[::-1].copy(), one(T), thr))
    noise = (10.0 ** rng.uniform(-5, 0.3, (70, ldf))).astype(np.float32)
    noise[rng.integers(0, 70, 40), rng.integers(0, F, 40)] = np.nan
    noise[5:9, 3:20] = 0
    for W in (33, 70, 97):
        for axis in png.AXES:
            out.append(('noise W%d %s' % (W, axis), noise, F, np.float32(1.3), png.axis_rows(F, 20, 16000, 64, axis),
                        png.axis_cols(70, W), thr))
    for r in (0.0, np.inf, -np.inf, np.nan, 2.0 ** -101, -1.0):
        out.append(('ref %r' % r, noise[:9], F, np.float32(r), png.axis_rows(F, 7, 16000, 64), png.axis_cols(9, 5), thr))
    tiny = (noise[:9] * np.float32(2.0 ** -100)).astype(np.float32)
    out.append(('ref 2^-100', tiny, F, np.float32(2.0 ** -100), png.axis_rows(F, 7, 16000, 64), png.axis_cols(9, 5), thr))
    return out


def test_level_rule_by_hand():
    from amt_saga import png
    thr = png.thresholds()
    name, mag, F, ref, rows, cols, _ = level_cases()[0]
    lv = R.levels(mag, ref, rows.tolist(), cols.tolist(), thr)
    flat = lv[::-1].T.reshape(-1)                                       # frame-major, as the magnitudes were laid
    assert flat[:255].tolist() == list(range(1, 256))                   # exactly on thr[k] ref: level k
    assert flat[255:510].tolist() == list(range(0, 255))                # one ulp below: level k - 1
    assert flat[510:517].tolist() == [0, 0, 255, 0, 0, 255, 255]        # 0, NaN, inf, -1, 1e-30, ref, above ref
    for case in level_cases():
        if case[0].startswith('ref ') and case[0] != 'ref 2^-100':
            assert not R.levels(*[case[i] for i in (1, 3)], case[4].tolist(), case[5].tolist(), thr).any(), case[0]
    name, mag, F, ref, rows, cols, _ = level_cases()[-1]
    assert R.levels(mag, ref, rows.tolist(), cols.tolist(), thr).max() == 255


def test_core_in_a_sanitised_stand_alone_program(files, tmp_path):
    """amt_png_core.h, host only, under the address and undefined-behaviour sanitizers: every corpus file byte for byte
    from buffers of exactly the stated sizes, every level case pixel for pixel -- and no sanitizer report (a report
    aborts the program: a nonzero exit)."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'png_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-ffp-contract=off', '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'png_host_main.cpp'), '-o', exe], check=True)
    cases = []
    for name, img, pal, data, info in files:
        cases.append(struct.pack('<iiii', 0, img.shape[1], img.shape[0], int(pal is not None))
                     + (pal.tobytes() if pal is not None else b'') + img.tobytes() + struct.pack('<q', len(data)) + data)
    n_enc = len(cases)
    for name, mag, F, ref, rows, cols, thr in level_cases():
        want = R.levels(mag, ref, rows.tolist(), cols.tolist(), thr)
        cases.append(struct.pack('<iiiiiiI', 1, mag.shape[0], mag.shape[1], F, len(cols), len(rows), int(np.float32(ref).view(np.uint32)))
                     + thr.astype('<f4').tobytes() + mag.astype('<f4').tobytes() + rows.astype('<i4').tobytes()
                     + cols.astype('<i4').tobytes() + want.tobytes())
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        f.write(b'PNGC' + struct.pack('<i', len(cases)) + b''.join(cases))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('-> ok') == len(cases) and 'runtime error' not in r.stderr
    assert r.stdout.count(' encode ') == n_enc


# ---------------------------------------------------------------------------------------------------------------
# compression against zlib's Z_RLE on spectrograms of the reference's recordings
# ---------------------------------------------------------------------------------------------------------------
RECORDINGS = ('w_0930fc9ea219', 'w_0c9a22988cb6', 'w_190e4c9fb3ad', 'w_01de8c09e152')
IMAGE_W, IMAGE_H = 400, 510


def spectrogram_image(pcm, sr=44100, n_fft=2048, hop=512):
    """The W x H log-axis level image of an int PCM recording: a Hann STFT in numpy, the tables of amt_saga.png."""
    from amt_saga import png
    y = pcm.astype(np.float64) / max(1.0, float(np.abs(pcm).max()))
    y = np.pad(y, n_fft // 2, mode='reflect')
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    frames = np.lib.stride_tricks.sliding_window_view(y, n_fft)[::hop]
    mag = np.abs(np.fft.rfft(frames * win, axis=1)).astype(np.float32)             # [T, F]
    rows, cols = png.axis_rows(mag.shape[1], IMAGE_H, sr, n_fft, 'log'), png.axis_cols(mag.shape[0], IMAGE_W)
    by_row = np.stack([mag[:, a:b].max(axis=1) for a, b in rows])                   # [H, T]
    cell = np.stack([by_row[:, a:b].max(axis=1) for a, b in cols], axis=1)          # [H, W]
    prod = (png.thresholds() * mag.max()).astype(np.float32)
    return np.searchsorted(prod, cell, side='right').astype(np.uint8)


def test_compression_stays_within_two_hundredths_of_zlib_rle():
    """Summed IDAT payloads of the rule over summed zlib Z_RLE output (the same run matches, one dynamic block over the
    whole image) on the same filtered bytes.  The bar: the ratio measured when the sizes were recorded plus 0.02, the
    room of the per-piece block headers."""
    with open(os.path.join(GOLDEN, 'png_sizes.json')) as f:
        rec = json.load(f)
    assert rec['recordings'] == list(RECORDINGS) and rec['size'] == [IMAGE_W, IMAGE_H]
    waves = np.load(os.path.join(GOLDEN, 'recorded_waves.npz'))
    ours = rle = raw = 0
    for key in RECORDINGS:
        img = spectrogram_image(waves[key])
        info = {}
        data = R.encode(img, None, info)
        assert np.array_equal(R.decode(data, pixels=False)[0].shape, (0, IMAGE_W))
        z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        rle += len(z.compress(info['filtered']) + z.flush())
        ours += info['payload']
        raw += len(info['filtered'])
        assert zlib.decompress(b''.join(_idat(data))) == info['filtered']
    ratio = ours / rle
    print('payload %d, Z_RLE %d, filtered %d: ratio %.4f (recorded %.4f)' % (ours, rle, raw, ratio, rec['ratio']))
    assert ratio <= rec['ratio'] + 0.02
    assert abs(ours - rec['payload']) <= 0.01 * rec['payload'] and raw == rec['filtered']
    assert ours < 0.6 * raw


def _idat(data):
    at = 8
    while at < len(data):
        n, kind = struct.unpack('>I4s', data[at:at + 8])
        if kind == b'IDAT':
            yield data[at + 8:at + 8 + n]
        at += 12 + n


# ---------------------------------------------------------------------------------------------------------------
# ABI, Python entry points, command line
# ---------------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_arguments_before_any_hip_call():
    from amt_saga import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                                        # never dereferenced: checks come first

    def levels(**kw):
        a = dict(mag=p, mag_floats=100, meta=p, n=1, max_w=4, max_h=4, tables=p, table_ints=16, thr=p, ref=p, out=p, out_bytes=16)
        a.update(kw)
        return lib.amt_spec_levels_ragged(a['mag'], a['mag_floats'], a['meta'], a['n'], a['max_w'], a['max_h'], a['tables'],
                                          a['table_ints'], a['thr'], a['ref'], a['out'], a['out_bytes'], None)

    def encode(meta=(0, 4, 4), n=1, **kw):
        m = (ctypes.c_longlong * len(meta))(*meta) if meta is not None else None
        a = dict(pix=p, pix_bytes=16, meta=m, palette=None, scratch=p, scratch_bytes=1 << 20, out=p, out_bytes=1 << 20, off=p)
        a.update(kw)
        return lib.amt_png_encode_ragged(a['pix'], a['pix_bytes'], a['meta'], n, a['palette'], a['scratch'], a['scratch_bytes'],
                                         a['out'], a['out_bytes'], a['off'], None)
    for k in ('mag', 'meta', 'tables', 'thr', 'ref', 'out'):
        assert levels(**{k: None}) == _lib.AMT_E_INVALID, k
    for kw in (dict(n=0), dict(n=65536), dict(max_w=0), dict(max_h=16385), dict(mag_floats=-1), dict(table_ints=-1),
               dict(out_bytes=-1)):
        assert levels(**kw) == _lib.AMT_E_INVALID, kw
    for k in ('pix', 'meta', 'scratch', 'out', 'off'):
        assert encode(**{k: None}) == _lib.AMT_E_INVALID, k
    for meta in ((0, 0, 4), (0, 4, 0), (0, 16385, 1), (0, 1, 16385), (0, 32769, 1), (-1, 4, 4), (1, 4, 4), (0, 5, 4)):
        assert encode(meta=meta) == _lib.AMT_E_INVALID, meta                       # the last two: outside pix
    assert encode(n=0) == encode(n=65536) == _lib.AMT_E_INVALID
    assert encode(scratch_bytes=64) == _lib.AMT_E_SHAPE and encode(out_bytes=64) == _lib.AMT_E_SHAPE
    assert lib.amt_png_file_bound(0, 4, 1) == lib.amt_png_file_bound(4, 16385, 0) == _lib.AMT_E_INVALID
    m = (ctypes.c_longlong * 3)(0, 16385, 1)
    assert lib.amt_png_scratch_bytes(m, 1) == _lib.AMT_E_INVALID


def test_file_bound_holds_every_corpus_file(files):
    from amt_saga import _lib
    lib = _lib.load()
    for name, img, pal, data, info in files:
        bound = lib.amt_png_file_bound(img.shape[1], img.shape[0], int(pal is not None))
        assert len(data) <= bound, name
        stored = 8 + 25 + (780 if pal is not None else 0) + 12 + len(info['kinds']) * (12 + 5) + 6 + img.shape[0] * (img.shape[1] + 1)
        assert bound == stored + 6 * (len(info['kinds']) - 1), name              # (every chunk counted as first and last)
    assert len(files[9][4]['kinds']) == 1 and files[9][0] == 'noise255' and \
        len(files[9][3]) == lib.amt_png_file_bound(130, 90, int(files[9][2] is not None))   # all stored: the bound is met


def test_python_and_command_line_refuse_bad_arguments_before_the_gpu(tmp_path, capsys):
    from amt_saga import audio, transcribe as tr
    with pytest.raises(ValueError, match='uint8 device tensors'):
        audio.png_encode([np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError, match='at least one image'):
        audio.png_encode([])
    with pytest.raises(ValueError, match='palette must be one of'):
        audio.png_encode([], palette='jet')
    with pytest.raises(ValueError, match='float32 device tensors'):
        audio.spectrogram_levels([np.zeros((4, 33), np.float32)], [1.0], size=(4, 4), sr=16000, n_fft=64)
    with pytest.raises(ValueError, match='axis must be one of'):
        audio.spectrogram_levels([], [], size=(4, 4), axis='mel', sr=16000, n_fft=64)
    missing = str(tmp_path / 'missing.flac')
    with pytest.raises(SystemExit, match='--spectrogram-dir needs --traversal song'):
        tr.main([missing, str(tmp_path / 'o.mid'), '--spectrogram-dir', str(tmp_path / 's')])
    for argv in ([missing, str(tmp_path / 'o.mid'), '--traversal', 'song'], ['--songs', missing, '--out-dir', str(tmp_path / 'o')]):
        with pytest.raises(SystemExit, match='WxH'):
            tr.main(argv + ['--spectrogram-dir', str(tmp_path / 's'), '--spectrogram-size', '1200'])
        with pytest.raises(FileNotFoundError):                                     # accepted: the file is what fails
            tr.main(argv + ['--spectrogram-dir', str(tmp_path / 's'), '--spectrogram-size', '300x200'])
