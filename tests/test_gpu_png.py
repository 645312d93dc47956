"""GPU: the spectrogram-image kernels (amt_png.hip) against the rule restated in tests/png_reference.py -- PNG files and
level images byte for byte, outputs prefilled with sentinels and followed by guard bytes -- then a song walk's spectra
and the command line.  Nothing here has a tolerance."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_reference as R                                          # noqa: E402
import song_oracle as so                                           # noqa: E402
from oracle import synth as osynth                                 # noqa: E402
from test_png_cpu import level_cases                               # noqa: E402

pytestmark = pytest.mark.gpu
SENT, GUARD = 0xAB, 64
ALL_HEADS = ('timing', 'pitch', 'instrument', 'velocity')


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import audio, png, _lib
    return dict(torch=torch, audio=audio, png=png, _lib=_lib, lib=_lib.load())


@pytest.fixture(scope='module')
def corpus():
    return R.corpus()


@pytest.fixture(scope='module')
def expected(corpus, env):
    """{(name, palette?): the reference's file}, computed once."""
    pal = env['png'].palette('cubehelix')
    return {(name, use): R.encode(img, pal if use else None) for name, img in corpus for use in (False, True)}


def _encode(env, images, palette):
    """amt_png_encode_ragged called directly: the images back to back behind 3 filler bytes, the output prefilled and
    followed by guard bytes.  Returns the files; the guards and the gaps are asserted."""
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    from amt_saga.device import ptr, stream_ptr
    blob, meta = bytearray(b'\xee' * 3), []
    for im in images:
        meta += [len(blob), im.shape[1], im.shape[0]]
        blob += im.tobytes()
    n = len(images)
    pix = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    m = (ctypes.c_longlong * len(meta))(*meta)
    bound = sum(int(lib.amt_png_file_bound(im.shape[1], im.shape[0], int(palette is not None))) for im in images)
    need = int(lib.amt_png_scratch_bytes(m, n))
    assert need > 0
    scratch = torch.full((need + GUARD,), SENT, dtype=torch.uint8).cuda()
    out = torch.full((bound + GUARD,), SENT, dtype=torch.uint8).cuda()
    off = torch.full((n + 1 + 4,), -7, dtype=torch.int64).cuda()
    pal = torch.from_numpy(np.ascontiguousarray(palette).reshape(-1)).cuda() if palette is not None else None
    rc = lib.amt_png_encode_ragged(ptr(pix), pix.numel(), m, n, ptr(pal) if pal is not None else None, ptr(scratch), need,
                                   ptr(out), bound, ptr(off), stream_ptr())
    assert rc == _lib.AMT_OK
    torch.cuda.synchronize()
    o, f, s = out.cpu().numpy(), off.cpu().numpy(), scratch.cpu().numpy()
    assert f[0] == 0 and np.all(f[n + 1:] == -7) and np.all(np.diff(f[:n + 1]) > 0) and f[n] <= bound
    assert np.all(o[f[n]:] == SENT) and np.all(s[need:] == SENT)
    return [o[f[i]:f[i + 1]].tobytes() for i in range(n)]


def test_every_corpus_shape_alone_byte_for_byte(env, corpus, expected):
    """1 x 1, 1 x N, the 258 cap and its remainders, runs of 2 / 3 / 4, zeros, noise (stored), 16-level noise (dynamic),
    a tiny image (fixed), one image per filter, R - 1 / R / R + 1 / 2 R + 1 rows, the widest row; palette and grey."""
    pal = env['png'].palette('cubehelix')
    for k, (name, img) in enumerate(corpus):
        for use in ((False, True) if img.size < 20000 else (bool(k % 2),)):
            got = _encode(env, [img], pal if use else None)[0]
            want = expected[(name, use)]
            assert len(got) == len(want) and got == want, (name, use, len(got), len(want))
            back, back_pal, _ = R.decode(got, pixels=img.size < 20000)
            assert img.size >= 20000 or np.array_equal(back, img), name


def test_whole_corpus_in_one_call_and_the_python_surface(env, corpus, expected):
    audio, torch = env['audio'], env['torch']
    imgs = [img for _, img in corpus]
    got = _encode(env, imgs, None)
    for (name, _), g in zip(corpus, got):
        assert g == expected[(name, False)], name
    dev = [torch.from_numpy(img).cuda() for img in imgs]
    for palette, use in (('cubehelix', True), ('gray', False)):
        files = audio.png_encode(dev, palette=palette)
        assert [f == expected[(name, use)] for (name, _), f in zip(corpus, files)] == [True] * len(corpus)
    # a non-contiguous image is taken by value
    wide = torch.from_numpy(np.ascontiguousarray(corpus[9][1])).cuda()
    assert audio.png_encode([wide[:, ::2]], 'gray')[0] == R.encode(corpus[9][1][:, ::2], None)


def test_six_ragged_images_one_call_equals_one_per_call(env):
    imgs = R.ragged_six()
    assert len({im.shape for im in imgs}) == 6
    pal = env['png'].palette('cubehelix')
    together = _encode(env, imgs, pal)
    for im, g in zip(imgs, together):
        assert g == _encode(env, [im], pal)[0] == R.encode(im, pal)
        assert np.array_equal(R.decode(g)[0], im)


@pytest.mark.parametrize('tag', ['300_of_3x2', '257_mixed'])
def test_more_images_than_threads_in_one_call(env, tag):
    """The size scan gives every thread of its one workgroup a run of images: 300 images of 3 x 2 and 257 images of
    mixed tiny sizes both make runs of 2 with the last thread short, so every file offset behind the first run is a sum
    across threads.  Every file byte for byte, palette and grey."""
    rng = np.random.RandomState(300 if tag == '300_of_3x2' else 257)
    if tag == '300_of_3x2':
        shapes = [(2, 3)] * 300
    else:
        shapes = [(1 + (i * 5) % 7, 1 + (i * 3) % 11) for i in range(257)]                     # (H, W)
        assert len(set(shapes)) > 50
    imgs = [rng.randint(0, 1 << rng.randint(1, 9), size=hw).astype(np.uint8) for hw in shapes]
    pal = env['png'].palette('cubehelix')
    for palette in (None, pal):
        got = _encode(env, imgs, palette)
        assert len({len(g) for g in got}) > 1
        assert [g == R.encode(im, palette) for im, g in zip(imgs, got)] == [True] * len(imgs)


def test_invalid_sizes_are_refused_with_nothing_written(env):
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    from amt_saga.device import ptr
    pix = torch.zeros(1 << 16, dtype=torch.uint8).cuda()
    out = torch.full((1 << 17,), SENT, dtype=torch.uint8).cuda()
    scratch = torch.full((1 << 17,), SENT, dtype=torch.uint8).cuda()
    off = torch.full((3,), -7, dtype=torch.int64).cuda()
    for meta in ((0, 4, 4, 0, 32769, 1), (0, 4, 4, 0, 16385, 1), (0, 0, 4, 0, 4, 4), (0, 4, 4, (1 << 16) - 3, 2, 2)):
        m = (ctypes.c_longlong * 6)(*meta)
        assert lib.amt_png_encode_ragged(ptr(pix), pix.numel(), m, 2, None, ptr(scratch), scratch.numel(), ptr(out),
                                         out.numel(), ptr(off), None) == _lib.AMT_E_INVALID, meta
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((scratch == SENT).all()) and bool((off == -7).all())


# ---------------------------------------------------------------------------------------------------------------
# levels
# ---------------------------------------------------------------------------------------------------------------
def _levels(env, cases):
    """amt_spec_levels_ragged on a ragged batch of level cases (spectrograms back to back, one table buffer)."""
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    from amt_saga.device import ptr, stream_ptr
    mags, tabs, meta, refs, at, tab_at, out_at = [], [], [], [], 5, 0, 3
    for name, mag, F, ref, rows, cols, thr in cases:
        T, ldf = mag.shape
        meta.append([at, T, ldf, F, len(cols), len(rows), tab_at, tab_at + rows.size, out_at, 0])
        mags.append(mag.reshape(-1))
        tabs += [rows.reshape(-1), cols.reshape(-1)]
        refs.append(ref)
        at += mag.size
        tab_at += rows.size + cols.size
        out_at += len(cols) * len(rows) + 1
    blob = torch.from_numpy(np.concatenate([np.full(5, 77.0, np.float32)] + mags)).cuda()
    tab = torch.from_numpy(np.concatenate(tabs).astype(np.int32)).cuda()
    d_meta = torch.tensor(meta, dtype=torch.int64).cuda()
    d_thr, d_ref = torch.from_numpy(cases[0][6]).cuda(), torch.tensor(np.asarray(refs, np.float32)).cuda()
    out = torch.full((out_at + GUARD,), SENT, dtype=torch.uint8).cuda()
    rc = lib.amt_spec_levels_ragged(ptr(blob), blob.numel(), ptr(d_meta), len(cases), max(len(c[5]) for c in cases),
                                    max(len(c[4]) for c in cases), ptr(tab), tab.numel(), ptr(d_thr), ptr(d_ref), ptr(out),
                                    out_at, stream_ptr())
    assert rc == _lib.AMT_OK
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    want = np.full(out_at + GUARD, SENT, np.uint8)
    for row, (name, mag, F, ref, rows, cols, thr) in zip(meta, cases):
        want[row[8]:row[8] + len(rows) * len(cols)] = R.levels(mag, ref, rows.tolist(), cols.tolist(), thr).reshape(-1)
    return o, want, meta


def test_levels_ragged_batch_pixel_for_pixel(env):
    """Magnitudes exactly on thr[k] ref and one ulp below, zeros, NaN, infinities; references of 0, inf, NaN, 2^-101 and
    2^-100; W < T, W = T, W > T on both axes: all in ONE launch, every byte of the output (gaps and guard included)."""
    cases = level_cases()
    assert {c[0] for c in cases} >= {'thresholds', 'noise W33 log', 'noise W70 linear', 'noise W97 log', 'ref inf'}
    o, want, meta = _levels(env, cases)
    bad = np.flatnonzero(o != want)
    assert bad.size == 0, (bad[:5], [c[0] for c, r in zip(cases, meta) if r[8] <= bad[0]][-1])
    # a table row that points outside costs only its own image
    torch, lib = env['torch'], env['lib']
    one = cases[1]
    o1, want1, _ = _levels(env, [one])
    assert np.array_equal(o1, want1) and want1[3:3 + 20 * 33].max() > 100


def test_levels_of_a_strided_pool_region_and_device_references(env):
    """audio.spectrogram_levels on views of one pool [G, frames, ldf] with references read from device tensors: the
    images are those of the rule on the same magnitudes copied out; the call copies nothing."""
    torch, audio, png = env['torch'], env['audio'], env['png']
    rng = np.random.default_rng(3)
    F, ldf = 33, 36
    pool = torch.from_numpy((10.0 ** rng.uniform(-4, 0, (3, 200, ldf))).astype(np.float32)).cuda()
    views = [pool[0, 10:80], pool[1, 100:131], pool[2, 10:80], pool[1, 100:160:2]]       # the last: every other frame
    assert views[3].stride(0) == 2 * ldf
    refs = torch.tensor([0.5, 1.0, 2.0, 0.25]).cuda()
    sizes = [(33, 20), (70, 9), (97, 20), (10, 64)]
    imgs = audio.spectrogram_levels(views, list(refs.unbind(0)), size=sizes, axis='log', sr=16000, n_fft=64)
    thr = png.thresholds()
    for v, r, (W, H), im in zip(views, refs.tolist(), sizes, imgs):
        assert tuple(im.shape) == (H, W) and im.dtype == torch.uint8
        want = R.levels(v.cpu().numpy(), r, png.axis_rows(F, H, 16000, 64, 'log').tolist(), R.cols(v.shape[0], W), thr)
        assert np.array_equal(im.cpu().numpy(), want)
    lin = audio.spectrogram_levels(views[:1], [0.5], size=(33, 20), axis='linear', sr=16000, n_fft=64, top_db=40.0)[0]
    want = R.levels(views[0].cpu().numpy(), 0.5, png.axis_rows(F, 20, 16000, 64, 'linear').tolist(), R.cols(70, 33),
                    R.thresholds(40.0))
    assert np.array_equal(lin.cpu().numpy(), want)
    # the two stages together equal the reference writer on the reference levels
    files = audio.spectrogram_png(views[:2], refs[:2], size=sizes[:2], sr=16000, n_fft=64)
    for f, im in zip(files, imgs[:2]):
        assert f == R.encode(im.cpu().numpy(), png.palette('cubehelix'))


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
def test_song_walk_spectra_and_plot_spec(env, tmp_path):
    """run_songs(residual=True, stems=True) on two short songs at 86-frame windows: region_spectra -> spectrogram_png
    equals the reference applied to the same magnitudes copied to the host; region_spectra has residual_waves' checks."""
    torch, audio, png = env['torch'], env['audio'], env['png']
    from amt_saga import hyperparams, loop
    p = hyperparams.Hyperparams(N=2048, window_size_note_time=1)
    lp = loop.TranscriptionLoop(p, heads=ALL_HEADS, guess='bank', groups=(0, 1, 2)).setup_device()
    songs = so.make_songs(p, 41, (2.3, 3.0))
    events, st = lp.run_songs(songs, max_notes=2, silence=1e-4, poll=4, residual=True, stems=True)
    spectra = st.region_spectra([0, 1])
    mags, refs = [], []
    for b, (res, stems) in enumerate(spectra):
        assert tuple(res.shape) == (st.frames[b], st.s_mag.shape[1]) and tuple(stems.shape) == (3, st.frames[b], st.s_mag.shape[1])
        assert res.data_ptr() == st.s_mag[st.region[b]].data_ptr()                 # views of the pool
        mags += [res] + list(stems.unbind(0))
        refs += [st.refs['ref_mag'][b]] * 4
    size = (96, 64)
    files = audio.spectrogram_png(mags, refs, size=size, sr=p.sr, n_fft=p.N)
    thr, pal = png.thresholds(), png.palette('cubehelix')
    rows = png.axis_rows(p.N // 2 + 1, size[1], p.sr, p.N, 'log').tolist()
    drawn = 0
    for m, r, f in zip(mags, refs, files):
        want = R.levels(m.cpu().numpy(), float(r), rows, R.cols(m.shape[0], size[0]), thr)
        assert f == R.encode(want, pal)
        drawn += int(want.max() > 0)
    assert drawn >= 3                                                              # residuals and at least one stem
    lp2 = loop.TranscriptionLoop(p, heads=ALL_HEADS, guess='bank', groups=(0, 1, 2)).setup_device()
    ev2, st2 = lp2.run_songs(songs, max_notes=2, silence=1e-4, poll=4)
    with pytest.raises(ValueError, match='without keep_residual and without keep_stems'):
        st2.region_spectra([0])
    with pytest.raises(ValueError, match='slot 5 holds no song'):
        st.region_spectra([5])
    st3 = lp.prepare_songs(songs, keep_residual=True)
    with pytest.raises(ValueError, match='is not finished'):
        st3.region_spectra([0])
    # audio_complete.plot_spec: 100 pixels per inch, the file written and returned
    y = osynth.render_window([(0, 60, 100, 0.1, 0.4), (1, 72, 90, 0.5, 0.3)], 20000, 22050).numpy()
    ac = audio.audio_complete(y, 1024, sample_rate=22050)
    path = str(tmp_path / 'spec.png')
    data = ac.plot_spec(width=1.5, height=0.8, filename=path)
    assert open(path, 'rb').read() == data
    mag = np.ascontiguousarray(np.asarray(ac.mag, np.float32).T)                   # [T, F]
    want = R.levels(mag, np.float32(ac.ref_mag), png.axis_rows(513, 80, 22050, 1024, 'log').tolist(), R.cols(mag.shape[0], 150), thr)
    assert data == R.encode(want, pal) and want.max() == 255


@pytest.mark.parametrize('cli', ['one_file', 'songs'])
def test_command_line_writes_the_named_files_at_the_requested_size(env, tmp_path, cli):
    from amt_saga import flac, transcribe as tr
    from amt_saga.hyperparams import Hyperparams
    p = Hyperparams(N=2048, window_size_note_time=1)
    n = int(1.4 * p.H * (p.timing_frames - 1))
    notes_in = [(j % 3, 60 + 2 * j, 100, 0.2 + 0.7 * j, 0.4) for j in range(int(n / p.sr / 0.7))]
    y = osynth.render_window(notes_in, n, p.sr).numpy()
    names = ['clip_a', 'clip_b'] if cli == 'songs' else ['clip_a']
    for k, name in enumerate(names):
        flac.save_float(y[:len(y) - 5000 * k], str(tmp_path / (name + '.flac')), p.sr)
    spec = str(tmp_path / 'spec')
    if cli == 'one_file':
        tr.main([str(tmp_path / 'clip_a.flac'), str(tmp_path / 'a.mid'), '--iters', '1', '--traversal', 'song',
                 '--spectrogram-dir', spec, '--spectrogram-size', '300x120'])
    else:
        tr.main(['--songs'] + [str(tmp_path / (nm + '.flac')) for nm in names] + ['--out-dir', str(tmp_path / 'mid'),
                 '--slots', '2', '--iters', '1', '--spectrogram-dir', spec, '--spectrogram-size', '300x120'])
    kinds = ['song', 'residual'] + ['group%d' % g for g in tr.CLI_GROUPS]
    assert sorted(os.listdir(spec)) == sorted('%s.%s.png' % (nm, k) for nm in names for k in kinds)
    for nm in names:
        levels = {}
        for k in kinds:
            img, pal, chunks = R.decode(open(os.path.join(spec, '%s.%s.png' % (nm, k)), 'rb').read())
            assert img.shape == (120, 300) and pal.shape == (256, 3)
            levels[k] = img
        assert levels['song'].max() == 255                                 # drawn against the song's own maximum
