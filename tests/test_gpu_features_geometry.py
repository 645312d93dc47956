"""GPU: the feature kernels of amt_features.hip (compress_bands / _fmax, short_window, gather_frames, amplitude_to_db,
db_to_amplitude, spectral_flatness) through the C ABI over every geometry they accept, against the numpy restatement of
tests/features_reference.py (pinned on the CPU by test_features_reference_cpu.py).

Set-up of every case: B = 3 windows scaled 1, 3 and 1e-3; input rows of ldf = ldf_of(N) + 8 bins and
spec_stride = (T + 2) * ldf, NaN in the pad bins and the two gap rows, so that a read of either poisons the output; outputs
filled with -7 and everything outside the documented extent asserted to hold it still.  These are the smallest shapes at
which each branch can go wrong, not workload shapes.

Bars (features_reference states them in full; u = 2^-24):
  * band means, DERIVED: |got - float64| <= (MAXQ + 8) u mean|x| / |ref| per band and frame -- no term of the kernel's
    sum passes through more than MAXQ additions in its lane and six in the wave reduction ((MAXQ + 6) u sum|x|, first
    order), and the two divisions are correctly rounded (2 u of a result that is at most sum|x| / (width |ref|)).  A band
    inside the first 64 bins is walked by one lane on the generic path: width - 1 additions and the divisions,
    (width + 2) u in its place.  Zero columns (a frame index outside [0, T)) have mean|x| = 0: exact.
  * frame_max, short_window mode 0, gather_frames: bit for bit.
  * short_window modes 1 / 2, dB, inverse dB, flatness rest on the device's log10f / atan2f / exp10f / logf / expf, whose
    accuracy is not derived here: e_gpu <= 2.5 e_f32numpy + 4 u scale per window, both errors measured against the float64
    run on the same float32 inputs.  Every such case's e_gpu, e_f32numpy and ratio are printed and written as
    features_error_vs_f64.json into the directory the environment variable AMT_RECORD_DIR names (a copy is kept as
    profiles/features_error_vs_f64.json).  The assertions are the bars; the ratio is a record."""
import json
import os

import numpy as np
import pytest

import features_reference as fr      # tests/features_reference.py

pytestmark = pytest.mark.gpu

SENT = fr.SENT
RECORD = []
REF3 = np.array([0.7, 2.0, 1e-3], np.float32)


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('AMT_RECORD_DIR')
    if out:
        try:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, 'features_error_vs_f64.json'), 'w') as f:
                json.dump(RECORD, f, indent=1)
        except OSError:
            pass
    for r in RECORD:
        print('e_gpu/e_f32numpy  %-18s %-44s gpu %.3g  f32numpy %.3g  ratio %.2f  bar %.3g' %
              (r['kernel'], r['geometry'], r['e_gpu'], r['e_f32numpy'], r['ratio'], r['bar']))


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import _lib
    return dict(torch=torch, lib=_lib.load(), _lib=_lib)


def _p(t):
    return None if t is None else t.data_ptr()


def _up(env, a):
    return None if a is None else env['torch'].from_numpy(np.ascontiguousarray(a)).cuda()


def _sent(env, n, dtype=None):
    torch = env['torch']
    return torch.full((n,), SENT, device='cuda', dtype=dtype or torch.float32)


def _fetch(env, buf, n):
    """The first n elements of a sentinel-filled buffer, after asserting that the rest still holds the sentinel."""
    env['torch'].cuda.synchronize()
    o = buf.cpu().numpy()
    assert np.all(o[n:] == SENT), 'written past the documented extent'
    return o[:n]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_transcendental(kernel, geometry, got, ref64, ref32):
    """Asserts e_gpu <= 2.5 e_f32numpy + 4 u scale for every window and records the window closest to its bar."""
    e_gpu, e_32, scale = fr.window_errors(got, ref64), fr.window_errors(ref32, ref64), fr.window_scales(ref64)
    bar = fr.transcendental_bar(e_32, scale)
    w = int(np.argmax(e_gpu / np.maximum(bar, 1e-300)))
    row = dict(kernel=kernel, geometry=geometry, window=w, e_gpu=float(e_gpu[w]), e_f32numpy=float(e_32[w]),
               ratio=float(e_gpu[w] / max(e_32[w], 1e-30)), bar=float(bar[w]))
    RECORD.append(row)
    print('%-18s %-44s window %d e_gpu %.3g e_f32numpy %.3g ratio %.2f bar %.3g' %
          (kernel, geometry, w, row['e_gpu'], row['e_f32numpy'], row['ratio'], row['bar']))
    assert np.all(e_gpu <= bar), (kernel, geometry, e_gpu.tolist(), bar.tolist())


# ---------------------------------------------------------------------------------------------------------------------
# compress_bands / compress_bands_fmax
# ---------------------------------------------------------------------------------------------------------------------
def _compress(env, d_mag, B, T, F, ldf, edges, d_ref, tab, target, fmax=False):
    """One launch on sentinel-filled outputs: (out [B][bands][target], frame_max [B][T] or None)."""
    lib = env['lib']
    bands = len(edges) - 1
    n = B * bands * target
    out, fm = _sent(env, n + 5), _sent(env, B * T + 1) if fmax else None
    d_e, d_t = _up(env, edges), _up(env, tab)
    if fmax:
        st = lib.amt_compress_bands_fmax(_p(d_mag), B, T, F, ldf, (T + 2) * ldf, _p(d_e), bands, _p(d_ref), _p(d_t), _p(out),
                                         target, _p(fm), None)
    else:
        st = lib.amt_compress_bands(_p(d_mag), B, T, F, ldf, (T + 2) * ldf, _p(d_e), bands, _p(d_ref), _p(d_t), _p(out),
                                    target, None)
    assert st == env['_lib'].AMT_OK, st
    got = _fetch(env, out, n).reshape(B, bands, target)
    return got, (_fetch(env, fm, B * T).reshape(B, T) if fmax else None)


def _columns(full, tab, T):
    """Columns of an identity-map result [B][bands][T] under a frame map (zero where the index is outside [0, T))."""
    if tab is None:
        return full
    ok = (tab >= 0) & (tab < T)
    return np.where(ok[None, None, :], full[:, :, np.where(ok, tab, 0)], 0.0)


@pytest.mark.parametrize('F', fr.CB_BINS)
def test_compress_bands_every_geometry(env, F):
    """All edge sets x T in 1, 3, 4, 5, 9 x all frame maps at one F: band means inside the derived bar, zero columns
    exact; with the identity map also amt_compress_bands_fmax -- the same bits, and frame_max bit-equal to the float32 row
    maximum, window 2 being negative throughout."""
    B = 3
    d_ref = _up(env, REF3)
    worst = (0.0, 0, '', '')
    for T in fr.CB_FRAMES:
        h = fr.spectra(B, T, F, 1000 * F + T)
        ldf = h.shape[2]
        assert ldf == fr.ldf_of_bins(F) + 8 and np.all(h[2, :T, :F] < 0)
        d = _up(env, h)
        rowmax = h[:, :T, :F].max(axis=2)
        for name, edges in fr.edge_sets(F).items():
            want_full, _ = fr.compress_bands(h, T, F, edges, REF3)
            bar_full = fr.compress_bands_bar(F, edges, fr.band_abs_means(h, T, F, edges), REF3,
                                             fast_path=tuple(edges) == fr.CB_STD_EDGES and F == 1025)
            for mname, (tab, target) in fr.frame_maps(T).items():
                got, _ = _compress(env, d, B, T, F, ldf, edges, d_ref, tab, target)
                want, bar = _columns(want_full, tab, T), _columns(bar_full, tab, T)
                assert not np.isnan(got).any(), (T, name, mname)
                err = np.abs(got - want)
                frac = float((err / np.maximum(bar, 1e-300)).max())
                worst = max(worst, (frac, T, name, mname))
                assert np.all(err <= bar), (T, name, mname, frac)
                if tab is None:
                    got2, fm = _compress(env, d, B, T, F, ldf, edges, d_ref, None, T, fmax=True)
                    assert np.array_equal(_bits(got2), _bits(got)), (T, name)
                    assert np.array_equal(_bits(fm), _bits(rowmax)), (T, name, fm.tolist(), rowmax.tolist())
    print('compress_bands F %d MAXQ %d: largest error / bar %.3f at T %d %s %s' % ((F, fr.maxq_of(F)) + worst))


def test_compress_bands_fast_and_generic_path_agree(env):
    """F = 1025: the 20 standard edges take the compile-time path; with one interior edge moved by one bin (90 -> 91) the
    kernel takes the generic one.  Each against float64 at its bar, and the eighteen bands the move leaves alone against
    each other at the bar of the band."""
    B, T, F = 3, 9, 1025
    h = fr.spectra(B, T, F, 77)
    ldf = h.shape[2]
    d, d_ref = _up(env, h), _up(env, REF3)
    std = np.array(fr.CB_STD_EDGES, np.int32)
    moved = std.copy()
    moved[13] += 1
    am = fr.band_abs_means(h, T, F, std)
    fast, _ = _compress(env, d, B, T, F, ldf, std, d_ref, None, T)
    gen, _ = _compress(env, d, B, T, F, ldf, moved, d_ref, None, T)
    assert np.all(np.abs(fast - fr.compress_bands(h, T, F, std, REF3)[0]) <= fr.compress_bands_bar(F, std, am, REF3, True))
    bar_g = fr.compress_bands_bar(F, moved, fr.band_abs_means(h, T, F, moved), REF3)
    assert np.all(np.abs(gen - fr.compress_bands(h, T, F, moved, REF3)[0]) <= bar_g)
    same = np.array([i not in (12, 13) for i in range(20)])
    diff = np.abs(fast.astype(np.float64) - gen)[:, same]
    print('fast vs generic: largest difference / bar %.3f' % float((diff / bar_g[:, same]).max()))
    assert np.all(diff <= bar_g[:, same])
    assert np.all(fast[:, :5] == gen[:, :5])                        # one-bin bands: x / 1 / ref on both paths


# ---------------------------------------------------------------------------------------------------------------------
# short_window
# ---------------------------------------------------------------------------------------------------------------------
def _tables(T, frames, seed):
    """[3][frames]: window 0 valid and invalid frames starting with frame 0, window 1 only -1 and indices >= T (its
    selection is all zero), window 2 mostly valid."""
    rng = np.random.default_rng(seed)
    tab = np.empty((3, frames), np.int32)
    tab[0] = rng.integers(-1, T + 2, frames)
    tab[0, 0] = 0
    tab[1] = np.where(np.arange(frames) % 2 == 0, -1, T + np.arange(frames) % 3)
    tab[2] = rng.integers(0, T, frames)
    if frames > 1:
        tab[2, frames // 2] = T
    return tab


@pytest.mark.parametrize('F,frames,bands', [(F, fr_, b) for F in fr.SW_BINS for fr_ in fr.SW_FRAMES for b in fr.SW_BANDS])
def test_short_window_every_geometry(env, F, frames, bands):
    """Modes 0 / 1 / 2 with band_min NULL, (-3, 0, 11) and (F - 5, 11, -3), tables holding -1 and indices >= T.  Mode 0
    bit for bit (one correctly rounded division; ref NULL = a copy); a window whose selection is all zero is all NaN in
    mode 1 and all 3.15f / 6.3f in mode 2; modes 1 / 2 at the transcendental bar."""
    lib, _lib = env['lib'], env['_lib']
    B, T = 3, 9
    m, ph = fr.spectra(B, T, F, F + frames, kind='mag'), fr.phases(B, T, F, F + bands)
    ldf = m.shape[2]
    ss = (T + 2) * ldf
    d_m, d_ph, d_ref = _up(env, m), _up(env, ph), _up(env, REF3)
    tab = _tables(T, frames, frames * 7 + bands)
    d_tab = _up(env, tab)
    n = B * bands * frames
    half = np.float32(3.15) / np.float32(6.3)
    for lo in (None, np.array([-3, 0, 11], np.int32), np.array([F - 5, 11, -3], np.int32)):
        d_lo = _up(env, lo)
        geom = 'F %d frames %d bands %d band_min %s' % (F, frames, bands, 'NULL' if lo is None else lo.tolist())
        for mode, ref in ((0, REF3), (0, None), (1, None), (2, None)):
            out = _sent(env, n + 3)
            st = lib.amt_short_window(_p(d_m) if mode != 2 else None, _p(d_ph) if mode == 2 else None, B, T, F, ldf, ss,
                                      _p(d_tab), frames, _p(d_lo), bands, _p(d_ref) if ref is not None else None, mode,
                                      _p(out), None)
            assert st == _lib.AMT_OK, st
            got = _fetch(env, out, n).reshape(B, bands, frames)
            r32 = fr.short_window(m, ph, T, F, tab, lo, bands, ref, mode, np.float32)
            if mode == 0:
                assert np.array_equal(_bits(got), _bits(r32)), geom
                assert np.all(got[1] == 0)
                continue
            r64 = fr.short_window(m, ph, T, F, tab, lo, bands, ref, mode)
            if mode == 1:
                assert np.all(np.isnan(got[1])), geom                  # (_check_transcendental: NaNs only where float64 has them)
            else:
                assert np.all(got[1] == half) and not np.isnan(got).any(), geom
                f0 = (0 if lo is None else int(lo[0])) + np.arange(bands)
                inside = np.isin(tab[0], np.arange(T))[None, :] & ((f0 >= 0) & (f0 < F))[:, None]
                assert np.all(got[0][~inside] == half)                  # frames outside [0, T), bins below 0 and past F
            _check_transcendental('short_window_mode%d' % mode, geom, got, r64, r32)
    if bands > 16:
        # the four axis points and the zero vector of phases(): frame 0 (column 0 of every table of window 0), bins
        # 12 .. 16 = rows 1 .. 5 at band_min 11
        out, d_lo = _sent(env, n + 3), _up(env, np.full(B, 11, np.int32))
        assert lib.amt_short_window(None, _p(d_ph), B, T, F, ldf, ss, _p(d_tab), frames, _p(d_lo), bands, None, 2,
                                    _p(out), None) == _lib.AMT_OK
        got = _fetch(env, out, n).reshape(B, bands, frames)[0, 1:6, 0]
        want = (np.array([0.0, np.pi / 2, np.pi, -np.pi / 2, 0.0]) + 3.15) / 6.3
        print('axis points', got.tolist())
        assert np.all(np.abs(got - want) <= 4 * fr.U) and got[0] == half and got[4] == half


# ---------------------------------------------------------------------------------------------------------------------
# gather_frames
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('elem', (1, 2))
def test_gather_frames_every_argument(env, elem):
    """Copies, bit for bit: band_min 0 / 5 with bands < ldf_out and the whole row; a per-window table (stride 9 > n_out)
    with -1 and indices >= T; table_stride 0 against a per-window table holding the same rows; T = 0.  The pad of every
    output row is zero, the gap between windows keeps the sentinel."""
    lib, _lib = env['lib'], env['_lib']
    B, T, F, n_out, ts = 3, 5, 257, 7, 9
    h = np.stack([fr.spectra(B, T, F, 40 + c) for c in range(elem)], axis=-1)       # [B][T + 2][ldf][elem]
    ldf = h.shape[2]
    d = _up(env, h)
    rng = np.random.default_rng(elem)
    tab = rng.integers(-1, T + 3, (B, ts)).astype(np.int32)
    tab[0, :4] = (-1, T, 0, T - 1)
    same = np.tile(tab[1], (B, 1))

    def run(T_, table, stride, band_min, bands, ldf_out):
        os_ = (n_out + 1) * ldf_out * elem                             # one gap row per window
        out, d_tab = _sent(env, B * os_ + 3), _up(env, table)
        st = lib.amt_gather_frames(_p(d), B, T_, F, ldf, (T + 2) * ldf * elem, elem, _p(d_tab), stride, n_out,
                                   band_min, bands, _p(out), ldf_out, os_, None)
        assert st == _lib.AMT_OK, st
        o = _fetch(env, out, B * os_).reshape(B, n_out + 1, ldf_out, elem)
        assert np.all(o[:, n_out] == SENT)
        want = fr.gather_frames(h.reshape(B, T + 2, -1), T_, F, elem, table, stride, n_out, band_min, bands, ldf_out)
        assert np.array_equal(_bits(o[:, :n_out]), _bits(want)), (T_, stride, band_min, bands, ldf_out)
        assert np.all(o[:, :n_out, bands:] == 0)
        return o[:, :n_out]

    for band_min, bands, ldf_out in ((0, 40, 48), (5, 40, 48), (0, F, fr.ldf_of_bins(F)), (5, F, F + 2), (F - 3, 9, 9)):
        run(T, tab, ts, band_min, bands, ldf_out)
        a = run(T, same, ts, band_min, bands, ldf_out)
        b = run(T, tab[1], 0, band_min, bands, ldf_out)
        assert np.array_equal(_bits(a), _bits(b))
    assert np.all(run(0, tab, ts, 0, 40, 48) == 0)


# ---------------------------------------------------------------------------------------------------------------------
# dB, inverse dB, flatness
# ---------------------------------------------------------------------------------------------------------------------
DB_CASES = [(257, 3, 5), (1025, 3, 4), (1025, 1, 1012), (1025, 1, 1013)]      # 1012 / 1013 frames of 1036: below / above
                                                                              # 1024 * 1024 elements (the capped grid)

@pytest.mark.parametrize('F,B,T', DB_CASES)
def test_amplitude_to_db_and_back(env, F, B, T):
    """Magnitudes over 1e-9 .. 10 (amin and the -80 dB floor are both hit), a reference per window, top_db 80 and < 0;
    the inverse on dB values over -100 .. 20.  Pad bins are written as zero, the gap rows keep the sentinel."""
    lib, _lib = env['lib'], env['_lib']
    m = fr.spectra(B, T, F, F + T, kind='wide')
    ldf = m.shape[2]
    ss = (T + 2) * ldf
    assert ldf == (1036 if F == 1025 else 268) and (T * ldf > 1024 * 1024) == (T == 1013)
    ref = np.array([1.0, 0.37, 5e-6], np.float32)[:B]
    wmax = m[:, :T, :F].reshape(B, -1).max(axis=1)
    d_m, d_ref, d_wmax = _up(env, m), _up(env, ref), _up(env, wmax)
    for top_db in (80.0, -1.0):
        out = _sent(env, B * ss + 3)
        assert lib.amt_amplitude_to_db(_p(d_m), B, T, F, ldf, ss, _p(d_ref), _p(d_wmax), 1e-5, top_db, _p(out),
                                       None) == _lib.AMT_OK
        o = _fetch(env, out, B * ss).reshape(B, T + 2, ldf)
        assert np.all(o[:, T:] == SENT) and np.all(o[:, :T, F:] == 0)
        r64 = fr.amplitude_to_db(m, T, F, ref, wmax, np.float32(1e-5), top_db)
        r32 = fr.amplitude_to_db(m, T, F, ref, wmax, np.float32(1e-5), top_db, np.float32)
        floor = r64[:, :, :F].min(axis=(1, 2))
        assert np.all((r64[:, :, :F] == floor[:, None, None]).mean(axis=(1, 2)) > 0.2)      # amin or the floor is hit
        _check_transcendental('amplitude_to_db', 'F %d B %d T %d top_db %g' % (F, B, T, top_db), o[:, :T], r64, r32)
    db = np.full_like(m, np.nan)
    db[:, :T, :F] = np.random.default_rng(F * T).uniform(-100.0, 20.0, (B, T, F))
    out, d_db = _sent(env, B * ss + 3), _up(env, db)
    assert lib.amt_db_to_amplitude(_p(d_db), B, T, F, ldf, ss, _p(d_ref), _p(out), None) == _lib.AMT_OK
    o = _fetch(env, out, B * ss).reshape(B, T + 2, ldf)
    assert np.all(o[:, T:] == SENT) and np.all(o[:, :T, F:] == 0)
    _check_transcendental('db_to_amplitude', 'F %d B %d T %d' % (F, B, T), o[:, :T],
                          fr.db_to_amplitude(db, T, F, ref), fr.db_to_amplitude(db, T, F, ref, np.float32))


@pytest.mark.parametrize('F', fr.FLAT_BINS)
def test_spectral_flatness(env, F):
    """One wave per frame, T = 9 (a last workgroup of one wave), F = 129 (a 64-lane trip of one lane) and 1025; noise-like
    (flatness near its largest) and wide-range (amin is hit) spectra."""
    lib, _lib = env['lib'], env['_lib']
    B, T = 3, 9
    for kind in ('mag', 'wide'):
        m = fr.spectra(B, T, F, F + 3, kind=kind)
        ldf = m.shape[2]
        out, d_m = _sent(env, B * T + 2), _up(env, m)
        assert lib.amt_spectral_flatness(_p(d_m), B, T, F, ldf, (T + 2) * ldf, 1e-10, _p(out), None) == _lib.AMT_OK
        got = _fetch(env, out, B * T).reshape(B, T)
        amin = np.float32(1e-10)
        _check_transcendental('spectral_flatness', 'F %d B %d T %d %s' % (F, B, T, kind), got,
                              fr.spectral_flatness(m, T, F, amin), fr.spectral_flatness(m, T, F, amin, np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    """Host-side return codes; nothing is launched and no buffer is touched."""
    lib, L = env['lib'], env['_lib']
    torch = env['torch']
    buf = torch.full((4 * 4200,), SENT, device='cuda')
    ibuf = torch.zeros(64, dtype=torch.int32, device='cuda')
    b, i = _p(buf), _p(ibuf)
    for F in (2113, 4097):
        assert lib.amt_compress_bands(b, 1, 1, F, 4100, 4100, i, 1, None, None, b, 1, None) == L.AMT_E_UNSUPPORTED
        assert lib.amt_compress_bands_fmax(b, 1, 1, F, 4100, 4100, i, 1, None, None, b, 1, b, None) == L.AMT_E_UNSUPPORTED
    assert lib.amt_compress_bands(b, 1, 2, 257, 256, 600, i, 1, None, None, b, 2, None) == L.AMT_E_SHAPE
    assert lib.amt_compress_bands_fmax(b, 1, 2, 257, 260, 600, i, 1, None, i, b, 2, b, None) == L.AMT_E_INVALID
    assert lib.amt_compress_bands_fmax(b, 1, 2, 257, 260, 600, i, 1, None, None, b, 3, b, None) == L.AMT_E_INVALID
    sw = lambda mag, ph, mode, ldf=260: lib.amt_short_window(mag, ph, 1, 2, 257, ldf, 600, i, 2, None, 4, None, mode, b, None)
    assert sw(b, b, 3) == L.AMT_E_INVALID and sw(b, b, -1) == L.AMT_E_INVALID
    assert sw(b, None, 2) == L.AMT_E_ATTRIB and sw(None, b, 0) == L.AMT_E_ATTRIB and sw(None, b, 1) == L.AMT_E_ATTRIB
    assert sw(b, b, 0, 256) == L.AMT_E_SHAPE
    gf = lambda elem=1, ts=0, n_out=4, bands=8, ldf_out=8, ldf=260: lib.amt_gather_frames(
        b, 1, 2, 257, ldf, 600, elem, i, ts, n_out, 0, bands, b, ldf_out, 64, None)
    assert gf(elem=3) == L.AMT_E_ATTRIB and gf(elem=0) == L.AMT_E_ATTRIB
    assert gf(ldf_out=7) == L.AMT_E_SHAPE and gf(ts=3) == L.AMT_E_SHAPE and gf(ldf=256) == L.AMT_E_SHAPE
    assert lib.amt_amplitude_to_db(b, 1, 2, 257, 260, 600, b, b, 0.0, 80.0, b, None) == L.AMT_E_SHAPE
    assert lib.amt_amplitude_to_db(b, 1, 2, 257, 256, 600, b, b, 1e-5, 80.0, b, None) == L.AMT_E_SHAPE
    assert lib.amt_db_to_amplitude(b, 1, 2, 257, 256, 600, b, b, None) == L.AMT_E_SHAPE
    assert lib.amt_spectral_flatness(b, 1, 2, 257, 260, 600, 0.0, b, None) == L.AMT_E_SHAPE
    assert lib.amt_spectral_flatness(b, 1, 2, 257, 256, 600, 1e-10, b, None) == L.AMT_E_SHAPE
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()) and bool((ibuf == 0).all())
