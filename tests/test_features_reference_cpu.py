"""CPU: the restatements of tests/features_reference.py against the oracle that is already pinned to the reference
(oracle/audio.py, oracle/cqt.py), against the vectors the reference's own methods recorded
(tests/golden/reference_vectors.npz), and the float32 run of compress_bands against the derived bar the GPU test
asserts.  The GPU tests rest on these functions; this module is what they rest on."""
import numpy as np
import pytest

import features_reference as fr      # tests/features_reference.py

from oracle import audio as oa
from oracle.cqt import slice_C_frames

ACO = oa.AudioCompleteOracle


def _dev(spec_ft, pad=3):
    """[F][T] of the reference -> device layout [1][T + 1][ldf], NaN in the gap row and the pad bins."""
    F, T = spec_ft.shape[:2]
    h = np.full((1, T + 1, fr.ldf_of_bins(F) + pad) + spec_ft.shape[2:], np.nan, spec_ft.dtype)
    h[0, :T, :F] = np.swapaxes(spec_ft, 0, 1)
    return h


def test_band_edges_and_tables():
    for F in fr.CB_BINS:
        for bands in (20, 40, 80):
            e = fr.band_edges(F, bands)
            assert np.array_equal(e, oa.band_edges(F, bands)) and e[0] == 0 and np.all(np.diff(e) >= 1)
        for name, e in fr.edge_sets(F).items():
            assert e.dtype == np.int32 and e[0] == 0 and e[-1] <= F and np.all(np.diff(e) >= 1), (F, name)
    assert tuple(fr.band_edges(1025, 20)) == fr.CB_STD_EDGES          # the kernel's compile-time edges
    assert [fr.maxq_of(F) for F in (1, 320, 321, 1088, 1089, 2112, 2113)] == [5, 5, 17, 17, 33, 33, None]
    for T in fr.CB_FRAMES:
        for name, (tab, target) in fr.frame_maps(T).items():
            assert tab is None or (tab.dtype == np.int32 and len(tab) == target)
        assert fr.frame_maps(T)['beyond'][0].max() >= T


@pytest.mark.parametrize('F', fr.CB_BINS)
def test_compress_bands_vs_oracle(F):
    """Every edge set and frame map of the matrix: float64 against compress_bands + _resize of the oracle (log bands
    through its own band_edges, the others as plain means), and the float32 run inside the derived bar."""
    T = 9
    h = fr.spectra(3, T, F, F, kind='mixed')
    ref = np.array([0.7, 2.0, 1e-3], np.float32)
    for name, edges in fr.edge_sets(F).items():
        for mname, (tab, target) in fr.frame_maps(T).items():
            got, fmax = fr.compress_bands(h, T, F, edges, ref, tab, target)
            assert got.shape == (3, len(edges) - 1, target) and fmax.shape == (3, T) and fmax.dtype == np.float32
            got32, _ = fr.compress_bands(h, T, F, edges, ref, tab, target, np.float32)
            assert got32.dtype == np.float32
            am = fr.band_abs_means(h, T, F, edges, tab, target)
            assert np.all(np.abs(got32 - got) <= fr.compress_bands_bar(F, edges, am, ref)), (name, mname)
            for b in range(3):
                S = h[b, :T, :F].T.astype(np.float64)
                if name.startswith('log'):
                    cb = ACO.compress_bands(S, len(edges) - 1)
                elif name == 'lin8':
                    cb = ACO.compress_bands(S, 8, log=False)
                else:
                    cb = np.stack([S[edges[i]:edges[i + 1]].mean(axis=0) for i in range(len(edges) - 1)])
                if tab is None:
                    want = cb
                elif mname.startswith('resize'):
                    t = int(mname[6:])
                    # the table is _resize of the first t frames; beyond T the kernel's columns are zero
                    src = cb[:, :t] if t <= T else np.concatenate([cb, np.zeros((len(cb), t - T))], axis=1)
                    want = ACO._resize(src, 8)
                else:
                    ok = (tab >= 0) & (tab < T)
                    want = np.where(ok[None, :], cb[:, np.where(ok, tab, 0)], 0.0)
                want = want / np.float64(ref[b])
                assert np.allclose(got[b], want, rtol=1e-13, atol=1e-300), (name, mname, b)
                assert np.array_equal(fmax[b], S.max(axis=0).astype(np.float32))
    assert np.all(fmax[2] < 0) and np.all(fmax[0] > 0)


def test_compress_bands_vs_recorded_vectors(refvec):
    """The reference took np.mean of float32 rows, i.e. summed in float32 in an order of numpy's choosing: any order of
    n terms stays within (n - 1) u sum|x| of the exact sum, one more u for the division -- taken as (n + 2) u mean|x|."""
    for F, T, edges, key in ((1025, 6, fr.band_edges(1025, 20), 'cb_%s_1025'), (2049, 6, fr.band_edges(2049, 20), 'cb_%s_2049'),
                             (64, 3, fr.linear_edges(64, 8), 'cb_lin_%s')):
        h = _dev(refvec[key % 'in'])
        got, _ = fr.compress_bands(h, T, F, edges)
        rec = refvec[key % 'out']
        bar = (np.diff(edges) + 2)[:, None] * fr.U * fr.band_abs_means(h, T, F, edges)[0]
        assert got[0].shape == rec.shape and np.all(np.abs(got[0] - rec) <= bar), key
        assert np.abs(got[0] - rec).max() > 0 or F == 64


def test_resize_table_every_interval():
    """Every (s, t) in [-2, T + 2]^2 at T = 12, frames 3 / 4 / 8 / 32, against the reference's concatenate / tile
    formulation (oracle.audio.resize_index_map through oracle.cqt.slice_C_frames): the whole len = 0 / < 3 / < frames /
    = frames / > frames partition."""
    T = fr.RESIZE_T
    s, t = [a.ravel() for a in np.meshgrid(np.arange(-2, T + 3), np.arange(-2, T + 3), indexing='ij')]
    seen = set()
    for frames in fr.RESIZE_FRAMES:
        tab = fr.resize_table(s, t, T, frames)
        assert tab.shape == (len(s), frames) and tab.dtype == np.int32
        for i in range(len(s)):
            assert np.array_equal(tab[i], slice_C_frames(T, int(s[i]), int(t[i]), frames)), (s[i], t[i], frames)
            n = max(min(t[i], T), min(max(s[i], 0), T)) - min(max(s[i], 0), T)
            seen.add((n == 0, 0 < n < 3, 3 <= n < frames, n == frames, n > frames))
    assert len(seen) == 5
    for n in range(0, 14):
        assert np.array_equal(fr.resize_table([0], [n], 64, 8)[0], oa.resize_index_map(n, 8))


def test_window_selection_vs_recorded_vectors(refvec):
    """gather_frames (elem 1 and 2) and short_window mode 0 with a resize_table row against what the reference's
    resize / section_power recorded."""
    mag, ph = refvec['sec_mag'], refvec['sec_ph']
    F, T = mag.shape
    o = ACO(np.zeros(128 * (T - 1), np.float32), 512)
    dm = _dev(mag)
    dp = _dev(np.stack([ph.real, ph.imag], axis=-1).astype(np.float32))
    lo = int(refvec['secpow_lo'])
    for i in range(4):
        start, dur = refvec['rsz%d_args' % i]
        s, t = o._seconds_to_frames(float(start)), o._seconds_to_frames(float(start + dur))
        tab = fr.resize_table([s], [t], T, 8)
        g = fr.gather_frames(dm, T, F, 1, tab, 8, 8, 0, F, F + 3)
        assert np.array_equal(g[0, :, :F, 0].T, refvec['rsz%d_mag' % i]) and np.all(g[0, :, F:] == 0)
        g2 = fr.gather_frames(dp.reshape(1, T + 1, -1), T, F, 2, tab, 0, 8, 0, F, F)
        assert np.array_equal(g2[0, :, :, 0].T + 1j * g2[0, :, :, 1].T, refvec['rsz%d_ph' % i])
        for band_min, key in ((lo, 'rsz%d_secpow'), (200, 'rsz%d_secpow_hi')):
            sw = fr.short_window(dm, None, T, F, tab, np.array([band_min]), 348, None, 0, np.float32)
            assert np.array_equal(sw[0], refvec[key % i])
            assert np.array_equal(fr.gather_frames(dm, T, F, 1, tab, 8, 8, band_min, 348, 348)[0, :, :, 0].T, sw[0])


def test_short_window_modes_vs_recipe():
    """Modes 0 / 1 / 2 against the recipe of training.py:347-363 written with the oracle's layout ([F][T] arrays,
    np.angle), for band_min below 0, inside and running past F, and table entries outside [0, T)."""
    B, T, F, bands, frames = 3, 5, 257, 40, 8
    m = fr.spectra(B, T, F, 1, kind='mag')
    p = fr.phases(B, T, F, 2)
    tab = np.array([[0, 1, 2, -1, 4, 5, 3, 0], [-1] * 8, [4, 4, 0, 7, 1, 2, 3, -1]], np.int32)
    lo = np.array([-3, 11, F - 5], np.int32)
    ref = np.array([0.5, 2.0, 3.0], np.float32)
    f0 = fr.short_window(m, None, T, F, tab, lo, bands, ref, 0)
    f1 = fr.short_window(m, None, T, F, tab, lo, bands, None, 1)
    f2 = fr.short_window(None, p, T, F, tab, lo, bands, None, 2)
    for b in range(B):
        S = m[b, :T, :F].T.astype(np.float64)
        P = (p[b, :T, :F, 0] + 1j * p[b, :T, :F, 1].astype(np.float64)).T
        band, bandp = np.zeros((bands, frames)), np.zeros((bands, frames), np.complex128)
        for j, t in enumerate(tab[b]):
            for r in range(bands):
                if 0 <= t < T and 0 <= lo[b] + r < F:
                    band[r, j], bandp[r, j] = S[lo[b] + r, t], P[lo[b] + r, t]
        assert np.array_equal(f0[b], band / np.float64(ref[b]))
        lg = np.log10(band * 1000 + 1)
        if lg.max() > 0:
            assert np.array_equal(f1[b], lg / lg.max())
        else:
            assert np.all(np.isnan(f1[b]))
        assert np.allclose(f2[b], (np.angle(bandp) + 3.15) / 6.3, rtol=0, atol=1e-15)
    assert np.all(np.isnan(f1[1])) and np.all(f2[1] == 3.15 / 6.3)
    # the four axis points and the zero vector (frame 0, bins 12 .. 16 = rows 1 .. 5 of window 1's band at 11)
    ax = fr.short_window(None, p, T, F, np.zeros((B, 1), np.int32), np.full(B, 11, np.int32), 6, None, 2)[1, 1:6, 0]
    assert np.allclose(ax, (np.array([0, np.pi / 2, np.pi, -np.pi / 2, 0]) + 3.15) / 6.3, rtol=0, atol=1e-15)
    out32 = fr.short_window(None, p, T, F, tab, lo, bands, None, 2, np.float32)
    assert out32.dtype == np.float32 and np.all(out32[1] == np.float32(3.15) / np.float32(6.3))


def test_db_and_flatness_vs_oracle():
    B, T, F = 3, 7, 257
    m = fr.spectra(B, T, F, 4, kind='wide')
    ref = np.array([1.0, 0.37, 5e-6], np.float32)                      # the last below amin
    wmax = np.nanmax(m.reshape(B, -1), axis=1)
    for top_db, o_top in ((80.0, 80.0), (30.0, 30.0), (-1.0, None)):
        d = fr.amplitude_to_db(m, T, F, ref, wmax, 1e-5, top_db)
        assert d.shape == (B, T, m.shape[2]) and np.all(d[:, :, F:] == 0)
        for b in range(B):
            want = oa.amplitude_to_db(m[b, :T, :F].astype(np.float64), ref=np.float64(ref[b]), top_db=o_top)
            assert np.allclose(d[b, :, :F], want, rtol=0, atol=1e-11), (top_db, b)
        assert (d[:, :, :F].min() < -95) == (top_db < 0)      # amin reached only without the floor
    assert fr.amplitude_to_db(m, T, F, ref, wmax, 1e-5, 80.0, np.float32).dtype == np.float32
    db = np.full_like(m, np.nan)
    db[:, :T, :F] = np.random.default_rng(5).uniform(-100, 20, (B, T, F))
    a = fr.db_to_amplitude(db, T, F, ref)
    for b in range(B):
        want = oa.db_to_amplitude(db[b, :T, :F].astype(np.float64), ref=np.float64(ref[b]))
        assert np.allclose(a[b, :, :F], want, rtol=1e-14, atol=0) and np.all(a[b, :, F:] == 0)
    for F2 in fr.FLAT_BINS:
        m2 = fr.spectra(B, T, F2, 6, kind='wide')
        fl = fr.spectral_flatness(m2, T, F2, 1e-10)
        for b in range(B):
            want = oa.spectral_flatness(m2[b, :T, :F2].T.astype(np.float64))
            assert np.allclose(fl[b], want[0], rtol=1e-12, atol=0)
        f32 = fr.spectral_flatness(m2, T, F2, 1e-10, np.float32)
        assert f32.dtype == np.float32 and np.allclose(f32, fl, rtol=1e-4)


def test_integer_glue_known_answers():
    x = np.array([0.5, 1.5, 2.5, -3.0, 99.7, np.nan, 2.4999, -0.5, -1.5, -2.5, np.inf, -np.inf, 3e9, -3e9, -0.0,
                  50.5, -0.4], np.float32)
    assert fr.round_clamp(x, 0, 50).tolist() == [0, 2, 2, 0, 50, 0, 2, 0, 0, 0, 50, 0, 50, 0, 0, 50, 0]
    assert fr.round_clamp(x, -5, 3).tolist() == [0, 2, 2, -3, 3, -5, 2, 0, -2, -2, 3, -5, 3, -5, 0, 3, 0]
    assert fr.round_clamp(x, 4, 4).tolist() == [4] * len(x)
    rng = np.random.default_rng(0)
    p = rng.standard_normal((50, 7)).astype(np.float32)
    p[:, 5] = p[:, 2]                                                   # ties
    assert np.array_equal(fr.argmax_rows(p), p.argmax(axis=1))
    nan, inf = np.nan, np.inf
    q = np.array([[nan, 1, 3, 3], [nan, nan, nan, nan], [nan, -inf, nan, -inf], [2, nan, 5, nan], [-inf] * 4,
                  [1, 1, 1, 1], [0, inf, nan, inf]], np.float32)
    assert fr.argmax_rows(q).tolist() == [2, 0, 1, 2, 0, 0, 1]
    group = np.array([2, 0, 1], np.int32)
    gi, gf = fr.note_select([-1, 0, 5, 1], [20, 21, 200, 60], [3, 9, 0, 0], [10, 2, 500, 0], group, 3, 21, 88, 43, 173)
    assert gi.tolist() == [2 * 88, 2 * 88, 88 + 87, 39] and gf.tolist() == [50, 43, 173, 43]
    gi, gf = fr.note_select(None, [30], [1], [2], None, 3, 21, 88, 43, 173)
    assert gi.tolist() == [9] and gf.tolist() == [44]
    ev = fr.pack_events(2, 100, 3, [60, 61], None, [5, 6], None, [9, 8])
    assert ev.tolist() == [[100, 3, 60, -1, 5, -1, 9], [101, 3, 61, -1, 6, -1, 8]]
    assert fr.affine_i32([0, 3, -2, 2 ** 30], -4, 7).tolist() == [7, -5, 15, 7] and fr.affine_i32([1], 2, 3).dtype == np.int32
