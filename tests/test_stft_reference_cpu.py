"""CPU: the float64 STFT / iSTFT restatement of tests/stft_reference.py against the oracle that is already pinned to
scipy and the reference vectors, the headroom ordinary float32 leaves inside the bars the GPU tests assert, and a check
that the error measures see an error confined to one quiet bin."""
import numpy as np
import pytest

import stft_reference as sr      # tests/stft_reference.py

from oracle import audio as oa

GEOMS = sr.GEOMETRIES
IDS = ['n%d-h%d-c%d' % g for g in GEOMS]


@pytest.mark.parametrize('n_fft,hop,center', GEOMS, ids=IDS)
def test_reference_agrees_with_oracle(n_fft, hop, center):
    """stft64 to complex64 rounding of oracle.audio.stft, istft64 to float32 rounding of oracle.audio.istft."""
    for L in sr.lengths_of(n_fft, hop, center):
        for y in sr.signals(L, L, n_fft, hop, center):
            F = sr.stft64(y, n_fft, hop, center)
            Fo = oa.stft(y, n_fft, hop, bool(center))
            assert Fo.dtype == np.complex64 and Fo.shape == F.shape == (n_fft // 2 + 1, sr.n_frames(L, n_fft, hop, center))
            # one rounding of each part to float32: half an ulp of the larger part
            assert np.all(np.abs(F - Fo) <= 2 * sr.U * np.abs(F) + 1e-300)
    for T in sr.inverse_frames(n_fft, hop, center):
        if sr.out_len(T, n_fft, hop, center) <= 0:
            continue
        L = sr.out_len(T, n_fft, hop, center)
        F = sr.ramped_spectrum(max(L, n_fft), T, n_fft, hop, center)[:, :T]
        y, wss, acc = sr.istft64(F, hop, center)
        yo = oa.istft(F, hop, bool(center))
        assert yo.dtype == np.float32 and yo.shape == y.shape == wss.shape == acc.shape == (L,)
        assert np.all(np.abs(y - yo) <= sr.U * np.abs(y) + 1e-300)
        nz = wss > sr.TINY32
        assert np.array_equal(y[nz], acc[nz] / wss[nz]) and np.array_equal(y[~nz], acc[~nz])


@pytest.mark.parametrize('n_fft,hop,center', GEOMS, ids=IDS)
def test_float32_sits_ten_times_inside_the_bars(n_fft, hop, center):
    """Every geometry, length and signal of the matrix: the float32 CPU restatement, under the measures the GPU tests
    assert, stays below a tenth of the bar (forward: magnitudes and complex; inverse: magnitude + unit phase and
    complex input)."""
    b = sr.bar(n_fft)
    for L in sr.lengths_of(n_fft, hop, center):
        for name, y in zip(sr.SIGNALS, sr.signals(L, L, n_fft, hop, center)):
            F64, F32 = sr.stft64(y, n_fft, hop, center), sr.stft32(y, n_fft, hop, center)
            e_c, e_m = sr.stft_error(F32, F64), sr.stft_error(np.abs(F32), np.abs(F64))
            assert max(e_c, e_m) <= b / 10, (L, name, e_c, e_m, b)
    for T in sr.inverse_frames(n_fft, hop, center):
        L = sr.out_len(T, n_fft, hop, center)
        if L <= 0:
            continue
        F = sr.ramped_spectrum(max(L, n_fft), T, n_fft, hop, center)[:, :T]
        mag32, ph32, Fmp = sr.split_magphase32(F)
        Fc = F.astype(np.complex64)
        for tag, Fin, F_in32 in (('magphase', Fmp, mag32 * ph32), ('complex', Fc.astype(np.complex128), Fc)):
            y, wss, _ = sr.istft64(Fin, hop, center)
            e = sr.istft_error(sr.istft32(F_in32, hop, center)[0], y, wss)
            assert e <= b / 10, (T, tag, e, b)


def test_phase_comparison_covers_half_of_white_noise():
    """The phase tests compare bins above 1e-3 of their frame's largest float64 magnitude: on the white-noise signal
    that is at least half of all bins, at every geometry."""
    for n_fft, hop, center in GEOMS:
        L = sr.lengths_of(n_fft, hop, center)[2]
        m = np.abs(sr.stft64(sr.white(L, 5), n_fft, hop, center))
        share = sr.phase_compared(m).mean()
        assert share >= 0.5, (n_fft, hop, center, share)


def test_measures_catch_one_quiet_bin():
    """One bin of one quiet frame off by 1e-3 of that frame's norm: the per-frame measure reports far more than its
    bar, the largest-difference-over-the-window's-maximum measure at 1e-4 (test_gpu_audio.REL) does not; the same
    error in one frame of an iSTFT input is reported by the iSTFT measure."""
    n_fft, hop, center = 2048, 512, 1
    L = 37 * hop
    y = sr.loud_quiet(L, 3, n_fft, hop, center)
    F = sr.stft64(y, n_fft, hop, center)
    T = F.shape[1]
    t = T - 3 - (T - 3) % 2                          # an even frame well inside the quiet half: its pair is quiet
    assert sr.loud_quiet_switch(L, n_fft, hop, center) <= t * hop - n_fft // 2
    nrm = np.sqrt((np.abs(F) ** 2).sum(0))
    assert max(nrm[t], nrm[t + 1]) < 1e-5 * nrm.max()
    bad = F.copy()
    bad[300, t] += 1e-3 * nrm[t]
    assert sr.stft_error(F, F) == 0.0
    for got, ref in ((bad, F), (np.abs(bad), np.abs(F))):
        assert sr.stft_error(got, ref) > 100 * sr.bar(n_fft)
        assert sr.relmax_of_window(np.abs(got), np.abs(ref)) < 1e-4
    Fr = sr.ramped_spectrum(L, 4, n_fft, hop, center)
    yr, wss, _ = sr.istft64(Fr, hop, center)
    assert sr.istft_error(yr, yr, wss) == 0.0
    badr = Fr.copy()
    badr[300, 10] += 1e-3 * np.sqrt((np.abs(Fr[:, 10]) ** 2).sum())
    assert sr.istft_error(sr.istft64(badr, hop, center)[0], yr, wss) > sr.bar(n_fft)
    # a sample librosa leaves undivided (wss = 0: the frame starts at hop = N) must come out as 0
    Fz = sr.ramped_spectrum(4 * n_fft, 6, n_fft, n_fft, 0)
    yz, wz, _ = sr.istft64(Fz, n_fft, 0)
    assert (wz <= sr.TINY32).sum() == Fz.shape[1]
    gz = yz.copy()
    gz[n_fft] = 1e-3 * np.abs(yz).max()
    assert sr.istft_error(gz, yz, wz) > sr.bar(n_fft)
