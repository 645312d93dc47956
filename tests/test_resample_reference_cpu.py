"""CPU: the resampler's definition (tests/resample_reference.py, float64) has the properties the device kernel is built
for -- output lengths and reduced ratios, unit gain of every phase, a flat passband, a stopband at or below -90 dB when
decimating and for the image when interpolating, zero phase -- and amt_saga.audio raises ValueError for every bad
argument before it touches the library or a GPU.

The -90 dB bar: Kaiser's design relation gives 8.7 + beta / 0.1102 = 99.4 dB for beta = 10; the bar leaves about 10 dB
for the relation being empirical and for the leakage of the estimate.  Measured values are printed."""
import math

import numpy as np
import pytest

import resample_reference as rr      # tests/resample_reference.py


@pytest.mark.parametrize('sr_in,sr_out', rr.PAIRS)
def test_length_and_ratios(sr_in, sr_out):
    from amt_saga.audio import Resampler
    L, M, R = rr.ratio(sr_in, sr_out)
    assert math.gcd(L, M) == 1 and L * sr_in == M * sr_out and R == max(L, M)
    rs = Resampler(sr_in, sr_out)
    assert (rs.L, rs.M, rs.taps) == (L, M, rr.taps_max(sr_in, sr_out))
    for n_in in (1, 2, 37, 1000, 4097, 13230000):
        n_out = rr.out_len(n_in, sr_in, sr_out)
        assert n_out == math.ceil(n_in * L / M) == rs.out_len(n_in)           # (exact in float64 at these sizes)
        assert (n_out - 1) * M < n_in * L <= n_out * M
    # the most taps any output uses is what taps_max says: the filter's support |n M - m L| <= Z R, counted
    _, _, valid = rr._taps(10 ** 6 * L + np.arange(L), 10 ** 9, sr_in, sr_out)
    assert valid.sum(axis=1).max() == rr.taps_max(sr_in, sr_out)
    assert valid.sum(axis=1).min() >= rr.taps_max(sr_in, sr_out) - 1


@pytest.mark.parametrize('sr_in,sr_out', rr.PAIRS + [rr.STEEP])
def test_phase_sums(sr_in, sr_out):
    s = rr.phase_sums(sr_in, sr_out)
    assert len(s) == rr.ratio(sr_in, sr_out)[0]
    print('phase sums %d -> %d: max |sum - 1| = %.3g' % (sr_in, sr_out, np.abs(s - 1).max()))
    assert np.abs(s - 1).max() <= 1e-5


@pytest.mark.parametrize('sr_in', (48000, 96000, 16000))
def test_passband(sr_in):
    sr_out = 44100
    nyq = min(sr_in, sr_out) / 2
    for frac in (0.05, 0.5, 0.8):
        x = rr.tone(frac * nyq, sr_in, 0.25)
        y, _, _ = rr.resample_at(x, sr_in, sr_out)
        gain = rr.db(rr.middle_rms(y) / rr.middle_rms(x))
        print('passband %d -> %d at %.2f x Nyquist: %+.4f dB' % (sr_in, sr_out, frac, gain))
        assert abs(gain) <= 0.05


@pytest.mark.parametrize('sr_in,sr_out', [(48000, 44100), (96000, 44100), (192000, 44100), (44100, 22050)])
def test_stopband_decimating(sr_in, sr_out):
    for frac in (1.02, 1.05, 1.2):
        if frac * sr_out >= sr_in:
            # 48 kHz -> 44.1 kHz: 1.2 x 22050 Hz lies above the INPUT's Nyquist; sampled at 48 kHz that tone is the
            # 21540 Hz tone, which belongs to the passband.  The other pairs carry the 1.2 case.
            assert (sr_in, frac) == (48000, 1.2)
            continue
        x = rr.tone(frac * sr_out / 2, sr_in, 0.25)
        y, _, _ = rr.resample_at(x, sr_in, sr_out)
        level = rr.db(rr.middle_rms(y) / rr.middle_rms(x))
        print('stopband %d -> %d at %.2f x output Nyquist: %.1f dB' % (sr_in, sr_out, frac, level))
        assert level <= -90.0


@pytest.mark.parametrize('sr_in,sr_out', [(22050, 44100), (16000, 44100), (8000, 44100), (44100, 48000)])
def test_stopband_interpolating_image(sr_in, sr_out):
    f = 0.8 * sr_in / 2
    f_image = sr_in - f
    if f_image > sr_out / 2:                       # 44.1 -> 48 kHz: the image at 26460 Hz shows folded, at 21540 Hz
        f_image = sr_out - f_image
    assert f < f_image < sr_out / 2
    y, _, _ = rr.resample_at(rr.tone(f, sr_in, 0.25), sr_in, sr_out)
    level = rr.image_db(y, sr_out, f, f_image)
    print('image %d -> %d: tone %.0f Hz, image %.0f Hz (seen at %.0f Hz) at %.1f dB'
          % (sr_in, sr_out, f, sr_in - f, f_image, level))
    assert level <= -90.0


@pytest.mark.parametrize('sr_in,sr_out', rr.PAIRS)
def test_zero_phase(sr_in, sr_out):
    L, M, _ = rr.ratio(sr_in, sr_out)
    n_in = 200 * M + 7
    for m0 in (100 * M, 100 * M + 1, 97 * M + M // 2 + 1):      # m0 L / M an integer, and two that are not
        x = np.zeros(n_in)
        x[m0] = 1.0
        y, _, _ = rr.resample_at(x, sr_in, sr_out)
        centre = m0 * L / M
        peak = int(np.argmax(np.abs(y)))
        # (half-way cases may peak on either neighbour)
        assert abs(peak - centre) <= 0.5 + 1e-9, (m0, peak, centre)
        if (m0 * L) % M == 0:
            c = m0 * L // M
            assert peak == c == round(centre)
            k = min(c, len(y) - 1 - c)
            assert k > rr.Z and np.array_equal(y[c - k:c], y[c + 1:c + k + 1][::-1])


def test_host_errors_need_no_gpu():
    from amt_saga import audio
    with pytest.raises(ValueError):
        audio.Resampler(44100, 48001)                          # R = 48001 > 2048
    for bad in ((0, 44100), (44100, 0), (-8000, 44100), (44100.5, 48000)):
        with pytest.raises(ValueError):
            audio.Resampler(*bad)
        with pytest.raises(ValueError):
            audio.resample(np.zeros(16, np.float32), *bad)
    with pytest.raises(ValueError):
        audio.Resampler(44100, 44100)                          # the filter would still low-pass: resample() passes through
    with pytest.raises(ValueError):
        audio.resample(np.zeros(16, np.float32), 44100, 48001)
    rs = audio.Resampler(48000, 44100)
    assert rs._handles == {}                                   # nothing built yet
    for bad in (np.zeros((100, 9), np.float32), np.zeros(0, np.float32), np.zeros((0, 2), np.float32),
                np.zeros((4, 4, 4), np.float32), [], [np.zeros(8, np.float32), np.zeros((8, 2), np.float32)]):
        with pytest.raises(ValueError):
            rs(bad)
    for bad in (np.zeros((100, 9), np.float32), np.zeros(0, np.float32)):
        with pytest.raises(ValueError):
            audio.resample(bad, 44100, 44100)                  # equal rates check the signal too
        with pytest.raises(ValueError):
            audio.resample(bad, 48000, 44100)
    assert rs._handles == {}


def test_float32_restatement_stays_inside_the_bar():
    """The bar of the GPU tests is not loose by accident and not out of reach: the kernel's arithmetic restated in
    float32 on the CPU stays below a fifth of it on the GPU test's own kind of input."""
    rng = np.random.default_rng(5)
    for sr_in, sr_out in rr.PAIRS[:2] + [rr.STEEP]:
        x = rng.standard_normal(2000).astype(np.float32)
        x[0] = x[-1] = 8.0
        y, scale, taps = rr.resample_at(x, sr_in, sr_out)
        ratio = np.abs(rr.resample_f32(x, sr_in, sr_out) - y) / rr.bar(scale, taps)
        print('float32 restatement %d -> %d: %.3f of the bar' % (sr_in, sr_out, ratio.max()))
        assert ratio.max() < 0.2
        # a wrong tap misses it by orders of magnitude: the same signal one input sample late
        late, _, _ = rr.resample_at(np.concatenate([[0.0], x[:-1]]), sr_in, sr_out)
        assert (np.abs(late - y) / rr.bar(scale, taps)).max() > 1e4
