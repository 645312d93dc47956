"""GPU: amt_note_features (the FFT-side instrument towers of a step in one launch) through the C ABI against
amt_short_window -- bit for bit per mode with band_min[b] = tone_bin[clamp(pitch[b])] -- and against the numpy
restatement of tests/features_reference.py; and the focused CQT grid of the loop through amt_cqt_slices against
oracle.cqt.cqt_frames.

Bars, those of tests/test_gpu_features_geometry.py for short_window (u = 2^-24):
  * lin (mode 0): bit for bit the float32 reference (one correctly rounded division).
  * log10, phase (modes 1 / 2) rest on the device's log10f / atan2f: e_gpu <= 2.5 e_f32numpy + 4 u scale per window, both
    errors measured against the float64 run on the same float32 inputs.
Conditions on the inputs, asserted on the float64 side: no phase within 1e-3 rad of +-pi (the angle jumps by 2 pi
there), no all-zero log10 tile (0 / 0: the reference gives NaN there too).
Set-up as in that file: NaN in the pad bins and the gap rows of the spectra, outputs filled with -7 and everything
outside the documented extent asserted to hold it still."""
import itertools

import numpy as np
import pytest

import features_reference as fr      # tests/features_reference.py

pytestmark = pytest.mark.gpu

SENT = fr.SENT
TONE_LO, TONE_HI = 21, 108
SHAPES = ((348, 8), (4, 1), (36, 8))                 # (bands, frames): the loop's tile, one element per lane, velocity-sized
KINDS = ('lin', 'log10', 'phase')


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import _lib, audio
    return dict(torch=torch, lib=_lib.load(), _lib=_lib, audio=audio)


def _p(t):
    return None if t is None else t.data_ptr()


def _up(env, a):
    return None if a is None else env['torch'].from_numpy(np.ascontiguousarray(a)).cuda()


def _sent(env, n):
    return env['torch'].full((n,), SENT, device='cuda', dtype=env['torch'].float32)


def _fetch(env, buf, n):
    env['torch'].cuda.synchronize()
    o = buf.cpu().numpy()
    assert np.all(o[n:] == SENT), 'written past the documented extent'
    return o[:n]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_transcendental(what, got, ref64, ref32):
    e_gpu, e_32, scale = fr.window_errors(got, ref64), fr.window_errors(ref32, ref64), fr.window_scales(ref64)
    bar = fr.transcendental_bar(e_32, scale)
    w = int(np.argmax(e_gpu / np.maximum(bar, 1e-300)))
    print('%-60s window %d e_gpu %.3g e_f32numpy %.3g bar %.3g' % (what, w, e_gpu[w], e_32[w], bar[w]))
    assert np.all(e_gpu <= bar), (what, e_gpu.tolist(), bar.tolist())


def _inputs(B, T, F, seed):
    """(mag, phase): fr.spectra / fr.phases, F = 257 at ldf 260 (no pad beyond the alignment), the axis points of
    fr.phases (they hold -1 = the angle pi) replaced by angles inside the condition."""
    pad = 0 if F == 257 else 8
    m, ph = fr.spectra(B, T, F, seed, kind='mag', pad=pad), fr.phases(B, T, F, seed + 1, pad=pad)
    a = np.random.default_rng(seed + 2).uniform(-3.0, 3.0, (B, 5))
    ph[:, 0, 12:17, 0], ph[:, 0, 12:17, 1] = np.cos(a), np.sin(a)
    ang = np.arctan2(ph[:, :T, :F, 1].astype(np.float64), ph[:, :T, :F, 0].astype(np.float64))
    assert np.all(np.pi - np.abs(ang) > 1e-3)
    assert m.shape[2] == (260 if F == 257 else fr.ldf_of_bins(F) + 8)
    return m, ph


def _table(B, T, frames, seed):
    """[B][frames]: valid frames; with more than one frame every third window holds a -1 and every third an index >= T
    (each window keeps a valid frame, so no log10 tile is all zero)."""
    rng = np.random.default_rng(seed)
    tab = rng.integers(0, T, (B, frames)).astype(np.int32)
    if frames > 1:
        for b in range(B):
            if b % 3 == 0:
                tab[b, b % frames] = -1
            elif b % 3 == 1:
                tab[b, b % frames] = T + b % 2
            tab[b, (b + 1) % frames] = b % T
    return tab


def _pitches(B, seed):
    """Pitch arrays that together hold both clamps (below and above the table), and None = the constant tone."""
    rng = np.random.default_rng(seed)
    if B == 1:
        return [np.array([TONE_LO - 9], np.int32), np.array([TONE_HI + 90], np.int32), None]
    p = rng.integers(TONE_LO, TONE_HI + 1, B).astype(np.int32)
    p[0], p[1], p[2], p[-1] = TONE_LO - 9, TONE_HI + 90, TONE_LO, TONE_HI
    return [p, None]


@pytest.mark.parametrize('B,F', [(B, F) for F in (257, 1025, 2049) for B in (1, 3, 300)])
def test_note_features_vs_short_window_and_float64(env, B, F):
    lib, L, torch = env['lib'], env['_lib'], env['torch']
    T = 9
    m, ph = _inputs(B, T, F, 100 * F + B)
    ldf = m.shape[2]
    ss = (T + 2) * ldf
    d_m, d_ph = _up(env, m), _up(env, ph)
    ref = np.random.default_rng(B).uniform(0.5, 2.0, B).astype(np.float32)
    d_ref = _up(env, ref)
    tone_bin = env['audio'].tone_bin_table(44100, 2 * (F - 1), TONE_LO, TONE_HI)
    d_tb = _up(env, tone_bin)
    n_tones = len(tone_bin)
    for bands, frames in SHAPES:
        tab = _table(B, T, frames, bands + frames)
        d_tab = _up(env, tab)
        n = B * bands * frames
        for pitch in _pitches(B, F + bands):
            tone = np.full(B, 60) if pitch is None else pitch
            lo = tone_bin[np.clip(tone - TONE_LO, 0, n_tones - 1)].astype(np.int32)
            if F == 257:
                assert np.any(lo + bands > F) or bands < 348            # bands that run past F: zero padding
            d_lo, d_pitch = _up(env, lo), _up(env, pitch)
            geom = 'B %d F %d bands %d frames %d pitch %s' % (B, F, bands, frames, 'NULL' if pitch is None else 'array')
            # what amt_short_window writes in the three modes
            sw = {}
            for mode, kind in enumerate(KINDS):
                out = _sent(env, n + 3)
                assert lib.amt_short_window(_p(d_m) if mode != 2 else None, _p(d_ph) if mode == 2 else None, B, T, F, ldf,
                                            ss, _p(d_tab), frames, _p(d_lo), bands, _p(d_ref) if mode == 0 else None, mode,
                                            _p(out), None) == L.AMT_OK
                sw[kind] = _fetch(env, out, n)
            for want in itertools.chain.from_iterable(itertools.combinations(KINDS, k) for k in (1, 2, 3)):
                outs = {k: _sent(env, n + 3) for k in want}
                st = lib.amt_note_features(_p(d_m), _p(d_ph), B, T, F, ldf, ss, _p(d_tab), frames, _p(d_pitch), 60, _p(d_tb),
                                           TONE_LO, n_tones, bands, _p(d_ref), _p(outs.get('lin')), _p(outs.get('log10')),
                                           _p(outs.get('phase')), None)
                assert st == L.AMT_OK, (geom, want, st)
                for k in want:
                    got = _fetch(env, outs[k], n)
                    assert np.array_equal(_bits(got), _bits(sw[k])), (geom, want, k)
            # (the last subset held all three) against the references
            shape = (B, bands, frames)
            r32 = fr.short_window(m, ph, T, F, tab, lo, bands, ref, 0, np.float32)
            assert np.array_equal(_bits(sw['lin'].reshape(shape)), _bits(r32)), geom
            for mode, kind in ((1, 'log10'), (2, 'phase')):
                r64 = fr.short_window(m, ph, T, F, tab, lo, bands, None, mode)
                assert not np.isnan(r64).any(), (geom, 'an all-zero log10 tile')
                _check_transcendental('%s %s' % (kind, geom), sw[kind].reshape(shape), r64,
                                      fr.short_window(m, ph, T, F, tab, lo, bands, None, mode, np.float32))


def test_note_features_argument_errors_launch_nothing(env):
    lib, L = env['lib'], env['_lib']
    B, T, F, bands, frames = 2, 3, 257, 4, 2
    m, ph = _inputs(B, T, F, 5)
    ldf = m.shape[2]
    d_m, d_ph = _up(env, m), _up(env, ph)
    d_tab, d_tb = _up(env, np.zeros((B, frames), np.int32)), _up(env, np.arange(88, dtype=np.int32))
    n = B * bands * frames
    o = [_sent(env, n) for _ in range(3)]

    def call(mag=d_m, phase=d_ph, B=B, T=T, F=F, ldf=ldf, tab=d_tab, frames=frames, tb=d_tb, n_tones=88, bands=bands,
             outs=(0, 1, 2)):
        return lib.amt_note_features(_p(mag), _p(phase), B, T, F, ldf, (T + 2) * ldf, _p(tab), frames, None, 60, _p(tb),
                                     TONE_LO, n_tones, bands, None, *[_p(o[i]) if i in outs else None for i in range(3)],
                                     None)
    for kw in (dict(outs=()), dict(tab=None), dict(tb=None), dict(B=0), dict(T=0), dict(frames=0), dict(bands=0),
               dict(n_tones=0)):
        assert call(**kw) == L.AMT_E_INVALID, kw
    for kw in (dict(ldf=F - 1), dict(F=0)):
        assert call(**kw) == L.AMT_E_SHAPE, kw
    for kw in (dict(mag=None, outs=(0,)), dict(mag=None, outs=(1, 2)), dict(phase=None, outs=(2,))):
        assert call(**kw) == L.AMT_E_ATTRIB, kw
    assert call(bands=4096, frames=8) == L.AMT_E_UNSUPPORTED          # a tile beyond a workgroup's LDS
    for buf in o:
        _fetch(env, buf, 0)                                             # every output still holds its sentinel
    assert call(mag=None, outs=(2,)) == L.AMT_OK and call(phase=None, outs=(0, 1)) == L.AMT_OK


@pytest.mark.parametrize('pitch', (21, 60, 108))
def test_focused_cqt_grid_vs_oracle(env, pitch):
    """amt_cqt_slices on the loop's focused grid (4 x instrument_bins_per_tone bins per semitone from pitch_low, Q about
    553: the lowest filters are longer than the window) with bin0 = the decided pitch's first bin, B = 3 oracle-sized
    windows, against oracle.cqt.cqt_frames on the same slice of the grid, at the bar of the CQT slice tests
    (test_gpu_rdcnn.py::test_cqt_slices: REL = 1e-4 of the slice's maximum)."""
    torch, audio = env['torch'], env['audio']
    from amt_saga.hyperparams import Hyperparams
    from amt_saga.loop import TranscriptionLoop
    from oracle import cqt as ocqt
    p = Hyperparams(N=2048, window_size_note_time=1)                    # 86 frames: the oracle-sized window
    lp = TranscriptionLoop(p, heads=('instrument',), instrument_model='instrument_focused').setup_device()
    bpt = 4 * p.instrument_bins_per_tone
    assert lp.foc_bpt == bpt and lp.tab_foc[0].shape[0] == bpt * (p.pitch_high - p.pitch_low) + p.instrument_bands
    B, L = 3, p.H * (p.timing_frames - 1)
    rng = np.random.default_rng(pitch)
    t = np.arange(L) / p.sr
    wave = np.stack([sum(a * np.sin(2 * np.pi * 440.0 * 2 ** ((pitch + d - 69) / 12) * t)
                         for a, d in zip(rng.uniform(0.1, 0.4, 4), (0, 0.37, 7, 12.2))) + 0.01 * rng.standard_normal(L)
                     for _ in range(B)]).astype(np.float32)
    src = np.stack([ocqt.slice_C_frames(p.timing_frames, s, e, p.pitch_frames) for s, e in ((0, 8), (40, 45), (80, 86))])
    bin0 = np.full(B, bpt * (pitch - p.pitch_low), np.int32)
    got = audio.cqt_slices(_up(env, wave), _up(env, src.astype(np.int32)), lp.tab_foc, p.instrument_bands, p.H,
                           bin0=_up(env, bin0)).cpu().numpy()
    inc, length, _ = ocqt.cqt_table(p.sr, float(audio.midi_to_hz(p.pitch_low)), lp.tab_foc[0].shape[0], 12 * bpt)
    b0 = int(bin0[0])
    assert length[0] > L and np.array_equal(lp.tab_foc[1].cpu().numpy(), length)
    for b in range(B):
        want = ocqt.cqt_frames(wave[b], src[b], inc[b0:b0 + p.instrument_bands], length[b0:b0 + p.instrument_bands], p.H)
        err = np.abs(got[b] - want).max()
        print('focused grid pitch %d window %d: max err / max %.3g' % (pitch, b, err / want.max()))
        assert err <= 1e-4 * max(want.max(), 1e-6), (pitch, b, err)
