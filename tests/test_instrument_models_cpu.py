"""CPU: the instrument-model table of the loop, the host tone-bin table and the oracle subclasses that stand for the
ten models (tests/instrument_models_oracle.py) -- tied to tests/features_reference.py and to the reference's recorded
vectors, so that the GPU parity tests compare the product with something pinned."""
import numpy as np
import pytest

import features_reference as fr              # tests/features_reference.py
import instrument_models_oracle as imo       # tests/instrument_models_oracle.py
from oracle import audio as oa

# training.py:466-477 (the names), :76-98 (gen_model: the variant) and thread_training's feeds (the towers), written out
EXPECTED = {
    'instrument': ('instrument', ('C_sw_inst',)),
    'instrument_focused_lin': ('instrument_focused', ('F_sw_inst_foc',)),
    'instrument_focused_lin_log10': ('instrument_focused', ('F_sw_inst_foc_log10',)),
    'instrument_focused_const_lin': ('instrument_focused_const', ('F_sw_inst_foc_const',)),
    'instrument_focused_const_lin_log10': ('instrument_focused_const', ('F_sw_inst_foc_const_log10',)),
    'instrument_dual_lin': ('instrument_dual', ('C_sw_inst', 'F_sw_inst_foc')),
    'instrument_dual_lin_phase': ('instrument_dual', ('F_sw_inst_foc', 'ph')),
    'instrument_focused': ('instrument_focused', ('C_sw_inst_foc',)),
    'instrument_focused_const': ('instrument_focused_const', ('C_sw_inst_foc_const',)),
    'instrument_dual': ('instrument_dual', ('C_sw_inst', 'C_sw_inst_foc')),
}


def test_model_table_matches_the_reference_list():
    from amt_saga import loop
    from amt_saga.hyperparams import Hyperparams
    assert loop.INSTRUMENT_MODELS == EXPECTED and imo.MODELS == EXPECTED
    assert list(loop.INSTRUMENT_MODELS) == list(EXPECTED)                  # the reference's order
    p = Hyperparams(N=2048, window_size_note_time=1)
    for bad in ('instrument_focused_log10', 'Instrument', '', None):
        with pytest.raises(ValueError, match='Invalid Variant Selected'):
            loop.TranscriptionLoop(p, heads=('instrument',), instrument_model=bad)
    for name, (variant, towers) in EXPECTED.items():
        lp = loop.TranscriptionLoop(p, heads=('instrument',), instrument_model=name)
        net = lp.nets['instrument']
        assert list(lp.nets) == ['instrument']
        assert net.checkpoint_prefix == 'checkpoint_' + name and net.variant == variant
        assert len(net.cfg['input_shapes']) == len(towers) == (2 if variant == 'instrument_dual' else 1)
        assert all(tuple(s) == (p.instrument_bands, p.instrument_frames, 1) for s in net.cfg['input_shapes'])
        assert lp.instrument_inputs == towers
        # the normalisers and spectra the towers read, and no other
        keys = [k for k, _ in lp.normalisers]
        assert ('ref_C_inst' in keys) == ('C_sw_inst' in towers)
        assert ('ref_C_foc' in keys) == any(t.startswith('C_sw_inst_foc') for t in towers)
        assert lp.needs_phase == ('ph' in towers)
        assert lp.needs_wave == any(t.startswith('C_') for t in towers)
    # the default is the plain CQT model, and a loop without the instrument head reads no tower
    assert loop.TranscriptionLoop(p, heads=('instrument',)).instrument_model == 'instrument'
    lp = loop.TranscriptionLoop(p, heads=('timing', 'pitch', 'velocity'), instrument_model='instrument_dual')
    assert lp.instrument_inputs == () and [k for k, _ in lp.normalisers] == ['ref_C_1', 'ref_C_foc']


@pytest.mark.parametrize('n_fft', (2048, 4096))
def test_tone_bin_table_is_midi_tone_to_fft(refvec, n_fft):
    from amt_saga import audio as pa
    from amt_saga.hyperparams import Hyperparams
    p = Hyperparams(N=n_fft)
    tab = pa.tone_bin_table(p.sr, n_fft, p.pitch_low, p.pitch_high)
    assert tab.dtype == np.int32 and tab.shape == (p.pitch_high - p.pitch_low + 1,)
    ac = pa.audio_complete(np.zeros(4 * p.H, np.float32), n_fft)
    want = [ac.midi_tone_to_FFT(t) for t in range(p.pitch_low, p.pitch_high + 1)]
    assert np.array_equal(tab, want)
    assert np.array_equal(tab, refvec['tone2fft_%d' % n_fft][p.pitch_low:p.pitch_high + 1])


def _window(p, seed):
    rng = np.random.default_rng(seed)
    L = p.H * (p.timing_frames - 1)
    t = np.arange(L) / p.sr
    w = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in
            zip(rng.uniform(0.05, 0.3, 6), rng.uniform(100, 5000, 6), rng.uniform(0, 6, 6)))
    return (w + 0.01 * rng.standard_normal(L)).astype(np.float32)


@pytest.mark.parametrize('n_fft,wsec,pitch,onset,end', [(2048, 1, 60, 10, 31), (2048, 1, 21, 80, 86), (2048, 1, 108, 3, 8),
                                                        (4096, 2, 72, 5, 5), (4096, 2, 108, 0, 86)])
def test_oracle_fft_features_are_short_window(refvec, n_fft, wsec, pitch, onset, end):
    """The subclass's FFT-side towers (resize -> section_power -> scalings, the reference's composition) against
    features_reference.short_window in its three modes on the same window, and its tone bins against the vectors the
    reference recorded (those of test_oracle_golden.py::test_frame_maps_and_tone_bins)."""
    from oracle.params import HyperparamsOracle
    p = HyperparamsOracle(N=n_fft, window_size_note_time=wsec)
    orc = imo.ModelLoopOracle(p, ('instrument',), {}, model='instrument_dual_lin_phase')
    ac = oa.AudioCompleteOracle(_window(p, n_fft + pitch), p.N, p.H)
    mag, ph = np.asarray(ac.mag), np.asarray(ac.ph)
    F, T = mag.shape
    ref_mag = 0.37
    got = orc.fft_features(ac, onset, end, pitch, ref_mag)
    tone2fft = refvec['tone2fft_%d' % n_fft]
    assert ac.midi_tone_to_FFT(pitch) == tone2fft[pitch] and ac.midi_tone_to_FFT(imo.CONST_TONE) == tone2fft[60]
    m_tm = np.ascontiguousarray(mag.T)[None]                            # frame-major [1][T][F]
    p_tm = np.stack([ph.T.real, ph.T.imag], axis=-1)[None]
    tab = fr.resize_table([onset], [end], T, p.instrument_frames)
    ref = np.array([ref_mag])
    for suffix, tone in (('', pitch), ('_const', imo.CONST_TONE)):
        lo = np.array([tone2fft[tone]], np.int32)
        want0 = fr.short_window(m_tm, None, T, F, tab, lo, p.instrument_bands, ref, 0)[0]
        want1 = fr.short_window(m_tm, None, T, F, tab, lo, p.instrument_bands, None, 1)[0]
        assert np.array_equal(got['F_sw_inst_foc' + suffix], want0)
        assert np.array_equal(got['F_sw_inst_foc%s_log10' % suffix], want1, equal_nan=True)
        assert got['_zero_tile' + suffix] == bool(np.isnan(want1).any())
    want2 = fr.short_window(None, p_tm, T, F, tab, np.array([tone2fft[pitch]], np.int32), p.instrument_bands, None, 2)[0]
    # the oracle's ph is complex64, as the reference's (librosa.magphase of a float32 STFT): np.angle, the sum and the
    # division round in float32 -- 1/2 ulp of an angle <= pi, of a sum <= 6.3 and of a quotient <= 1, under 4 u in all
    assert np.allclose(got['ph'], want2, rtol=0, atol=4 * fr.U)
    assert got['ph'].shape == (p.instrument_bands, p.instrument_frames)
    if end > onset:
        assert tone2fft[pitch] + p.instrument_bands <= F or np.all(got['F_sw_inst_foc'][F - tone2fft[pitch]:] == 0)


def test_oracle_subclasses():
    from oracle.loop import LoopOracle
    from song_oracle import SongOracle
    assert issubclass(imo.ModelLoopOracle, LoopOracle) and issubclass(imo.ModelSongOracle, SongOracle)
    assert imo.ModelSongOracle._detect is not SongOracle._detect
    import inspect
    assert 'model' in inspect.signature(imo.ModelLoopOracle.run_window).parameters


def test_default_model_keeps_the_six_argument_loop_factory(monkeypatch):
    """transcribe() and the song queue build the default model's loop through _make_loop(p, iters, heads, groups,
    weights_dir, guess) -- the call other code wraps -- and name the model by keyword for the other nine."""
    from amt_saga import transcribe as tr
    calls = []

    class Stop(Exception):
        pass

    def factory(*a, **kw):
        calls.append((len(a), kw))
        raise Stop
    monkeypatch.setattr(tr, '_make_loop', factory)
    for kw in ({}, {'instrument_model': 'instrument_dual'}):
        with pytest.raises(Stop):
            tr.transcribe(np.zeros(8, np.float32), **kw)
        with pytest.raises(Stop):
            list(tr.iter_transcribe_songs([np.zeros(8, np.float32)], **kw))
    assert calls == [(6, {}), (6, {}), (6, {'instrument_model': 'instrument_dual'}),
                     (6, {'instrument_model': 'instrument_dual'})]
