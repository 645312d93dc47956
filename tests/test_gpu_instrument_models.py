"""GPU: the transcription loop, the song walk and the driver with each of the reference's instrument models
(TranscriptionLoop(instrument_model=), training.py:466-477) against the CPU oracles of
tests/instrument_models_oracle.py.

Policy: oracle/compare.py's -- integer events bit for bit, the heads' pre-rounding floats inside their bands, the
residual to 1e-4, every window compared, a decision inside the band of a rounding tie handed to the oracle.  The
'instrument' band is compare.FLOAT_TOL's 1e-4 unless the oracle ALONE shows that to be too tight for a model: the oracle
is run with float32 and with float64 networks on the test's windows, and where 2.5 x the largest distance between the
two runs' probabilities exceeds 1e-4 that product is the model's band (2.5: the margin tests/test_gpu_rdcnn.py grants
another evaluation order against numpy-float32's own distance from float64).  The distance and the band are printed.
Conditions asserted on the oracle's side: every step has end > onset, no element of a `ph` tower within 1e-4 rad of
+-pi (the angle jumps by 2 pi there), no all-zero log10 tile (0 / 0)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instrument_models_oracle as imo                            # noqa: E402
import song_oracle as so                                          # noqa: E402
from oracle import synth as osynth                                # noqa: E402
from oracle.compare import bands_for, compare_windows             # noqa: E402

pytestmark = pytest.mark.gpu

HEADS = ('timing', 'pitch', 'instrument')
GROUPS = (0, 1, 2)
MODELS = [m for m in imo.MODELS if m != 'instrument']
# the seed of a model's windows, chosen so that the conditions below hold on the oracle's side (screened with the oracle
# alone).  A `ph` tower holds 348 x 8 angles per step: one within 1e-4 rad of +-pi somewhere in twelve steps is more
# likely than not, so that model has a seed of its own.
SEED = 64
SEEDS = {'instrument_dual_lin_phase': 71}


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import synth, loop, hyperparams
    return dict(torch=torch, synth=synth, loop=loop, hp=hyperparams)


def windows(p, B, seed=SEED):
    """B oracle-sized windows: seeded note lists of the three instrument groups through the float64 synthesiser
    restatement over a seeded noise floor 60 dB below full scale (a rendered note starts and ends in digital silence,
    and a band of exact zeros is the 0 / 0 log10 tile the conditions exclude), as 24-bit PCM values (exact in float32,
    the same on every machine)."""
    from amt_saga import synth
    L = p.H * (p.timing_frames - 1)
    notes = synth.window_notes(B, seed, (1, 3), GROUPS, 0.4 * p.window_size_note_time)
    w = osynth.render_notes(notes, L, p.sr).astype(np.float64)
    w = w + 1e-3 * np.random.default_rng(seed).standard_normal((B, L))
    return (np.clip(np.rint(w * 8388608.0), -8388608, 8388607) / 8388608.0).astype(np.float32)


def prog_group(p):
    from amt_saga import synth
    remap = np.zeros(3, np.int32)
    for i, g in enumerate(GROUPS):
        remap[g] = i
    return remap[synth.prog_group_table(p.instrument_classes)]


def oracle_probability_distance(make, waves, refs):
    """The largest |float32 run - float64 run| of the instrument probabilities over the windows' steps, oracle alone.
    make(dtype) -> ModelLoopOracle.  Steps after the two runs part at a rounding tie are not counted (they no longer
    see the same residual)."""
    o32, o64 = make(np.float32), make(np.float64)
    dist = 0.0
    for i in range(len(waves)):
        r = {k: float(v[i]) for k, v in refs.items()}
        o32.run_window(waves[i], r, i)
        o64.run_window(waves[i], r, i)
        for a, c in zip(o32.decisions, o64.decisions):
            if a[0] == 'instrument':
                dist = max(dist, float(np.abs(np.asarray(a[2], np.float64) - np.asarray(c[2], np.float64)).max()))
            if a[4] != c[4]:
                break
    return dist


def instrument_band(dist):
    return max(1e-4, 2.5 * dist)


def assert_conditions(orc, towers):
    c = orc.conditions
    assert c['steps'] > 0 and c['empty_steps'] == 0, c
    if 'ph' in towers:
        assert c['min_pi_distance'] > 1e-4, c
    assert c['zero_log_tiles'] == 0, c


@pytest.mark.parametrize('model', MODELS)
def test_loop_vs_oracle_per_model(env, model):
    """timing + pitch + instrument heads, 2 iterations, B = 6 oracle-sized windows: every window compared."""
    torch = env['torch']
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    B, iters = 6, 2
    waves = windows(p, B, SEEDS.get(model, SEED))
    lp = env['loop'].TranscriptionLoop(p, heads=HEADS, iters=iters, groups=GROUPS, instrument_model=model).setup_device()
    lp.trace = []
    events, b = lp.run(torch.from_numpy(waves).cuda(), window0=100)
    trace, lp.trace = [{k: v.cpu().numpy() for k, v in t.items()} for t in lp.trace], None
    ev = events.cpu().numpy()
    assert ev.shape == (iters, B, 7) and len(trace) == iters and set(trace[0]) == {'timing_start', 'timing_end', 'pitch',
                                                                                   'instrument'}
    refs = {k: v.cpu().numpy() for k, v in lp.refs.items()}
    towers = imo.MODELS[model][1]
    assert ('ref_C_inst' in refs) == ('C_sw_inst' in towers)
    assert ('ref_C_foc' in refs) == any(t.startswith('C_sw_inst_foc') for t in towers)
    weights = {k: n.weights for k, n in lp.nets.items()}
    bank = osynth.guess_bank_waves(GROUPS, p.pitch_low, p.pitch_high, sr=p.sr)
    memo = {}

    def make(dtype):
        o = imo.ModelLoopOracle(p, HEADS, weights, iters=iters, prog_group=prog_group(p), bank_waves=bank, dtype=dtype,
                                model=model)
        o._cqt_memo = memo
        return o
    dist = oracle_probability_distance(make, waves, refs)
    bands = dict(bands_for(p))
    bands['instrument'] = instrument_band(dist)
    orc = make(np.float32)
    diffs = {}
    clean, ties, forced = compare_windows(orc, waves, refs, ev, trace, b.mag.cpu().numpy(), b.ref_max.cpu().numpy(), bands,
                                          window0=100, diffs=diffs)
    assert clean + ties == B
    assert_conditions(orc, towers)
    programs = len(np.unique(ev[:, :, 3]))
    print('model %s: oracle float32 - float64 probabilities %.3g -> instrument band %.3g; product - oracle %.3g; '
          '%d distinct programs; %d windows compared, %d near a tie, %d decisions handed over; conditions %s'
          % (model, dist, bands['instrument'], max(diffs['instrument']), programs, B, ties, forced, orc.conditions))
    assert np.all(ev[:, :, 3] >= 0) and np.all(ev[:, :, 6] > ev[:, :, 5])


@pytest.mark.parametrize('model', ('instrument_focused_lin', 'instrument_dual'))
def test_song_walk_per_model(env, model):
    """run_songs on two songs of three half windows each against the SongOracle subclass, in the manner of
    tests/test_gpu_song_loop.py::test_walk_vs_cpu_restatement."""
    torch = env['torch']
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    max_notes, silence = 2, 1e-4
    lp = env['loop'].TranscriptionLoop(p, heads=HEADS, groups=GROUPS, instrument_model=model).setup_device()
    songs = so.make_songs(p, 17, (3.0, 3.0))
    lp.trace = []
    events, state = lp.run_songs(songs, max_notes=max_notes, silence=silence, poll=4, song0=3)
    torch.cuda.synchronize()
    trace, lp.trace = [{k: v.cpu().numpy() for k, v in t.items()} for t in lp.trace], None
    ev = events.cpu().numpy()
    steps, B = ev.shape[0], len(songs)
    assert ev.shape == (steps, B, 9) and state.finished.cpu().tolist() == [1] * B
    towers = imo.MODELS[model][1]
    assert set(state.refs) == {'ref_mag', 'ref_C_1'} | ({'ref_C_inst'} if 'C_sw_inst' in towers else set()) | \
        ({'ref_C_foc'} if 'C_sw_inst_foc' in towers else set())
    bank = osynth.guess_bank_waves(GROUPS, p.pitch_low, p.pitch_high, sr=p.sr)
    orc = imo.ModelSongOracle(p, HEADS, {k: n.weights for k, n in lp.nets.items()}, prog_group=prog_group(p),
                              bank_waves=bank, model=model)
    bands = bands_for(p)
    refs = {k: v.cpu().numpy() for k, v in state.refs.items()}
    mags = state.batch.mag.cpu().numpy()
    half, tf, F = p.timing_frames // 2, p.timing_frames, p.N // 2 + 1
    forced = live = detects = 0
    for i in range(B):
        r = {k: float(v[i]) for k, v in refs.items()}
        ev_ref, mag_ref = orc.run_song(songs[i], r, max_notes, silence, song_id=3 + i, force=(ev[:, i, :], bands))
        for name, it, y, margin, v, was_forced in orc.decisions:
            dlt = float(np.abs(np.asarray(trace[it][name][i], np.float64).ravel() - np.asarray(y, np.float64).ravel()).max())
            assert dlt <= bands[name], ('float', i, name, it, dlt, bands[name])
            forced += was_forced
        live += len(ev_ref)
        want = so.pad_finished(ev_ref, steps, 3 + i, half)
        assert np.array_equal(ev[:, i, :], want), ('events', i, ev[:, i, :].tolist(), want.tolist())
        detects += int(np.sum(want[:, 2] == so.DETECT))
        scale = max(float(mag_ref.max()), 1e-30)
        assert np.abs(mags[i][:, :F].T - mag_ref[:, :tf]).max() / scale < 1e-4, ('residual', i)
    assert_conditions(orc, towers)
    print('walk %s: %d steps x %d songs, %d live, %d detections, %d decisions handed over' % (model, steps, B, live, detects,
                                                                                           forced))
    assert detects > 0 and forced * 10 <= live, (detects, forced, live)


def test_driver_and_command_line(env, tmp_path, monkeypatch):
    """transcribe(instrument_model=) on a 2-window signal gives the events of the loop run directly on its windows and
    whole-song normalisers; --instrument-model reaches the loop in both command-line modes, and --weights looks for
    <model name>.npz."""
    torch = env['torch']
    from amt_saga import flac, transcribe as tr
    model = 'instrument_dual_lin_phase'
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    L = p.H * (p.timing_frames - 1)
    wf = osynth.render_window([(0, 60, 100, 0.2, 0.4), (1, 67, 90, 0.9, 0.3)], L + L // 2, p.sr).numpy().astype(np.float32)
    heads = ('timing', 'pitch', 'instrument', 'velocity')
    notes, evs = tr.transcribe(wf, p, iters=2, heads=heads, instrument_model=model)
    wins, starts = tr.cut_windows(wf, L, L // 2)
    assert len(starts) == 2 and evs.shape == (2, 2, 7)
    lp = env['loop'].TranscriptionLoop(p, heads=heads, iters=2, groups=(0, 1, 2), instrument_model=model).setup_device()
    levels = lp.song_levels(torch.from_numpy(wf).cuda())
    assert set(levels) == {'ref_mag', 'ref_C_1', 'ref_C_foc'}            # no tower reads C_sw_inst; velocity reads ref_C_foc
    direct, _ = lp.run(torch.from_numpy(wins).cuda(), refs={k: v.expand(2).contiguous() for k, v in levels.items()})
    assert np.array_equal(direct.cpu().numpy(), evs)
    with pytest.raises(ValueError, match='Invalid Variant Selected'):
        tr.transcribe(wf, p, iters=1, heads=heads, instrument_model='instrument_lin')
    # the command line, both modes: the loop it builds, and the weight file it looks for
    built, looked = [], []

    class Recording(tr.TranscriptionLoop):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self.instrument_model)
    monkeypatch.setattr(tr, 'TranscriptionLoop', Recording)
    real_exists = os.path.exists
    monkeypatch.setattr(tr.os.path, 'exists', lambda f: (looked.append(os.path.basename(f)), real_exists(f))[1])
    path = str(tmp_path / 'clip.flac')
    flac.save_float(wf, path, p.sr)
    wdir = str(tmp_path / 'weights')
    os.makedirs(wdir)
    tr.main([path, str(tmp_path / 'one.mid'), '--iters', '1', '--instrument-model', model, '--weights', wdir])
    assert built == [model] and model + '.npz' in looked and 'instrument.npz' not in looked
    tr.main(['--songs', path, '--out-dir', str(tmp_path / 'out'), '--iters', '1', '--slots', '1',
             '--instrument-model', 'instrument_focused_const_lin'])
    assert built == [model, 'instrument_focused_const_lin']
    tr.main([path, str(tmp_path / 'two.mid'), '--iters', '1', '--weights', wdir])
    assert built[-1] == 'instrument' and 'instrument.npz' in looked
    assert os.path.getsize(str(tmp_path / 'one.mid')) > 20 and os.path.getsize(str(tmp_path / 'out' / 'clip.mid')) > 20
    with pytest.raises(SystemExit):
        tr.main([path, str(tmp_path / 'x.mid'), '--instrument-model', 'nope'])
