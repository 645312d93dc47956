"""GPU parity of the composed detect -> subtract loop vs the CPU oracle loop:
predicted note events bit-exact (away from rounding ties), residual magnitudes
within 1e-4 of the window maximum; glue kernels vs numpy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import synth, loop, hyperparams, audio, _lib
    from oracle import loop as oloop, audio as oa
    return dict(torch=torch, synth=synth, loop=loop, hp=hyperparams, audio=audio, lib=_lib.load(),
                oloop=oloop, oa=oa)


def test_glue_kernels(env):
    torch, audio = env['torch'], env['audio']
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    lp = env['loop'].TranscriptionLoop(p, heads=(), iters=1)
    x = torch.tensor([[0.5], [1.5], [2.5], [-3.0], [99.7], [float('nan')], [2.4999]], device='cuda')
    assert lp._round(x, 0, 50).cpu().tolist() == [0, 2, 2, 0, 50, 0, 2]      # half-to-even, clamp, NaN
    pr = torch.tensor([[0.1, 0.7, 0.7], [0.3, 0.2, 0.1]], device='cuda')
    assert lp._argmax(pr).cpu().tolist() == [1, 0]                            # first maximum
    T = 40
    s = np.array([0, 5, 10, 38, 39, 40, 7, 3, 20], np.int32)
    e = np.array([0, 6, 13, 40, 45, 50, 3, 30, 28], np.int32)
    tab = lp._resize_table(torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda(), T, 8).cpu().numpy()
    from oracle.cqt import slice_C_frames
    for i in range(len(s)):
        assert np.array_equal(tab[i], slice_C_frames(T, int(s[i]), int(e[i]), 8)), i


# ---------------------------------------------------------------------------------------------------------------------
# the integer glue through the C ABI against the restatements of tests/features_reference.py
# (test_features_reference_cpu.py pins those); every comparison is exact
# ---------------------------------------------------------------------------------------------------------------------
def _glue(env):
    import features_reference as fr      # tests/features_reference.py
    from amt_saga import _lib
    torch = env['torch']
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()

    def ints(n):                                  # sentinel-filled int32 output with room behind it
        return torch.full((n + 3,), -7, dtype=torch.int32, device='cuda')

    def fetch(buf, n):
        torch.cuda.synchronize()
        o = buf.cpu().numpy()
        assert np.all(o[n:] == -7), 'written past the documented extent'
        return o[:n]
    return fr, _lib, env['lib'], up, ptr, ints, fetch


def test_resize_table_every_interval(env):
    """Every (s, t) in [-2, T + 2]^2 at T = 12 in one launch per frames = 3, 4, 8, 32: 17 x 17 = 289 windows, at 32 frames
    9248 entries in 37 workgroups, the last one partial.  That is the whole len 0 / < 3 / < frames / >= frames partition
    of _resize.  frames < 3 is refused."""
    fr, L, lib, up, ptr, ints, fetch = _glue(env)
    T = fr.RESIZE_T
    s, t = [a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(-2, T + 3), np.arange(-2, T + 3), indexing='ij')]
    n = len(s)
    assert n >= 256
    d_s, d_t = up(s), up(t)
    for frames in fr.RESIZE_FRAMES:
        out = ints(n * frames)
        assert lib.amt_resize_table(ptr(d_s), ptr(d_t), n, T, frames, ptr(out), None) == L.AMT_OK
        got = fetch(out, n * frames).reshape(n, frames)
        want = fr.resize_table(s, t, T, frames)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (frames, int(s[bad[0]]), int(t[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist())
    out = ints(n * 2)
    for frames in (2, 0, -1):
        assert lib.amt_resize_table(ptr(d_s), ptr(d_t), n, T, frames, ptr(out), None) == L.AMT_E_INVALID
    fetch(out, 0)


def test_round_clamp_edges(env):
    """n = 600 (three workgroups): halves of both parities and signs, lo and hi themselves, lo - 0.5 and hi + 0.5,
    +-inf, NaN, +-3e9, -0.0, among values spread over and beyond [lo, hi]; stride 1 and stride 3 over an [n, 3] tensor
    whose other columns would give other answers; lo == hi; lo > hi refused."""
    fr, L, lib, up, ptr, ints, fetch = _glue(env)
    n = 600
    rng = np.random.default_rng(12)
    for lo, hi in ((0, 50), (-7, 6), (21, 21)):
        x = rng.uniform(lo - 5, hi + 5, n).astype(np.float32)
        x[:200] = np.round(x[:200]) + rng.choice([-0.5, 0.5], 200)      # halves, both parities and signs
        special = [0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, lo, hi, lo - 0.5, hi + 0.5, lo + 0.5, hi - 0.5, np.inf,
                   -np.inf, np.nan, 3e9, -3e9, -0.0, 2.4999, 2.5001]
        x[300:300 + len(special)] = special
        x[-1], x[255], x[256] = np.nan, hi + 0.5, lo - 0.5              # the last thread, both sides of a workgroup edge
        want = fr.round_clamp(x, lo, hi)
        out, d_x = ints(n), up(x)
        assert lib.amt_round_clamp(ptr(d_x), n, 1, lo, hi, ptr(out), None) == L.AMT_OK
        got = fetch(out, n)
        assert np.array_equal(got, want), (lo, hi, x[got != want].tolist(), got[got != want].tolist())
        x3 = np.stack([x[::-1], x, np.full(n, np.nan, np.float32)], axis=1)
        d_x3 = up(x3)
        for col in range(2):
            out = ints(n)
            assert lib.amt_round_clamp(ptr(d_x3) + 4 * col, n, 3, lo, hi, ptr(out), None) == L.AMT_OK
            assert np.array_equal(fetch(out, n), fr.round_clamp(x3[:, col], lo, hi)), (lo, hi, col)
    out = ints(n)
    assert lib.amt_round_clamp(ptr(d_x), n, 1, 5, 4, ptr(out), None) == L.AMT_E_INVALID
    assert lib.amt_round_clamp(ptr(d_x), n, 0, 0, 4, ptr(out), None) == L.AMT_E_INVALID
    fetch(out, 0)


def test_argmax_rows_ties_inf_nan(env):
    """K = 1, 2, 88, 129 at n = 300 (two workgroups): ties at the first / a middle / the last class, rows of equal
    values, rows holding -inf and +inf, a row of NaNs (-> 0) and rows with one NaN at the first, a middle and the last
    class.  A NaN is never selected (the header's rule, not numpy's)."""
    fr, L, lib, up, ptr, ints, fetch = _glue(env)
    n = 300
    for K in (1, 2, 88, 129):
        rng = np.random.default_rng(K)
        p = rng.standard_normal((n, K)).astype(np.float32)
        mid = K // 2
        top = np.float32(9.0)
        p[0, [0, K - 1]] = top                                          # tie first / last
        p[1, [mid, K - 1]] = top                                        # tie middle / last
        p[2, [0, mid]] = top
        p[3] = 0.25                                                     # all equal
        p[4] = -np.inf                                                  # all -inf
        p[5] = -np.inf
        p[5, K - 1] = -1e30                                             # one number behind -inf
        p[6, mid] = np.inf
        p[7] = np.nan                                                   # a row of NaNs
        p[8, 0] = np.nan                                                # one NaN: first, middle, last
        p[9, mid] = np.nan
        p[10, K - 1] = np.nan
        p[11] = np.nan
        p[11, K - 1] = -np.inf                                          # NaNs, then -inf: the -inf is the choice
        p[12, 0], p[12, K - 1] = np.nan, top
        p[256:268] = p[:12]                                             # the same in the second workgroup
        p[299] = p[8]
        want = fr.argmax_rows(p)
        clean = ~np.isnan(p).any(axis=1)
        assert np.array_equal(want[clean], p[clean].argmax(axis=1))
        out, d_p = ints(n), up(p)
        assert lib.amt_argmax_rows(ptr(d_p), n, K, ptr(out), None) == L.AMT_OK
        got = fetch(out, n)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (K, bad.tolist(), got[bad].tolist(), want[bad].tolist())
        chosen = p[np.arange(n), got]
        assert not np.isnan(chosen[~np.isnan(p).all(axis=1)]).any()


def test_note_select_clamps(env):
    """n = 300: programs -1, 0 .. n_prog + 3 with and without a prog_group table and with program NULL; pitches below
    pitch_lo and at / above pitch_lo + n_pitch; end < onset; end - onset + tail above bank_frames."""
    fr, L, lib, up, ptr, ints, fetch = _glue(env)
    n, n_prog, pitch_lo, n_pitch, tail, bank = 300, 5, 21, 88, 43, 173
    rng = np.random.default_rng(3)
    program = rng.integers(-1, n_prog + 4, n).astype(np.int32)
    pitch = rng.integers(pitch_lo - 4, pitch_lo + n_pitch + 4, n).astype(np.int32)
    onset = rng.integers(0, 200, n).astype(np.int32)
    end = (onset + rng.integers(-50, 200, n)).astype(np.int32)
    program[:3], program[-3:] = (-1, 0, n_prog + 3), (n_prog + 3, -1, n_prog)
    pitch[:4] = (pitch_lo - 1, pitch_lo, pitch_lo + n_pitch - 1, pitch_lo + n_pitch)
    pitch[-2:] = (pitch_lo + n_pitch + 3, pitch_lo - 4)
    onset[4:8], end[4:8] = (10, 10, 0, 100), (9, 10, bank - tail, 100 + bank - tail + 1)
    group = np.array([2, 0, 1, 1, 3], np.int32)
    assert (end < onset).any() and (end - onset + tail > bank).any()
    for prog, grp in ((program, group), (program, None), (None, group), (None, None)):
        gi, gf = ints(n), ints(n)
        d = [up(a) for a in (prog, pitch, onset, end, grp)]
        st = lib.amt_note_select(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), n_prog, n,
                                 pitch_lo, n_pitch, tail, bank, ptr(gi), ptr(gf), None)
        assert st == L.AMT_OK
        wi, wf = fr.note_select(prog, pitch, onset, end, grp, n_prog, pitch_lo, n_pitch, tail, bank)
        assert np.array_equal(fetch(gi, n), wi) and np.array_equal(fetch(gf, n), wf), (prog is None, grp is None)
        assert wi.min() >= 0 and wi.max() < (4 if grp is not None else 1) * n_pitch and wf.min() >= tail and wf.max() == bank


def test_pack_events_and_affine(env):
    """pack_events at n = 300 with window0 and iter non-zero: all five columns, then each of them NULL in turn (-1);
    affine_i32 with a negative multiplier."""
    fr, L, lib, up, ptr, ints, fetch = _glue(env)
    n = 300
    rng = np.random.default_rng(4)
    cols = [rng.integers(0, 500, n).astype(np.int32) for _ in range(5)]
    d_cols = [up(c) for c in cols]
    for drop in (None, 0, 1, 2, 3, 4):
        out = ints(n * 7)
        args = [None if c == drop else ptr(d_cols[c]) for c in range(5)]
        assert lib.amt_pack_events(n, 1000, 3, *args, ptr(out), None) == L.AMT_OK
        want = fr.pack_events(n, 1000, 3, *[None if c == drop else cols[c] for c in range(5)])
        assert np.array_equal(fetch(out, n * 7).reshape(n, 7), want), drop
    x = rng.integers(-1000, 1000, n).astype(np.int32)
    d_x = up(x)
    for mul, add in ((-4, 7), (3, -100), (0, 5)):
        out = ints(n)
        assert lib.amt_affine_i32(ptr(d_x), n, mul, add, ptr(out), None) == L.AMT_OK
        assert np.array_equal(fetch(out, n), fr.affine_i32(x, mul, add)), (mul, add)


# Near-tie policy and the per-window comparison: oracle/compare.py (shared with test_gpu_synth and smoke()).
import os
from oracle.compare import bands_for, compare_windows
DIFFS = {}       # head -> list of |gpu float - oracle float|, all cases of this module
# AMT_TEST_BAND_SCALE widens the bands for a measurement run (the diffs are still recorded): how FLOAT_TOL was set
BAND_SCALE = float(os.environ.get('AMT_TEST_BAND_SCALE', '1'))


@pytest.fixture(scope='module', autouse=True)
def _dump_diffs():
    import json, os
    yield
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    summary = {k: dict(n=len(v), max=float(np.max(v)), p99=float(np.percentile(v, 99)), median=float(np.median(v)))
               for k, v in DIFFS.items() if len(v)}
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'loop_float_diffs.json'), 'w') as f:
            json.dump(summary, f, indent=1)
    except OSError:
        pass
    print('loop float diffs (output units):', summary)


def _run_case(env, p, heads, iters, B, seed, groups=(0,), subtract=True, tweak=None, max_onset=0.4, guess='bank',
              notes=(1, 3), wave_host=None, oracle_refs=None):
    """Product loop vs oracle loop on B windows; EVERY window is compared.  Returns
    (events, n_clean, n_tie, ...): n_clean windows had no decision inside the tie band, n_tie had at least one
    (and were still compared in full, with that decision handed to the oracle when the two sides differ).
    wave_host: the windows (numpy [B, L]) instead of the seeded GPU rendering; oracle_refs: dict name -> [B] of the
    ORACLE's own song-level normalisers -- the oracle then runs on them, not on the product's, and the product's are
    compared with them for every window."""
    torch, synth = env['torch'], env['synth']
    lp = env['loop'].TranscriptionLoop(p, heads=heads, iters=iters, groups=groups, subtract=subtract, guess=guess)
    if tweak:
        tweak(lp)
    lp.setup_device()
    L = p.H * (p.timing_frames - 1)
    if wave_host is not None:
        assert wave_host.shape == (B, L)
        wave = torch.from_numpy(wave_host).cuda()
    else:
        wave, _ = synth.make_windows(B, L, seed=seed, notes_per_window=notes, groups=groups,
                                     max_onset=max_onset * p.window_size_note_time, device='cuda')
    lp.trace = []
    events, b = lp.run(wave, window0=100)
    trace, lp.trace = [{k: v.cpu().numpy() for k, v in t.items()} for t in lp.trace], None
    ev = events.cpu().numpy()
    assert ev.shape == (iters, B, 7) and len(trace) == iters
    from oracle import synth as osynth
    bank = osynth.guess_bank_waves(groups, p.pitch_low, p.pitch_high, sr=p.sr) if subtract else None
    remap = np.zeros(3, np.int32)
    for i, g in enumerate(groups):
        remap[g] = i
    orc = env['oloop'].LoopOracle(p, heads, {k: n.weights for k, n in lp.nets.items()}, iters=iters,
                                  subtract=subtract,
                                  prog_group=remap[synth.prog_group_table(p.instrument_classes)],
                                  bank_waves=bank)
    bands = bands_for(p, BAND_SCALE)
    wave_h = wave.cpu().numpy()
    refs_h = {k: v.cpu().numpy() for k, v in lp.refs.items()}
    if oracle_refs is not None:
        for k, v in refs_h.items():
            rel = np.abs(v - oracle_refs[k]) / oracle_refs[k]
            assert rel.max() < 1e-4, ('normaliser', k, rel)
        refs_h = {k: oracle_refs[k] for k in refs_h}
    clean, ties, forced = compare_windows(orc, wave_h, refs_h, ev, trace,
                                          b.mag.cpu().numpy(), b.ref_max.cpu().numpy(), bands, window0=100,
                                          diffs=DIFFS)
    print('loop parity %s iters %d: %d windows compared in full (events bit-exact, floats within the band, residual '
          '1e-4): %d with no decision near a tie, %d with one inside the band (%d decisions handed over)' %
          ('+'.join(heads), iters, B, clean, ties, forced))
    return ev, clean, ties, lp, orc, wave_h


def _distinct(ev, col):
    return len(np.unique(ev[0, :, col]))


def test_loop_32_windows_distinct_decisions(env):
    """The main parity case: 32 windows through timing + pitch + velocity heads and two subtraction
    iterations.  The calibrated synthetic heads are input-sensitive, so the windows get DIFFERENT onsets,
    ends, pitches and velocities, and bit-exact agreement of the integer events with the CPU oracle is a
    statement about 32 different functions values per head, not about a constant."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import fixture_waves as fw
    # The oracle runs on ITS OWN song-level normalisers for every one of the 32 windows (round 3 handed it the
    # product's): LoopOracle.ref_levels needs ~4 s per window on the 1392-bin grid, so they were computed in the build
    # container (tests/golden/gen_fullsize_fixtures.py, case main32) on the 24-bit audio fixture_waves re-renders here.
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fullsize_fixtures.npz'))
    c = fw.CASES['main32']
    p = fw.params_for('main32')                                            # 86 frames: oracle-sized
    pcm = fw.render_pcm('main32', fw.note_lists('main32', 32))
    assert fw.sha1(pcm) == str(fx['main32_sha1'])
    orefs = {k: fx['main32_refs'][:, j] for j, k in enumerate(('ref_mag', 'ref_C_1', 'ref_C_inst', 'ref_C_foc'))}
    ev, checked, skipped, lp, orc, wave_h = _run_case(env, p, c['heads'], c['iters'], 32, seed=c['seed'],
                                                      wave_host=fw.pcm_to_wave(pcm), oracle_refs=orefs)
    # all 32 windows are compared (_run_case); with bands of ~1e-3 of an output unit and 8 rounded decisions per
    # window at most a window or two are expected to have a decision inside a band at all
    assert checked >= 29, (checked, skipped)
    assert _distinct(ev, 5) >= 10 and _distinct(ev, 6) >= 10      # onset / end frames
    assert _distinct(ev, 2) >= 10 and _distinct(ev, 4) >= 8       # pitch / velocity
    # the stored normalisers are the oracle's definition: recomputed live for one window
    r0 = orc.ref_levels(wave_h[0])
    for k, v in r0.items():
        assert abs(float(orefs[k][0]) - v) / v < 1e-6, k


def _shift_end(delta):
    def tweak(lp):
        # timing_end = timing_start's network with the last Dense's bias moved: end - onset becomes a few frames
        # (tile rule of _resize, 3 <= t < 8) or negative (empty slice -> zero columns)
        w = {k: v.copy() for k, v in lp.nets['timing_start'].weights.items()}
        w['dense2/bias'] = w['dense2/bias'] + np.float32(delta)
        lp.nets['timing_end'].set_weights(w)
    return tweak


@pytest.mark.parametrize('heads,iters,B,nfft,wsec,groups,tweak,what', [
    (('pitch', 'instrument'), 2, 6, 2048, 1, (0, 1, 2), None, 'no timing heads: frames 0..8, instrument argmax'),
    (('timing', 'pitch', 'instrument', 'velocity'), 3, 6, 2048, 1, (0, 1, 2), None, 'all heads, 3 iterations'),
    (('timing', 'pitch', 'velocity'), 1, 8, 2048, 1, (0,), _shift_end(0.3), 'end - onset of a few frames: tile rule'),
    (('timing', 'pitch'), 1, 6, 2048, 1, (0,), _shift_end(-0.5), 'end < onset: empty slice -> zero columns'),
    (('timing', 'pitch', 'velocity'), 2, 6, 4096, 2, (0,), None, 'reference default N = 4096 (F = 2049)'),
    (('timing', 'pitch', 'instrument', 'velocity'), 5, 4, 2048, 1, (0, 1, 2), None, 'C5 shape: all heads, 5 iterations'),
])
def test_loop_vs_oracle(env, heads, iters, B, nfft, wsec, groups, tweak, what):
    p = env['hp'].Hyperparams(N=nfft, window_size_note_time=wsec)
    ev, checked, skipped, lp, orc, _ = _run_case(env, p, heads, iters, B, seed=21 + iters, groups=groups, tweak=tweak)
    assert checked + skipped == B and checked >= B - 2, (what, checked, skipped)
    if 'tile rule' in what:
        d = ev[0, :, 6] - ev[0, :, 5]
        assert np.any((d >= 3) & (d < 8)), d
    if 'empty slice' in what:
        assert np.any(ev[0, :, 6] <= ev[0, :, 5])


def test_loop_without_subtraction_c2_shape(env):
    """BASELINE config C2's shape: STFT + pitch head only, no subtraction (subtract=False): events agree
    with the oracle and the magnitudes are left untouched."""
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    ev, checked, skipped, lp, orc, _ = _run_case(env, p, ('pitch',), 1, 12, seed=2, subtract=False)
    assert checked >= 11
    assert _distinct(ev, 2) >= 4
    assert np.all(ev[..., 3] == -1) and np.all(ev[..., 4] == -1)           # no instrument / velocity head


def test_loop_full_size_c3_vs_oracle(env):
    """Four BASELINE-sized windows (516 frames, N = 2048) of config C3 -- timing(start, end) + pitch + velocity,
    one subtraction -- against the oracle loop: events bit-exact, residual within 1e-4."""
    p = env['hp'].Hyperparams(N=2048)
    ev, checked, skipped, lp, orc, _ = _run_case(env, p, ('timing', 'pitch', 'velocity'), 1, 4, seed=3, max_onset=0.5)
    assert checked + skipped == 4


def test_loop_c4_as_stated(env):
    """BASELINE config C4 as stated: mixed-instrument windows (piano / strings / guitar groups 0-2, 2-4 notes),
    instrument + pitch heads, THREE subtractive iterations, N = 2048 at the full 516 frames -- a few windows of one
    rank's 1024-window shard, every one compared with the oracle loop."""
    p = env['hp'].Hyperparams(N=2048)
    ev, checked, skipped, lp, orc, _ = _run_case(env, p, ('instrument', 'pitch'), 3, 6, seed=4, groups=(0, 1, 2),
                                                 notes=(2, 4), max_onset=0.5)
    assert checked + skipped == 6 and checked >= 5
    assert np.all(ev[..., 3] >= 0) and np.all(ev[..., 4] == -1)            # instrument decided, no velocity head


def test_loop_properties_full_size(env):
    """BASELINE-sized windows (516 frames): size-independent properties --
    subtraction never raises the residual, ReLU keeps it non-negative, a second
    run is bit-identical (deterministic kernels), events are well-formed, and the
    events of a batch do not depend on how it is split."""
    torch, synth = env['torch'], env['synth']
    p = env['hp'].Hyperparams(N=2048)
    lp = env['loop'].TranscriptionLoop(p, heads=('timing', 'pitch', 'velocity'), iters=2).setup_device()
    L = p.H * (p.timing_frames - 1)
    wave, _ = synth.make_windows(6, L, seed=33, notes_per_window=(3, 3), device='cuda')
    b0 = lp.prepare(wave)
    refs = lp.refs
    m0 = b0.mag.clone()
    ev, b = lp.run(wave, refs=refs)
    ev2, b2 = lp.run(wave, refs=refs)
    assert torch.equal(ev, ev2) and torch.equal(b.mag, b2.mag)
    assert float(b.mag.min()) >= 0.0
    assert bool((b.mag <= m0).all())
    e = ev.cpu().numpy()
    assert np.all((e[..., 2] >= 21) & (e[..., 2] <= 108))
    assert np.all((e[..., 5] >= 0) & (e[..., 5] < 516) & (e[..., 6] >= 0) & (e[..., 6] <= 516))
    assert np.all((e[..., 4] >= 1) & (e[..., 4] <= 127))
    sub = {k: v[2:5].contiguous() for k, v in refs.items()}
    ev3, _ = lp.run(wave[2:5].contiguous(), window0=2, refs=sub)
    assert np.array_equal(ev3.cpu().numpy(), e[:, 2:5, :])


def test_run_stream_overlapped_copy_equals_run(env):
    """TranscriptionLoop.run_stream (host batches, copy of batch i+1 on a second stream under the compute of
    batch i, two staging buffers) yields bit-identical events to run() on device-resident copies of the same
    batches -- including a ragged last batch and pageable (unpinned) host memory."""
    torch, synth = env['torch'], env['synth']
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    lp = env['loop'].TranscriptionLoop(p, heads=('timing', 'pitch', 'velocity'), iters=2).setup_device()
    L = p.H * (p.timing_frames - 1)
    sizes = (6, 6, 6, 6, 3)
    waves = [synth.make_windows(n, L, seed=40 + i, notes_per_window=(1, 3), device='cuda')[0] for i, n in enumerate(sizes)]
    want, w0 = [], 7
    for w in waves:
        want.append(lp.run(w, window0=w0)[0].cpu().numpy())
        w0 += w.shape[0]
    hosts = [w.cpu().pin_memory() if i % 2 == 0 else w.cpu().numpy() for i, w in enumerate(waves)]
    got = [e.cpu().numpy() for e, _ in lp.run_stream(hosts, window0=7)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert list(lp.run_stream([])) == []


def test_timing_heads_on_two_streams(env):
    """AMT_TIMING_STREAMS=2 / TranscriptionLoop.timing_streams = 2: timing_end on a second stream, joined before the
    rounding.  Same events, bit for bit."""
    torch, synth = env['torch'], env['synth']
    p = env['hp'].Hyperparams(N=2048, window_size_note_time=1)
    lp = env['loop'].TranscriptionLoop(p, heads=('timing', 'pitch', 'velocity'), iters=2).setup_device()
    L = p.H * (p.timing_frames - 1)
    wave = synth.make_windows(12, L, seed=77, notes_per_window=(1, 3), device='cuda')[0]
    lp.timing_streams = 1
    a = lp.run(wave)[0].cpu().numpy()
    lp.timing_streams = 2
    b = lp.run(wave)[0].cpu().numpy()
    c = lp.run(wave)[0].cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, c)
