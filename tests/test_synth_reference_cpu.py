"""CPU gate on the synthesiser case list (tests/synth_reference.py): what makes the list valid before any GPU sees it.

For every case the float32 restatement of the kernel is within HALF the kernel's bar of the float64 checker
(oracle/synth.py, oracle/sf2.py), relative to the window's float64 peak -- so a case that sits on a threshold of the
definition fails here and is moved, instead of failing on a GPU for the wrong reason -- every case that is not declared
silent has a float64 peak > 0, and every declared-silent case is exactly 0.  The list must also be able to fail: each of the
wrong kernels the restatement can be turned into moves at least one case past its full bar."""
import numpy as np
import pytest

import synth_reference as R


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_case_is_valid(case):
    want = R.f64_of(case)
    got = R.f32_of(case)
    assert want.shape == got.shape == (case['L'],) and got.dtype == np.float32
    assert np.isfinite(got).all() and np.isfinite(want).all()
    e, peak = R.rel_err(got, want)
    print('%-32s e_f32 %.3g peak %.3g' % (case['name'], e, peak))
    if case['silent']:
        assert peak == 0.0 and np.all(got == 0)
        return
    assert peak > 0
    assert e <= 0.5 * R.bar_of(case['kernel']), (case['name'], e)
    if case['zero_from']:
        k = R.tail_end(case)
        assert 0 < k < case['L'] - 256                      # the tail ends inside the window, blocks before its end
        assert want[k - 1] != 0 and np.all(want[k:] == 0) and np.all(got[k:] == 0)


def test_case_list_covers_what_it_claims():
    by = {c['name']: c for c in R.CASES}
    add = [c for c in R.CASES if c['kernel'] == 'add']
    for sr in (8000, 11025, 16000, 22050, 48000, 96000):
        assert {c['L'] for c in add if c['sr'] == sr} >= {1, 255, 256, 257, 16384, 16385}
    assert all(c['sr'] != 44100 for c in add)
    assert any(len(R.used(c['notes'])) == 16 for c in add) and any(len(R.used(c['notes'])) == 33 for c in add)
    notes = [n for c in add for n in R.used(c['notes'])]
    assert any(n[3] < 0 for n in notes) and any(n[4] == 0 for n in notes)
    assert {1, 127} <= {n[2] for n in notes}
    # onset on a sample instant: t - onset is exactly 0 at one sample of the window
    c = by['add_onset_on_sample']
    on = np.float32(c['notes'][0][3])
    assert np.any(np.arange(c['L'], dtype=np.float64) / c['sr'] - float(on) == 0.0)
    # Nyquist: harmonic 10 of A4 is exactly sr / 2 at 8800 and just under it at 8801
    assert 10 * 440.0 == 8800 / 2 and 10 * 440.0 < 8801 / 2 < 11 * 440.0
    # the two-note window whose second note is outside: two used slots, one audible
    c = by['add_one_audible_one_outside']
    assert c['notes'][1][3] * c['sr'] > c['L']


@pytest.mark.parametrize('mutate', R.MUTATIONS_ADD + R.MUTATIONS_SF2)
def test_case_list_can_fail(mutate):
    """Each plausible wrong kernel is past the FULL bar on at least one case (the names are in the assertion message
    when none is)."""
    kernel = 'add' if mutate in R.MUTATIONS_ADD else 'sf2'
    # the cases that can show it, to keep this quick: all of them would do
    pick = {'phase_f32': lambda c: '6s' in c['name'], 'nyquist_gt': lambda c: 'nyquist' in c['name'],
            'scale_no_stride': lambda c: c['L'] == 16385, 'count_audible': lambda c: 'one_audible' in c['name'],
            'i1_no_wrap': lambda c: 'loop_end' in c['name'] or 'mix' in c['name'],
            'release_from_t': lambda c: 'release_in' in c['name']}[mutate]
    caught = []
    for c in R.CASES:
        if c['kernel'] != kernel or c['silent'] or not pick(c):
            continue
        e, _ = R.rel_err(R.f32_of(c, mutate=mutate), R.f64_of(c))
        if e > R.bar_of(kernel):
            caught.append((c['name'], e))
    print(mutate, caught)
    assert caught, mutate


def test_guess_notes_restatement():
    """The restatement against the rule spelled out per element in Python scalars."""
    for n, n_prog, null, fs, max_dur in R.GUESS_CASES:
        program, pitch, velocity, onset, end, group = R.guess_inputs(n, n_prog)
        got = R.guess_notes(None if null == 'program' else program, pitch, None if null == 'velocity' else velocity,
                            onset, end, None if null == 'prog_group' else group, n_prog, fs, max_dur, 100.0)
        assert got.dtype == np.float32 and got.shape == (n, 5)
        for i in range(n):
            pr = 0 if null == 'program' else min(max(int(program[i]), 0), n_prog - 1)
            d = np.float32(max(int(end[i]) - int(onset[i]), 0)) * np.float32(fs)
            want = [0.0 if null == 'prog_group' else float(group[pr]), float(pitch[i]),
                    100.0 if null == 'velocity' else float(velocity[i]), 0.0, float(min(d, np.float32(max_dur)))]
            assert got[i].tolist() == want, (n, n_prog, null, i)
        assert (got[:, 4] == 0).any() or n == 1
        assert (got[:, 4] == np.float32(max_dur)).any() or n == 1
    assert R.guess_notes(None, [60], None, [5], [3], None, 4, 0.01, 1.0, 100.0)[0].tolist() == [0, 60, 100, 0, 0]


def test_host_timbre_table_is_checked_before_the_device():
    """A caller's host table with a non-finite entry, H < 1 or attack <= 0 is refused before any device call (the kernel
    and the float64 checker disagree on such rows: one returns 1, the other NaN)."""
    from amt_saga import synth
    good = np.array([[3, 2.0, 0.0, 0.01, 0.0]], np.float32)
    assert synth.check_host_timbres(good).dtype == np.float32
    for col, val in ((1, np.nan), (2, np.inf), (0, 0.0), (0, 0.5), (3, 0.0), (3, -0.01)):
        bad = np.concatenate([good, good])
        bad[1, col] = val
        with pytest.raises(ValueError):
            synth.render_windows_device([[(0, 69, 100, 0.0, 0.5)]], 100, 44100, timbres=bad)
    with pytest.raises(ValueError):
        synth.render_windows_device([[(0, 69, 100, 0.0, 0.5)]], 100, 44100, timbres=np.zeros((2, 4), np.float32))
