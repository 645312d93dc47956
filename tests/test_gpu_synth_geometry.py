"""GPU: the four kernels of csrc/amt_synth.hip over rates, lengths and note edges.

Every case of tests/synth_reference.py:CASES (validated on the CPU by test_synth_reference_cpu.py) is rendered on the
device and held to the project's bars against the float64 checkers: 2e-5 of the window's float64 peak for the additive
kernel (oracle/synth.py), 5e-5 for SoundFont playback (oracle/sf2.py) -- the values test_gpu_synth.py holds at 44100 Hz.
Beside it: bit-identity of a window over its row, its neighbours, max_notes padding, batch size, an `out=` view of a
wider buffer and a second call; the guess bank at two rates; amt_guess_notes against its numpy restatement, exactly; the
program rule of amt_sf2_synth_windows (outside 0 .. n_prog - 1 = silent).

Per case (kernel, sr, L, notes, e_gpu, e_f32, peak) go to synth_error_vs_f64.json in the run's output directory
(test_gpu_rdcnn.py:dump_records); DESIGN.md section 22 carries the worst ratio per kernel."""
import numpy as np
import pytest

import synth_reference as R
from test_gpu_rdcnn import dump_records

pytestmark = pytest.mark.gpu

RECORDS = []


@pytest.fixture(scope='module', autouse=True)
def _dump_records():
    yield
    dump_records('synth_error_vs_f64.json', RECORDS)
    for k in ('add', 'sf2'):
        rs = [r for r in RECORDS if r['kernel'] == k and r['peak'] > 0 and r['e_f32'] is not None]
        if rs:
            w = max(rs, key=lambda r: r['e_gpu'])
            print('synth %s: %d cases, worst e_gpu %.3g of peak (%s; e_f32 %.3g), bar %.3g' %
                  (k, len(rs), w['e_gpu'], w['case'], w['e_f32'], R.bar_of(k)))


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import synth, sf2, _lib
    return dict(torch=torch, synth=synth, sf2=sf2, _lib=_lib, lib=_lib.load())


def render(env, case, row=None, out=None):
    """The device window(s) of a case; row: a float32 [B, M, 5] array replacing the case's own one-row tensor."""
    torch = env['torch']
    nt = R.case_row(case)[None] if row is None else row
    nt = torch.from_numpy(np.ascontiguousarray(nt)).cuda()
    if case['kernel'] == 'add':
        return env['synth'].render_windows_device(nt, case['L'], case['sr'], out=out, timbres=R.case_table(case))
    return env['sf2'].render_windows_device(nt, case['L'], R.font(), case['sr'], out=out)


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_parity_vs_float64(env, case):
    want = R.f64_of(case)
    got = render(env, case).cpu().numpy()[0]
    assert got.shape == (case['L'],) and np.isfinite(got).all()
    e_gpu, peak = R.rel_err(got, want)
    e_f32, _ = R.rel_err(R.f32_of(case), want)
    RECORDS.append(dict(case=case['name'], kernel=case['kernel'], sr=case['sr'], L=case['L'],
                        notes=len(R.used(case['notes'])), e_gpu=e_gpu, e_f32=e_f32, peak=peak))
    print('%-32s e_gpu %.3g e_f32 %.3g peak %.3g' % (case['name'], e_gpu, e_f32, peak))
    if case['silent']:
        assert peak == 0 and np.all(got == 0)
        return
    assert peak > 0 and e_gpu < R.bar_of(case['kernel']), (case['name'], e_gpu, e_f32)
    if case['zero_from']:
        assert np.all(got[R.tail_end(case):] == 0)
    # the scale law: the window's peak is (vel_max / 128)^4, vel_max - 12 (at least 1) for a single used slot
    ns = R.used(case['notes'])
    vmax = max(n[2] for n in ns)
    vmax = max(1, vmax - 12) if len(ns) == 1 else vmax
    assert abs(np.abs(got).max() - (vmax / 128.0) ** 4) <= 1e-5 * (vmax / 128.0) ** 4


IDENTITY_CASES = ['add_33_notes', 'add_sr48000_L16385', 'add_gm_sr16000', 'sf2_mix_sr22050']


@pytest.mark.parametrize('name', IDENTITY_CASES)
def test_window_is_independent_of_row_neighbours_and_padding(env, name):
    """Alone, as row 0, as the last of 37 rows and with max_notes padded to 33: the same bits; so are a second call and
    an `out=` view of a wider buffer, whose columns from L on keep their sentinel."""
    torch = env['torch']
    case = R.CASES[R.CASE_IDS.index(name)]
    L = case['L']
    alone = render(env, case)
    assert torch.equal(alone, render(env, case))
    M = 33
    mine = R.case_row(case, max_notes=M)
    other = R.CASES[R.CASE_IDS.index('add_16_notes' if case['kernel'] == 'add' else 'sf2_mix_sr48000')]
    rows = np.stack([R.notes_row(other['notes'][:1 + i % 5] + [None] * (i % 3), M) for i in range(37)])
    assert torch.equal(render(env, case, row=mine[None])[0], alone[0])            # padded
    first = rows.copy()
    first[0] = mine
    assert torch.equal(render(env, case, row=first)[0], alone[0])                 # row 0 of 37
    last = rows.copy()
    last[-1] = mine
    got = render(env, case, row=last)
    assert torch.equal(got[-1], alone[0])                                         # row 36 of 37
    assert torch.equal(got[:-1], render(env, case, row=rows)[:-1])                # and its neighbours do not see it
    # out = a [B, L] view of a wider buffer
    buf = torch.full((37, L + 19), -7.0, device='cuda')
    ret = render(env, case, row=last, out=buf[:, :L])
    assert ret.data_ptr() == buf.data_ptr() and torch.equal(buf[:, :L], got)
    assert bool((buf[:, L:] == -7.0).all())
    with pytest.raises(ValueError):
        render(env, case, row=last, out=buf[:36, :L])                             # not [B, L]
    with pytest.raises(ValueError):
        render(env, case, row=last, out=buf[:, 0:2 * L:2] if L < 19 else buf.t()[:37, :L])   # sample stride != 1


@pytest.mark.parametrize('kernel', ['add', 'sf2'])
def test_batch_of_300_equals_small_batches(env, kernel):
    torch = env['torch']
    rng = np.random.default_rng(300)
    progs = (0, 1, 2) if kernel == 'add' else (0, 8, 16, 24, 32, 40, 48, 99)
    rows = np.stack([R.notes_row(R.many_notes(int(rng.integers(1, 5)), 0.05, 1000 + i, groups=progs), 4)
                     for i in range(300)])
    case = dict(kernel=kernel, sr=16000, L=777, timbres=None)
    whole = render(env, case, row=rows)
    assert whole.shape == (300, 777) and bool(torch.isfinite(whole).all()) and float(whole.abs().max()) > 0
    parts = torch.cat([render(env, case, row=rows[i:i + 7]) for i in range(0, 300, 7)])
    assert torch.equal(whole, parts)


@pytest.mark.parametrize('sr', [22050, 48000])
def test_guess_bank_vs_float64(env, sr):
    from oracle import synth as osynth
    groups = (0, 1, 2)
    bank = env['synth'].guess_bank_waves(groups, sr=sr)
    Lg = int(round(2 * sr))
    assert tuple(bank.shape) == (len(groups) * 88, Lg)
    bank = bank.cpu().numpy()
    assert np.isfinite(bank).all()
    pitches = sorted(set(range(21, 109, 7)) | {21, 108})
    worst = 0.0
    for gi, g in enumerate(groups):
        for p in pitches:
            want = osynth.render_window([(g, p, 100, 0.0, 1.0)], Lg, sr).numpy()
            e, peak = R.rel_err(bank[gi * 88 + p - 21], want)
            worst = max(worst, e)
            assert peak > 0 and e < R.ADD_BAR, (sr, g, p, e)
    want = osynth.guess_bank_waves((1,), 60, 61, sr=sr)                       # the checker's own bank, same layout
    assert want.shape == (2, Lg)
    for k in range(2):
        assert R.rel_err(bank[88 + 60 - 21 + k], want[k])[0] < R.ADD_BAR
    RECORDS.append(dict(case='bank_sr%d' % sr, kernel='add', sr=sr, L=Lg, notes=1, e_gpu=worst, e_f32=None, peak=1.0))


@pytest.mark.parametrize('n,n_prog,null,frame_seconds,max_dur', R.GUESS_CASES)
def test_guess_notes_exact(env, n, n_prog, null, frame_seconds, max_dur):
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    program, pitch, velocity, onset, end, group = R.guess_inputs(n, n_prog)
    host = dict(program=program, pitch=pitch, velocity=velocity, onset=onset, end=end, prog_group=group)
    if null:
        host[null] = None
    dev = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in host.items()}
    p = lambda k: None if dev[k] is None else dev[k].data_ptr()
    notes = torch.full((n + 1, 5), -7.0, device='cuda')
    _lib.check(lib.amt_guess_notes(p('program'), p('pitch'), p('velocity'), p('onset'), p('end'), p('prog_group'),
                                   n_prog, n, frame_seconds, max_dur, 100.0, notes.data_ptr(), None))
    torch.cuda.synchronize()
    got = notes.cpu().numpy()
    want = R.guess_notes(host['program'], pitch, host['velocity'], onset, end, host['prog_group'], n_prog,
                         frame_seconds, max_dur, 100.0)
    assert np.array_equal(got[:n], want)
    assert np.all(got[n] == -7.0)                                             # nothing past row n - 1


def test_sf2_program_outside_table_is_silent(env):
    """amt_sf2_synth_windows with the fixture's tables cut to n_prog = 41: a note at program 100 or -1 plays nothing
    (it used to play program 40 / program 0), as a program without a preset does; beside an audible note it changes
    nothing but the note count of the scale law."""
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    from amt_saga.device import to_dev
    z, first = R.font().tables(41)
    samples, zd, fd = to_dev(R.font().samples), to_dev(z), to_dev(first, torch.int32)
    L, sr = 4000, 44100

    def run(notes):
        nt = to_dev(R.notes_row(notes)[None])
        wave = torch.full((1, L), -7.0, device='cuda')
        peak = torch.empty(1, device='cuda')
        _lib.check(lib.amt_sf2_synth_windows(nt.data_ptr(), nt.shape[1], 1, L, float(sr), samples.data_ptr(),
                                             samples.shape[0], zd.data_ptr(), zd.shape[0], fd.data_ptr(), 41,
                                             wave.data_ptr(), L, peak.data_ptr(), None))
        torch.cuda.synchronize()
        return wave.cpu().numpy()[0]
    assert np.abs(run([(40, 60, 100, 0.0, 0.05)])).max() > 0 and np.abs(run([(0, 60, 100, 0.0, 0.05)])).max() > 0
    for prog in (100, -1, 41, 48):                                            # 48 has a preset, beyond this table
        assert np.all(run([(prog, 60, 100, 0.0, 0.05)]) == 0), prog
    from oracle import sf2 as osf2
    notes = [(48, 60, 100, 0.0, 0.05), (0, 64, 90, 0.0, 0.05)]
    want = osf2.render_window(notes, L, R.font().samples, {k: v for k, v in R.font().programs.items() if k < 41}, sr)
    e, peak = R.rel_err(run(notes), want)
    assert peak > 0 and e < R.SF2_BAR
