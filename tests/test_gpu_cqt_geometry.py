"""GPU: the constant-Q kernels of csrc/amt_cqt.hip at every hop, filter length and frame.

The case lists are those of tests/cqt_reference.py (validated on the CPU by test_cqt_reference_cpu.py); the float64
definition is oracle/cqt.py.  Bars: the project's REL = 1e-4 -- for the slices PER BIN ROW, max_j |got[k, j] - ref[k, j]|
<= REL * max_j |ref[k, j]| -- bit equality where the kernel's last statement makes it one (the division by `ref`, the
table row a workgroup reads, the window it reads), and 2^-23 for the float32 phasor table.

The whole-window forms return one number per window; the tests aim the window's maximum at a chosen (bin, frame) with
cqt_reference.matched_burst, so that a wrong value at that frame or bin moves the result by 20 % (the CPU premise).

The worst per-row ratio per hop and form goes to cqt_geometry_errors.json in the run's output directory
(test_gpu_rdcnn.py:dump_records); DESIGN.md section 25 quotes the figures."""
import functools
import time

import numpy as np
import pytest

import cqt_reference as R
from oracle import cqt as ocqt
from test_gpu_rdcnn import REL, dump_records

pytestmark = pytest.mark.gpu

RECORDS = []


@pytest.fixture(scope='module', autouse=True)
def _dump_records():
    yield
    dump_records('cqt_geometry_errors.json', RECORDS)
    for r in RECORDS:
        print('cqt slices hop %-5d %-8s %-9s worst row ratio %.3g of the row maximum (%s), bar %.3g' %
              (r['hop'], r['kernel'], r['form'], r['worst'], r['where'], REL))


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import _lib, audio
    return dict(torch=torch, audio=audio, _lib=_lib, lib=_lib.load())


def dev_table(env, inc, length):
    """(phase_inc, length, coef) on the device for hand-set lengths: amt_cqt_coef called directly."""
    torch, audio = env['torch'], env['audio']
    inc_d = torch.from_numpy(np.ascontiguousarray(inc).view(np.int32)).cuda()
    len_d = torch.from_numpy(np.ascontiguousarray(length, np.int32)).cuda()
    coef = torch.empty((len(length), 192), device='cuda')
    env['_lib'].check(env['lib'].amt_cqt_coef(audio.ptr(inc_d), audio.ptr(len_d), len(length), audio.ptr(coef),
                                              audio.stream_ptr()))
    return inc_d, len_d, coef


def slices(env, wave, src, table, n_bins, hop, complex_out=False, bin0=None, ref=None):
    """audio.cqt_slices on numpy / device inputs; numpy out (complex128 for the complex form)."""
    torch = env['torch']
    dev = lambda a, dt: a if a is None or hasattr(a, 'data_ptr') else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    out = env['audio'].cqt_slices(dev(wave, np.float32), dev(src, np.int32), table, n_bins, hop, bin0=dev(bin0, np.int32),
                                  ref=dev(ref, np.float32), complex_out=complex_out)
    if complex_out:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def row_ratios(got, ref):
    """Per bin row: max_j |got - ref| over max_j |ref|; a row whose reference is all zero must be exactly zero."""
    err, top = np.abs(got - ref).max(axis=-1), np.abs(ref).max(axis=-1)
    assert np.all(err[top == 0] == 0), 'a row the reference has at zero is not zero'
    return np.where(top > 0, err / np.where(top > 0, top, 1.0), 0.0)


def oracle_slices(wave, src, inc, length, hop):
    """complex128 [B, n_bins, frames]; its modulus is the magnitude form."""
    return np.stack([ocqt.cqt_frames(wave[b], src[b], inc, length, hop, complex_out=True) for b in range(len(src))])


class Worst:
    """The worst per-row ratio of a (hop, kernel, form), and every row over the bar."""
    def __init__(self, hop, kernel):
        self.hop, self.kernel, self.w, self.over = hop, kernel, {}, []

    def add(self, form, ratios, where):
        b, k = np.unravel_index(np.argmax(ratios), ratios.shape)
        if ratios[b, k] >= self.w.get(form, (-1.0, ''))[0]:
            self.w[form] = (float(ratios[b, k]), '%s window %d bin %d' % (where, b, k))
        for b, k in zip(*np.nonzero(ratios > REL)):
            self.over.append((form, where, int(b), int(k), float(ratios[b, k])))

    def done(self):
        for form, (v, where) in sorted(self.w.items()):
            RECORDS.append(dict(hop=self.hop, kernel=self.kernel, form=form, worst=v, where=where))
        assert not self.over, self.over[:20]


# ---- slices, block-sum form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hop', R.HOPS)
def test_slices_block_sum_sweep(env, hop):
    """Every hand-set length table x every sweep length x frame sets of 1, 3 and 8 frames, magnitudes and complex form,
    held per bin row."""
    inc = R.grid(R.SWEEP_FMIN, 16)[0]
    worst = Worst(hop, 'block-sum')
    for name in R.LENGTH_CASE_NAMES:
        length = R.length_cases(hop)[name]
        table = dev_table(env, inc[:len(length)], length)
        for L in R.sweep_lengths(hop):
            assert R.blocks_fit_lds(env['lib'], L, hop)
            T = 1 + L // hop
            wave = R.sweep_wave(L, 6, hop + L)
            wd = env['torch'].from_numpy(wave).cuda()
            for frames in (1, 3, 8):
                src = R.frame_sets(T, frames)
                B = len(src)
                ref = oracle_slices(wave, src, inc, length, hop)
                mag = slices(env, wd[:B], src, table, len(length), hop)
                re, im = slices(env, wd[:B], src, table, len(length), hop, complex_out=True)
                where = '%s L %d frames %d' % (name, L, frames)
                assert np.isfinite(mag).all() and np.isfinite(re).all() and np.isfinite(im).all()
                worst.add('magnitude', row_ratios(mag, np.abs(ref)), where)
                worst.add('complex', row_ratios(re + 1j * im, ref), where)
                assert np.all(mag[src[:, None, :].repeat(len(length), 1) < 0] == 0)
    worst.done()


def _block_and_direct(env):
    """(hop, L, table, inc, length) of one block-sum and one direct-form geometry, 16 table rows each."""
    out = []
    for hop, L, lengths in ((512, 512 * 21 + 9, R.length_cases(512)['r32_lo']), (441, 441 * 25 + 3, None)):
        inc, length = R.grid(R.SWEEP_FMIN, 16)
        length = length if lengths is None else lengths
        out.append((hop, L, dev_table(env, inc, length), inc, length))
    return out


def test_slices_ref_is_one_division(env):
    """Per-window `ref`: bit for bit numpy float32 unnormalised / ref[b] -- the last statement of both forms is
    __fdiv_rn -- for the magnitudes and for both complex parts."""
    ref = np.array([3.0, 1e-3, 7e5, 1.0], np.float32)
    for hop, L, table, inc, length in _block_and_direct(env):
        T = 1 + L // hop
        src = np.array([[0, T - 1, -1, 5, 5, T // 2, 1, T - 2]] * 4, np.int32)
        wave = R.sweep_wave(L, 4, 3)
        raw = slices(env, wave, src, table, 16, hop)
        got = slices(env, wave, src, table, 16, hop, ref=ref)
        assert raw.dtype == np.float32 and raw.max() > 0
        assert np.array_equal(got, raw / ref[:, None, None]), hop
        rr, ri = slices(env, wave, src, table, 16, hop, complex_out=True)
        gr, gi = slices(env, wave, src, table, 16, hop, complex_out=True, ref=ref)
        assert np.array_equal(gr, rr / ref[:, None, None]) and np.array_equal(gi, ri / ref[:, None, None]), hop
        assert np.all(got[:, :, 2] == 0) and np.all(gr[:, :, 2] == 0) and np.all(gi[:, :, 2] == 0)


def test_slices_bin0_per_window(env):
    """A 16-row table, n_bins = 6, bin0 = -2, 0, 5, 10, 11, 14: window b's rows are rows bin0[b] .. bin0[b] + 5 of a
    full-table launch of that window alone, bit for bit (a workgroup depends only on its table row and window); rows
    outside the table are exactly zero in both outputs."""
    bin0 = np.array([-2, 0, 5, 10, 11, 14], np.int32)
    for hop, L, table, inc, length in _block_and_direct(env):
        T = 1 + L // hop
        src = np.array([[0, T - 1, T // 2, -1, 3]] * 6, np.int32)
        wave = R.sweep_wave(L, 6, 5)
        mag = slices(env, wave, src, table, 6, hop, bin0=bin0)
        re, im = slices(env, wave, src, table, 6, hop, bin0=bin0, complex_out=True)
        for b in range(6):
            full = slices(env, wave[b:b + 1], src[b:b + 1], table, 16, hop)[0]
            fr, fi = slices(env, wave[b:b + 1], src[b:b + 1], table, 16, hop, complex_out=True)
            assert full.max() > 0
            for i in range(6):
                row = int(bin0[b]) + i
                if 0 <= row < 16:
                    assert np.array_equal(mag[b, i], full[row]), (hop, b, i)
                    assert np.array_equal(re[b, i], fr[0, row]) and np.array_equal(im[b, i], fi[0, row]), (hop, b, i)
                else:
                    assert np.all(mag[b, i] == 0) and np.all(re[b, i] == 0) and np.all(im[b, i] == 0), (hop, b, i)
        assert np.all(mag[0, :2] == 0) and np.all(mag[5, 2:] == 0) and np.all(mag[4, 5] == 0)      # the rows meant


def test_slices_wave_stride_and_batch_independence(env):
    """wave_stride = L + 37 with NaN in the gap: equal to the contiguous call and free of NaN; a window alone equals the
    same window inside the batch, bit for bit."""
    torch = env['torch']
    for hop, L, table, inc, length in _block_and_direct(env):
        T = 1 + L // hop
        src = R.frame_sets(T, 8)
        B = len(src)
        wave = R.sweep_wave(L, B, 7)
        buf = torch.full((B, L + 37), float('nan'), device='cuda')
        buf[:, :L] = torch.from_numpy(wave).cuda()
        view = buf[:, :L]
        assert view.stride(0) == L + 37
        for cx in (False, True):
            tight = slices(env, wave, src, table, 16, hop, complex_out=cx)
            wide = slices(env, view, src, table, 16, hop, complex_out=cx)
            assert np.array_equal(np.asarray(tight), np.asarray(wide)) and np.isfinite(np.asarray(wide)).all(), (hop, cx)
            for b in (0, 2, B - 1):
                alone = slices(env, wave[b:b + 1], src[b:b + 1], table, 16, hop, complex_out=cx)
                assert np.array_equal(np.asarray(alone)[..., 0, :, :], np.asarray(tight)[..., b, :, :]), (hop, cx, b)


# ---- slices, direct form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hop', (441, 64, 4096))
def test_slices_direct_form(env, hop):
    """Hops outside the block-sum kernel's set: per-row parity with the oracle, holes, per-window bin0 and ref."""
    assert not any(hop == h for h in R.HOPS)
    inc, length = R.grid(R.SWEEP_FMIN, 16)
    table = dev_table(env, inc, length)
    worst = Worst(hop, 'direct')
    for L in (hop * 23 + 11, R.SHORT_L):
        T = 1 + L // hop
        wave = R.sweep_wave(L, 6, hop + L)
        for frames in (1, 3, 8):
            src = R.frame_sets(T, frames)
            B = len(src)
            ref = oracle_slices(wave, src, inc, length, hop)
            mag = slices(env, wave[:B], src, table, 16, hop)
            re, im = slices(env, wave[:B], src, table, 16, hop, complex_out=True)
            where = 'L %d frames %d' % (L, frames)
            worst.add('magnitude', row_ratios(mag, np.abs(ref)), where)
            worst.add('complex', row_ratios(re + 1j * im, ref), where)
    # bin0 and ref together, against the oracle's rows
    L = hop * 23 + 11
    T = 1 + L // hop
    bin0 = np.array([-2, 0, 5, 10, 11, 14], np.int32)
    div = np.array([3.0, 1e-3, 7e5, 1.0, 3.0, 1e-3], np.float32)
    src = np.array([[0, T - 1, T // 2, -1, 3]] * 6, np.int32)
    wave = R.sweep_wave(L, 6, 11)
    ref = oracle_slices(wave, src, inc, length, hop)
    mag = slices(env, wave, src, table, 6, hop, bin0=bin0, ref=div)
    re, im = slices(env, wave, src, table, 6, hop, bin0=bin0, ref=div, complex_out=True)
    want = np.zeros((6, 6, 5), np.complex128)
    for b in range(6):
        for i in range(6):
            if 0 <= bin0[b] + i < 16:
                want[b, i] = ref[b, bin0[b] + i] / np.float64(div[b])
    worst.add('magnitude', row_ratios(mag, np.abs(want)), 'bin0 and ref')
    worst.add('complex', row_ratios(re + 1j * im, want), 'bin0 and ref')
    worst.done()


# ---- the LDS boundary ------------------------------------------------------------------------------------------------
def _nomem(env, wd, table, hop, need, give):
    torch, audio = env['torch'], env['audio']
    out = torch.zeros((wd.shape[0],), device='cuda')
    ws = torch.empty((max(give, 8) + 7) // 8, dtype=torch.float64, device='cuda')
    return env['lib'].amt_cqt_window_max(audio.ptr(wd), wd.shape[0], wd.shape[1], wd.shape[1], hop, audio.ptr(table[0]),
                                         audio.ptr(table[1]), audio.ptr(table[2]), int(table[0].shape[0]), audio.ptr(out),
                                         audio.ptr(ws) if give else None, give, audio.stream_ptr())


@pytest.mark.timeout(60)
@pytest.mark.parametrize('hop,n_bins', ((128, 4), (2048, 3)))
def test_dispatch_boundary(env, hop, n_bins):
    """The largest L whose block sums fit the LDS, found by bisection on the host, and L + hop: slices run the block-sum
    and then the direct form, the whole-window maximum the LDS and then the HBM-workspace form; without the workspace,
    or with a byte too little, the latter is refused on the host."""
    torch, audio, lib = env['torch'], env['audio'], env['lib']
    L_fit = R.largest_lds_length(lib, hop)
    assert L_fit == (R.LDS_HOPS_MAX + 1) * hop - 1                    # L // hop <= 1692, as the header says
    fmin = 440.0
    inc, length = R.grid(fmin, n_bins)
    table = audio.cqt_table(R.SR, fmin, n_bins, R.BPO, 'cuda')
    assert np.array_equal(table[1].cpu().numpy(), length)
    worst = Worst(hop, 'boundary')
    for L, fits in ((L_fit, True), (L_fit + hop, False)):
        assert R.blocks_fit_lds(lib, L, hop) == fits
        T = 1 + L // hop
        wave = R.sweep_wave(L, 1, hop)
        wave[0, :3 * hop] *= 2.0                                       # the ends count: louder there
        wave[0, -3 * hop:] *= 2.5
        wd = torch.from_numpy(wave).cuda()
        src = np.array([[0, 1, T // 2, T - 2, T - 1]], np.int32)
        t0 = time.time()
        ref = oracle_slices(wave, src, inc, length, hop)
        want = ocqt.cqt_window_max(wave[0], inc, length, hop)
        print('hop %d L %d: oracle %.1f s' % (hop, L, time.time() - t0))
        mag = slices(env, wd, src, table, n_bins, hop)
        re, im = slices(env, wd, src, table, n_bins, hop, complex_out=True)
        form = 'block-sum' if fits else 'direct'
        worst.add(form + ' magnitude', row_ratios(mag, np.abs(ref)), 'L %d' % L)
        worst.add(form + ' complex', row_ratios(re + 1j * im, ref), 'L %d' % L)
        got = float(audio.cqt_window_max(wd, table, hop, form='valu')[0])
        assert abs(got - want) <= REL * want, (hop, L, got, want)
        need = int(lib.amt_cqt_window_max_workspace(L, hop, n_bins, 1))
        if fits:
            assert need == 0
        else:
            assert need > 0
            assert _nomem(env, wd, table, hop, need, 0) == env['_lib'].AMT_E_NOMEM
            assert _nomem(env, wd, table, hop, need, need - 1) == env['_lib'].AMT_E_NOMEM
    worst.done()


# ---- whole-window maximum by targeting -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_reference(name):
    """(waves float32 [targets, L], float64 oracle maximum per window), computed once per case."""
    case = R.MAX_CASES[R.MAX_CASE_IDS.index(name)]
    inc, length = R.case_grid(case)
    waves = R.case_waves(case)
    want = np.array([ocqt.cqt_window_max(x, inc, length, case['hop']) for x in waves])
    waves.setflags(write=False)
    want.setflags(write=False)
    return waves, want


def _case_table(env, case):
    inc, length = R.case_grid(case)
    table = env['audio'].cqt_table(R.SR, case['fmin'], case['n_bins'], R.BPO, 'cuda')
    assert np.array_equal(table[0].cpu().numpy().view(np.uint32), inc) and np.array_equal(table[1].cpu().numpy(), length)
    return table


def _check_targets(case, got, want, form):
    bad = [(form, case['name'], kt, float(g), float(w)) for kt, g, w in zip(case['targets'], got, want)
           if not abs(g - w) <= REL * w]
    assert not bad, bad


@pytest.mark.parametrize('case', R.MAX_CASES, ids=R.MAX_CASE_IDS)
def test_window_max_valu_targets(env, case):
    """One launch: window b peaks at target b.  O(L)-per-bin block-sum form."""
    waves, want = _case_reference(case['name'])
    wd = env['torch'].tensor(waves).cuda()
    got = env['audio'].cqt_window_max(wd, _case_table(env, case), case['hop'], form='valu').cpu().numpy()
    _check_targets(case, got, want, 'valu')


@pytest.mark.parametrize('case', [c for c in R.MAX_CASES if 'mfma' in c['forms']],
                         ids=[c['name'] for c in R.MAX_CASES if 'mfma' in c['forms']])
def test_window_max_mfma_targets(env, case):
    """The split-fp16 MFMA form on the same windows: within REL of the oracle and of the VALU form, 'auto' takes it, a
    second call is bit-identical."""
    audio = env['audio']
    waves, want = _case_reference(case['name'])
    wd = env['torch'].tensor(waves).cuda()
    table = _case_table(env, case)
    assert R.cqm_geometry(case['L'], case['hop']) is not None
    got = audio.cqt_window_max(wd, table, case['hop'], form='mfma').cpu().numpy()
    _check_targets(case, got, want, 'mfma')
    valu = audio.cqt_window_max(wd, table, case['hop'], form='valu').cpu().numpy()
    assert np.all(np.abs(got - valu) <= REL * valu), (case['name'], got, valu)
    assert np.array_equal(audio.cqt_window_max(wd, table, case['hop'], form='mfma').cpu().numpy(), got)
    assert np.array_equal(audio.cqt_window_max(wd, table, case['hop']).cpu().numpy(), got)


def test_window_max_mfma_refusals(env):
    """545 blocks and hop 128: form='mfma' is refused (AMT_E_UNSUPPORTED), form='auto' gives the VALU result."""
    audio, torch = env['audio'], env['torch']
    for hop, L, name in ((256, R.REFUSED_L, 'q4r2'), (128, 145 * 128, 'hop128_edges')):
        assert R.cqm_geometry(L, hop) is None
        case = R.MAX_CASES[R.MAX_CASE_IDS.index(name)]
        inc, length = R.case_grid(case)
        table = _case_table(env, case)
        T = 1 + L // hop
        waves = np.stack([R.matched_burst(L, k, t, inc, length, hop) for k, t in ((0, 0), (6, T - 1), (3, T // 2))])
        wd = torch.from_numpy(waves).cuda()
        with pytest.raises(ValueError):
            audio.cqt_window_max(wd, table, hop, form='mfma')
        valu = audio.cqt_window_max(wd, table, hop, form='valu').cpu().numpy()
        assert np.array_equal(audio.cqt_window_max(wd, table, hop).cpu().numpy(), valu)
        for b in range(3):
            want = ocqt.cqt_window_max(waves[b], inc, length, hop)
            assert abs(valu[b] - want) <= REL * want, (hop, b, valu[b], want)


@pytest.mark.parametrize('form', ('valu', 'mfma'))
def test_window_max_windows_do_not_see_each_other(env, form):
    """A window 1e6 times louder, one 1e-6 times quieter and a silent one among the targets leave the others
    bit-identical to a launch without them (the MFMA form scales its operands per window); silence gives exactly 0."""
    audio, torch = env['audio'], env['torch']
    case = R.MAX_CASES[R.MAX_CASE_IDS.index(R.SCALED_CASE)]
    waves, want = _case_reference(case['name'])
    table = _case_table(env, case)
    plain = audio.cqt_window_max(torch.tensor(waves).cuda(), table, case['hop'], form=form).cpu().numpy()
    mixed = np.concatenate([waves[3:4] * np.float32(1e6), waves[:5], np.zeros_like(waves[:1]), waves[5:],
                            waves[7:8] * np.float32(1e-6)])
    got = audio.cqt_window_max(torch.from_numpy(mixed).cuda(), table, case['hop'], form=form).cpu().numpy()
    n = len(waves)
    assert np.array_equal(got[1:6], plain[:5]) and np.array_equal(got[7:n + 2], plain[5:])
    assert got[6] == 0.0
    inc, length = R.case_grid(case)
    for i, b in ((0, 3), (n + 2, 7)):
        ref = ocqt.cqt_window_max(mixed[i], inc, length, case['hop'])
        assert abs(got[i] - ref) <= REL * ref and 0.5 < ref / (want[b] * (1e6 if i == 0 else 1e-6)) < 2.0, (form, i)


# ---- tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hop', (128, 2048))
def test_coef_table_is_the_rounded_float64_formula(env, hop):
    """amt_cqt_coef on hand-set lengths: every one of the 192 floats per bin within 2^-23 of the float64 value of its
    formula in cqt_coef_kernel (one float32 rounding of a number of magnitude at most 1, plus slack for the device's
    double sincospi)."""
    inc = R.grid(R.SWEEP_FMIN, 16)[0]
    for name in R.LENGTH_CASE_NAMES:
        length = R.length_cases(hop)[name]
        n = len(length)
        coef = dev_table(env, inc[:n], length)[2].cpu().numpy().reshape(n, 32, 6)
        i = np.arange(32, dtype=np.float64)[None, :]
        ph = inc[:n].astype(np.float64)[:, None] * 2.0 ** -31 * i              # phi i in half-turns: exact in float64
        th = 2.0 / length.astype(np.float64)[:, None] * i
        want = np.empty((n, 32, 6))
        for j, a in enumerate((-ph, th - ph, -th - ph)):
            a = np.fmod(a, 2.0)                                                # exact
            want[:, :, 2 * j], want[:, :, 2 * j + 1] = np.cos(np.pi * a), np.sin(np.pi * a)
        assert np.abs(coef - want).max() <= 2.0 ** -23, (hop, name, np.abs(coef - want).max())


def test_mfma_table_bytes(env):
    lib = env['lib']
    for n_bins in (0, 1, 6, 7, 8, 13, 14, 15, 1392):
        assert lib.amt_cqt_mfma_table_bytes(128, n_bins) == 0
        for hop in (256, 512, 1024, 2048):
            want = -(-n_bins // 7) * (hop // 32) * 2 * 128 * 32 * 2
            assert lib.amt_cqt_mfma_table_bytes(hop, n_bins) == want, (hop, n_bins)
    assert lib.amt_cqt_mfma_table_bytes(4096, 8) == 0 and lib.amt_cqt_mfma_table_bytes(384, 8) == 0
