"""GPU: amt_stft_mag / amt_stft_mag_ragged / amt_istft / amt_window_max over every plan amt_stft_plan_create accepts,
against the float64 restatement of tests/stft_reference.py at the bars stated there (8 u log2(n_fft): per frame and pair
for the STFT, window-sum-weighted for the iSTFT).  Five sizes x five hops (N/8, N/4, N/2, N, one that is no power of
two) x centred / uncentred x with / without phases, forward and inverse; the layouts the C ABI allows beyond the
default one; the register carry of the 2048 / 512 magnitude-only form at several frame pairs per workgroup; the ragged
entry uncentred and off the N/4 hop; the segment boundaries of both iSTFT kernels.

Every geometry's distance from float64 -- the GPU's and that of the float32 CPU restatement under the same measure -- is
printed, and written as stft_error_vs_f64.json into the directory the environment variable AMT_RECORD_DIR names (a copy
is kept as profiles/stft_error_vs_f64.json).  The assertions are the bars; the ratio is a record."""
import json
import os

import numpy as np
import pytest

import stft_reference as sr      # tests/stft_reference.py

pytestmark = pytest.mark.gpu

GEOMS = sr.GEOMETRIES
IDS = ['n%d-h%d-c%d' % g for g in GEOMS]
SENT = -7.0
RECORD = {}


def _note(n_fft, hop, center, kind, e_gpu, e_cpu32):
    r = RECORD.setdefault((n_fft, hop, center, kind), dict(n_fft=n_fft, hop=hop, center=center, kind=kind,
                                                           bar=float(sr.bar(n_fft)), e_gpu=0.0, e_cpu32=0.0))
    r['e_gpu'] = max(r['e_gpu'], float(e_gpu))
    r['e_cpu32'] = max(r['e_cpu32'], float(e_cpu32))


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    rows = [RECORD[k] for k in sorted(RECORD)]
    for r in rows:
        r['ratio'] = r['e_gpu'] / max(r['e_cpu32'], 1e-30)
    out = os.environ.get('AMT_RECORD_DIR')
    if out:
        try:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, 'stft_error_vs_f64.json'), 'w') as f:
                json.dump(rows, f, indent=1)
        except OSError:
            pass
    for r in rows:
        print('e_gpu/e_cpu32  n_fft %4d hop %4d center %d %-12s gpu %.3g  cpu %.3g  ratio %.2f  bar %.3g' %
              (r['n_fft'], r['hop'], r['center'], r['kind'], r['e_gpu'], r['e_cpu32'], r['ratio'], r['bar']))


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import audio, _lib
    return dict(torch=torch, lib=_lib.load(), _lib=_lib, audio=audio)


def _p(t):
    return None if t is None else t.data_ptr()


def _stft(env, n_fft, hop, center, wave, with_phase, strided=False, want_ref=True):
    """amt_stft_mag through the C ABI on sentinel-filled buffers.  strided: wave_stride = L + 13, ldf = ldf_of(N) + 8,
    spec_stride = T * ldf + 8 * ldf.  Returns mag [B, T, ldf], phase [B, T, ldf, 2] or None, ref_max [B] or None (numpy),
    after checking that nothing outside [B][T][ldf] (and [B] of ref_max) was written."""
    torch, lib, audio = env['torch'], env['lib'], env['audio']
    B, L = wave.shape
    plan = audio._plan(n_fft, hop, center)
    T = lib.amt_stft_frames(plan, L)
    assert T == sr.n_frames(L, n_fft, hop, center)
    ldf = audio.ldf_of(n_fft) + (8 if strided else 0)
    ws = L + (13 if strided else 0)
    ss = T * ldf + (8 * ldf if strided else 0)
    w = torch.full((B, ws), float('nan'), device='cuda')
    w[:, :L] = torch.from_numpy(wave).cuda()
    mag = torch.full((B, ss), SENT, device='cuda')
    ph = torch.full((B, ss, 2), SENT, device='cuda') if with_phase else None
    ref = torch.full((B + 1,), SENT, device='cuda') if want_ref else None
    st = lib.amt_stft_mag(plan, _p(w), B, L, ws, _p(mag), _p(ph), _p(ref), T, ldf, ss, None)
    assert st == env['_lib'].AMT_OK, st
    torch.cuda.synchronize()
    m = mag.cpu().numpy()
    assert np.all(m[:, T * ldf:] == SENT)
    m = m[:, :T * ldf].reshape(B, T, ldf)
    p = None
    if with_phase:
        p = ph.cpu().numpy()
        assert np.all(p[:, T * ldf:] == SENT)
        p = p[:, :T * ldf].reshape(B, T, ldf, 2)
    r = None
    if want_ref:
        r = ref.cpu().numpy()
        assert r[B] == SENT
        r = r[:B]
    return m, p, r


def _forward_errors(n_fft, hop, center, y, mag, ph, rmax):
    """One signal: (e_gpu, e_cpu32) under the STFT measure, after the exact checks (pad columns, ref_max, unit phases)
    and the per-bin phase comparison."""
    Fb = n_fft // 2 + 1
    b = sr.bar(n_fft)
    F64 = sr.stft64(y, n_fft, hop, center)
    M64 = np.abs(F64)
    F32 = sr.stft32(y, n_fft, hop, center)
    assert mag.shape[0] == F64.shape[1]
    assert np.all(mag[:, Fb:] == 0)
    gm = mag[:, :Fb].T
    e_gpu, e_cpu = sr.stft_error(gm, M64), sr.stft_error(np.abs(F32), M64)
    pn = sr.pair_norms(F64)
    if rmax is not None:
        assert rmax == mag.max()                                       # bit-equal to the returned magnitudes' maximum
        assert abs(float(rmax) - M64.max()) <= b * pn.max()
    if ph is not None:
        assert np.all(ph[:, Fb:] == 0)
        pc = (ph[:, :Fb, 0].astype(np.float64) + 1j * ph[:, :Fb, 1].astype(np.float64)).T
        # |p| = 1 to the roundings of x^2 + y^2, v_rsq_f32 (1 ulp = 2 u) and the product: 3.25 u, taken as 8 u
        assert np.abs(np.abs(pc) - 1).max() <= 8 * sr.U
        e_gpu = max(e_gpu, sr.stft_error(gm.astype(np.float64) * pc, F64))
        e_cpu = max(e_cpu, sr.stft_error(F32, F64))
        # per bin: |X/|X| - Y/|Y|| <= 2 |X - Y| / |Y|, and |X_k - Y_k| <= ||X_t - Y_t||_2 <= bar x pair norm
        sel = sr.phase_compared(M64)
        with np.errstate(divide='ignore', invalid='ignore'):
            tol = 2 * b * pn[None, :] / M64 + 8 * sr.U
            dp = np.abs(pc - F64 / M64)
        assert np.all(dp[sel] <= tol[sel]), float((dp[sel] / tol[sel]).max())
    return e_gpu, e_cpu


@pytest.mark.parametrize('n_fft,hop,center', GEOMS, ids=IDS)
def test_forward_vs_float64(env, n_fft, hop, center):
    """Magnitudes, unit phases and ref_max of B = 3 signals (tonal, white noise, loud-then-quiet) at the shortest
    accepted length, an odd and an even frame count and a length off the hop grid, with and without phases."""
    b = sr.bar(n_fft)
    worst = []
    for L in sr.lengths_of(n_fft, hop, center):
        wave = sr.signals(L, L, n_fft, hop, center)
        for with_phase in (True, False):
            mag, ph, rmax = _stft(env, n_fft, hop, center, wave, with_phase)
            for i in range(3):
                e_gpu, e_cpu = _forward_errors(n_fft, hop, center, wave[i], mag[i], ph[i] if with_phase else None, rmax[i])
                _note(n_fft, hop, center, 'fwd_phase' if with_phase else 'fwd_mag', e_gpu, e_cpu)
                print('fwd n_fft %d hop %d center %d L %d phase %d %-10s e_gpu %.3g e_cpu32 %.3g bar %.3g' %
                      (n_fft, hop, center, L, with_phase, sr.SIGNALS[i], e_gpu, e_cpu, b))
                worst.append((e_gpu, L, with_phase, sr.SIGNALS[i]))
    assert max(worst)[0] <= b, max(worst)


@pytest.mark.parametrize('n_fft,hop,center', [(256, 100, 0), (2048, 512, 1), (4096, 4096, 0)])
def test_silence(env, n_fft, hop, center):
    L = sr.lengths_of(n_fft, hop, center)[1]
    mag, ph, rmax = _stft(env, n_fft, hop, center, np.zeros((2, L), np.float32), True)
    Fb = n_fft // 2 + 1
    assert np.all(mag == 0) and np.all(rmax == 0)
    assert np.all(ph[:, :, :Fb, 0] == 1) and np.all(ph[:, :, :Fb, 1] == 0)
    mag, _, rmax = _stft(env, n_fft, hop, center, np.zeros((2, L), np.float32), False)
    assert np.all(mag == 0) and np.all(rmax == 0)


@pytest.mark.parametrize('n_fft,hop,center', [(2048, 512, 1), (1024, 441, 0)])
def test_layout_freedoms_change_no_bit(env, n_fft, hop, center):
    """wave_stride = L + 13, spec_stride = T * ldf + 8 * ldf, ldf = ldf_of(N) + 8 on sentinel-filled buffers (the hoisted
    2048-point form and the generic one): the same bits as the default layout, zeros in the pad columns, no sentinel
    outside [B][T][ldf] touched (_stft checks); ref_max = NULL leaves the magnitudes as they are."""
    Fb = n_fft // 2 + 1
    L = sr.lengths_of(n_fft, hop, center)[1] + hop // 3          # an odd frame count: the last pair has one frame
    assert sr.n_frames(L, n_fft, hop, center) % 2 == 1
    wave = sr.signals(L, 9, n_fft, hop, center)
    for with_phase in (True, False):
        m0, p0, r0 = _stft(env, n_fft, hop, center, wave, with_phase)
        m1, p1, r1 = _stft(env, n_fft, hop, center, wave, with_phase, strided=True)
        assert m1.shape[2] == m0.shape[2] + 8
        assert np.array_equal(m0[:, :, :Fb], m1[:, :, :Fb]) and np.all(m1[:, :, Fb:] == 0) and np.array_equal(r0, r1)
        if with_phase:
            assert np.array_equal(p0[:, :, :Fb], p1[:, :, :Fb]) and np.all(p1[:, :, Fb:] == 0)
        for strided in (False, True):
            m2, p2, r2 = _stft(env, n_fft, hop, center, wave, with_phase, strided=strided, want_ref=False)
            assert r2 is None and np.array_equal(m2, m1 if strided else m0)
            if with_phase:
                assert np.array_equal(p2, p1 if strided else p0)


def test_register_carry_vs_float64(env):
    """n_fft = 2048, hop = 512, magnitudes only, T = 516, B = 128: launch_stft gives every workgroup several frame pairs
    (its rule is restated and the value asserted), so interior pairs take ten of their sixteen samples per thread from
    the previous pair's registers.  Windows 0, 63 and 127 (tonal, loud-then-quiet, white noise) against float64 at the
    per-frame bar."""
    torch, audio = env['torch'], env['audio']
    n_fft, hop, T, B = 2048, 512, 516, 128
    L = hop * (T - 1)
    pairs, ppb = (T + 1) // 2, 16
    while ppb > 1 and ((pairs + ppb - 1) // ppb) * B < 16384:
        ppb >>= 1
    assert ppb >= 2
    rows = {0: sr.tonal(L, 21), 63: sr.loud_quiet(L, 22, n_fft, hop, 1), 127: sr.white(L, 23)}
    wave = torch.randn(B, L, device='cuda', generator=torch.Generator('cuda').manual_seed(5))
    for i, y in rows.items():
        wave[i] = torch.from_numpy(y).cuda()
    b = audio.AudioBatch(wave, n_fft, hop).stft(with_phase=False)
    assert b.T == T and b.ph is None
    bar = sr.bar(n_fft)
    worst = []
    for i, y in rows.items():
        mag, rmax = b.mag[i].cpu().numpy(), b.ref_max[i].cpu().numpy()
        e_gpu, e_cpu = _forward_errors(n_fft, hop, 1, y, mag, None, rmax)
        print('carry window %d ppb %d e_gpu %.3g e_cpu32 %.3g bar %.3g' % (i, ppb, e_gpu, e_cpu, bar))
        worst.append((e_gpu, i))
    assert max(worst)[0] <= bar, max(worst)


@pytest.mark.parametrize('n_fft,hop,center', [(256, 100, 0), (256, 128, 1), (1024, 256, 0), (1024, 441, 1),
                                              (2048, 512, 0), (2048, 441, 0), (2048, 1024, 1)])
def test_ragged_entry_uncentred_and_other_hops(env, n_fft, hop, center):
    """amt_stft_mag_ragged bit for bit against amt_stft_mag on each signal alone, uncentred and at hops other than
    N/4: the shortest legal signal, lengths on and off the hop grid, and one signal too short for the plan in the same
    launch, whose region and maximum stay unwritten."""
    torch, lib, _lib, audio = env['torch'], env['lib'], env['_lib'], env['audio']
    ldf = audio.ldf_of(n_fft)
    shortest = n_fft // 2 + 1 if center else n_fft
    lens = [shortest, shortest - 1, shortest + hop, n_fft + 9 * hop + hop // 2, n_fft + 20 * hop, n_fft + 13 * hop - 1,
            shortest + 1]
    n = len(lens)
    t = [sr.n_frames(L, n_fft, hop, center) if L >= shortest else 2 for L in lens]
    rng = np.random.default_rng(n_fft + hop)
    fb, sb, f_at, s_at = np.zeros(n, np.int64), np.zeros(n, np.int64), 2, 3
    for i in rng.permutation(n):
        fb[i], sb[i] = f_at, s_at
        f_at += t[i] + int(rng.integers(0, 3))
        s_at += lens[i] + int(rng.integers(0, 7))
    pool_frames, n_samples = f_at + 2, s_at + 3
    samples = torch.zeros(n_samples, device='cuda')
    waves = [torch.from_numpy(sr.white(L, 100 + i)).cuda() for i, L in enumerate(lens)]
    for i, w in enumerate(waves):
        samples[sb[i]:sb[i] + lens[i]] = w
    d_sb, d_fb = torch.from_numpy(sb).cuda(), torch.from_numpy(fb).cuda()
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    plan = audio._plan(n_fft, hop, center)
    for with_phase in (True, False):
        mag = torch.full((pool_frames, ldf), SENT, device='cuda')
        ph = torch.full((pool_frames, ldf, 2), SENT, device='cuda') if with_phase else None
        ref = torch.full((n,), SENT, device='cuda')
        st = lib.amt_stft_mag_ragged(plan, _p(samples), _p(d_sb), _p(d_len), n, max(lens), n_samples, sum(lens), _p(mag),
                                     _p(ph), _p(ref), _p(d_fb), pool_frames, ldf, None)
        assert st == _lib.AMT_OK
        torch.cuda.synchronize()
        written = torch.zeros(pool_frames, dtype=torch.bool, device='cuda')
        for i, w in enumerate(waves):
            if lens[i] < shortest:
                assert float(ref[i]) == 0.0                         # the launcher's memset; the kernel skipped the signal
                continue
            one = audio.AudioBatch(w[None, :], n_fft, hop, bool(center)).stft(with_phase=with_phase)
            assert one.T == t[i]
            assert torch.equal(mag[fb[i]:fb[i] + t[i]], one.mag[0]), (lens[i], 'mag', with_phase)
            if with_phase:
                assert torch.equal(ph[fb[i]:fb[i] + t[i]], one.ph[0]), (lens[i], 'phase')
            assert torch.equal(ref[i], one.ref_max[0]), (lens[i], 'ref_max')
            written[fb[i]:fb[i] + t[i]] = True
        assert bool((mag[~written] == SENT).all())
        if with_phase:
            assert bool((ph[~written] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# inverse
# ---------------------------------------------------------------------------------------------------------------------
def _istft(env, n_fft, hop, center, specs, mode, strided):
    """amt_istft through the C ABI.  specs: B complex128 [F, T] spectrograms; mode 'magphase' (float32 magnitudes and
    unit phases) or 'complex' (interleaved complex64; spec_stride in floats).  strided: 8 * ldf bins between windows
    (NaN there, as in the pad columns: nothing may read them) and wave_stride = Lout + 5.  Returns the output [B, Lout]
    and per window (float64 spectrum as rounded for the kernel, complex64 input of the float32 restatement)."""
    torch, lib, audio = env['torch'], env['lib'], env['audio']
    B, (Fb, T) = len(specs), specs[0].shape
    ldf = audio.ldf_of(n_fft)
    gap = 8 * ldf if strided else 0
    Lout = sr.out_len(T, n_fft, hop, center)
    ws = Lout + (5 if strided else 0)
    hm = np.full((B, T * ldf + gap), np.nan, np.float32)
    hc = np.full((B, T * ldf + gap, 2), np.nan, np.float32)
    fed = []
    for i, F in enumerate(specs):
        vm, vc = hm[i, :T * ldf].reshape(T, ldf), hc[i, :T * ldf].reshape(T, ldf, 2)
        if mode == 'magphase':
            mag32, ph32, Fin = sr.split_magphase32(F)
            vm[:, :Fb] = mag32.T
            vc[:, :Fb, 0], vc[:, :Fb, 1] = ph32.real.T, ph32.imag.T
            fed.append((Fin, mag32 * ph32))
        else:
            Fc = F.astype(np.complex64)
            vc[:, :Fb, 0], vc[:, :Fb, 1] = Fc.real.T, Fc.imag.T
            fed.append((Fc.astype(np.complex128), Fc))
    out = torch.full((B, max(ws, 1)), SENT, device='cuda')
    dc = torch.from_numpy(hc).cuda()
    plan = audio._plan(n_fft, hop, center)
    if mode == 'magphase':
        dm = torch.from_numpy(hm).cuda()
        st = lib.amt_istft(plan, _p(dm), _p(dc), B, T, ldf, T * ldf + gap, _p(out), ws, None)
    else:
        st = lib.amt_istft(plan, _p(dc), None, B, T, ldf, 2 * (T * ldf + gap), _p(out), ws, None)
    if Lout <= 0:
        assert st == env['_lib'].AMT_E_SHAPE                        # centred, one frame: librosa returns no samples
        return None, fed
    assert st == env['_lib'].AMT_OK, st
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:, Lout:] == SENT)
    return o[:, :Lout], fed


def _inverse_case(env, n_fft, hop, center, T, B, mode, strided, note=True):
    Ls = max(sr.out_len(T, n_fft, hop, center), n_fft)
    specs = [sr.ramped_spectrum(Ls, T + 7 * i, n_fft, hop, center, which=(i + 1) % 3)[:, :T] for i in range(B)]
    got, fed = _istft(env, n_fft, hop, center, specs, mode, strided)
    if got is None:
        return 0.0
    worst = 0.0
    for i in range(B):
        y, wss, _ = sr.istft64(fed[i][0], hop, center)
        e_gpu = sr.istft_error(got[i], y, wss)
        e_cpu = sr.istft_error(sr.istft32(fed[i][1], hop, center)[0], y, wss)
        if note:
            _note(n_fft, hop, center, 'inv_' + mode, e_gpu, e_cpu)
        print('inv n_fft %d hop %d center %d T %d B %d %-8s strided %d window %d e_gpu %.3g e_cpu32 %.3g bar %.3g' %
              (n_fft, hop, center, T, B, mode, strided, i, e_gpu, e_cpu, sr.bar(n_fft)))
        worst = max(worst, e_gpu)
    return worst


@pytest.mark.parametrize('n_fft,hop,center', GEOMS, ids=IDS)
def test_inverse_vs_float64(env, n_fft, hop, center):
    """Spectra that are no consistent STFT, as magnitude + unit phase and as interleaved complex, B = 3 with a
    spec_stride larger than a window and B = 1 at the default layout; T = 1, 2, 3 and the frame counts that put the last
    frame one before, on and one after the first segment boundary of the kernel serving the geometry (GH hops of the
    generic kernel, 4 of the streaming one -- the rule is restated in stft_reference and the kernel choice asserted)."""
    streaming = n_fft % 1024 == 0 and hop * 4 == n_fft
    worst = []
    for T in sr.inverse_frames(n_fft, hop, center):
        gh = sr.stream_gh(n_fft, hop, center, T, 3)
        assert (gh == 4) if streaming else (gh is None and sr.generic_gh(hop) >= 1)
        for mode in ('magphase', 'complex'):
            worst.append((_inverse_case(env, n_fft, hop, center, T, 3, mode, True), T, mode, 3))
            if T in (2, sr.inverse_frames(n_fft, hop, center)[-1]):
                worst.append((_inverse_case(env, n_fft, hop, center, T, 1, mode, False), T, mode, 1))
    assert max(worst)[0] <= sr.bar(n_fft), max(worst)


def test_inverse_complex_batch_through_audiobatch(env):
    """AudioBatch.istft with interleaved complex input (ph None) and B = 3 at the default layout: every window is its
    own spectrogram's inverse (spec_stride counts the floats of the complex array: 2 * T * ldf a window)."""
    torch, audio = env['torch'], env['audio']
    for n_fft, hop, center in ((2048, 512, 1), (512, 100, 0)):
        T, B = 9, 3
        ldf = audio.ldf_of(n_fft)
        Fb = n_fft // 2 + 1
        specs = [sr.ramped_spectrum(sr.out_len(T, n_fft, hop, center) + n_fft, 30 + i, n_fft, hop, center,
                                    which=i)[:, :T].astype(np.complex64) for i in range(B)]
        h = np.zeros((B, T, ldf, 2), np.float32)
        for i, Fc in enumerate(specs):
            h[i, :, :Fb, 0], h[i, :, :Fb, 1] = Fc.real.T, Fc.imag.T
        b = audio.AudioBatch(None, n_fft, hop, bool(center))
        b.mag, b.ph = torch.from_numpy(h).cuda(), None
        got = b.istft().cpu().numpy()
        for i, Fc in enumerate(specs):
            y, wss, _ = sr.istft64(Fc.astype(np.complex128), hop, center)
            e = sr.istft_error(got[i], y, wss)
            print('complex batch n_fft %d window %d e_gpu %.3g bar %.3g' % (n_fft, i, e, sr.bar(n_fft)))
            assert e <= sr.bar(n_fft), (n_fft, i, e)


def test_inverse_streaming_32_hop_segments(env):
    """n_fft = 2048, hop = 512, B = 66: the streaming iSTFT kernel with 32 output hops per workgroup (launch_istft's rule
    restated, the value asserted), last frame one before, on and one after a segment boundary (T - 1 = 991, 992, 993).
    One buffer of 994 frames per window serves all three (spec_stride = 994 * ldf > T * ldf); 66 windows = 22 copies of
    three spectrograms, windows 0, 1, 2 against float64 and window 65 bit-equal to window 2."""
    torch, lib, _lib, audio = env['torch'], env['lib'], env['_lib'], env['audio']
    n_fft, hop, center, B, Tmax = 2048, 512, 1, 66, 994
    ldf, Fb = audio.ldf_of(n_fft), n_fft // 2 + 1
    specs = [sr.ramped_spectrum(hop * (Tmax - 1), 60 + i, n_fft, hop, center, which=i) for i in range(3)]
    hm = np.zeros((3, Tmax, ldf), np.float32)
    hp = np.zeros((3, Tmax, ldf, 2), np.float32)
    fed = []
    for i, F in enumerate(specs):
        mag32, ph32, Fin = sr.split_magphase32(F)
        hm[i, :, :Fb] = mag32.T
        hp[i, :, :Fb, 0], hp[i, :, :Fb, 1] = ph32.real.T, ph32.imag.T
        fed.append((Fin, mag32 * ph32))
    dm = torch.from_numpy(hm).cuda().repeat(B // 3, 1, 1)
    dp = torch.from_numpy(hp).cuda().repeat(B // 3, 1, 1, 1)
    dz = (dm[..., None] * dp).contiguous()                          # interleaved complex of the same spectra
    plan = audio._plan(n_fft, hop, center)
    worst = []
    for T in (992, 993, 994):
        assert sr.stream_gh(n_fft, hop, center, T, B) == 32 and (T - 1) % 32 in (31, 0, 1)
        Lout = hop * (T - 1)
        for mode in ('magphase', 'complex'):
            if mode == 'complex' and T != 993:
                continue
            out = torch.full((B, Lout + 3), SENT, device='cuda')
            if mode == 'magphase':
                st = lib.amt_istft(plan, _p(dm), _p(dp), B, T, ldf, Tmax * ldf, _p(out), Lout + 3, None)
            else:
                st = lib.amt_istft(plan, _p(dz), None, B, T, ldf, 2 * Tmax * ldf, _p(out), Lout + 3, None)
            assert st == _lib.AMT_OK
            torch.cuda.synchronize()
            assert bool((out[:, Lout:] == SENT).all()) and torch.equal(out[65], out[2])
            got = out[:3, :Lout].cpu().numpy()
            for i in range(3):
                Fin = fed[i][0][:, :T]
                F32 = fed[i][1][:, :T]
                if mode == 'complex':
                    F32 = (hm[i, :T, :Fb] * (hp[i, :T, :Fb, 0] + 1j * hp[i, :T, :Fb, 1])).T.astype(np.complex64)
                    Fin = F32.astype(np.complex128)
                y, wss, _ = sr.istft64(Fin, hop, center)
                e_gpu = sr.istft_error(got[i], y, wss)
                e_cpu = sr.istft_error(sr.istft32(F32, hop, center)[0], y, wss)
                _note(n_fft, hop, center, 'inv_' + mode, e_gpu, e_cpu)
                print('inv stream32 T %d %-8s window %d e_gpu %.3g e_cpu32 %.3g bar %.3g' %
                      (T, mode, i, e_gpu, e_cpu, sr.bar(n_fft)))
                worst.append((e_gpu, T, mode, i))
    assert max(worst)[0] <= sr.bar(n_fft), max(worst)


# ---------------------------------------------------------------------------------------------------------------------
# amt_window_max, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_window_max_negative_last_element_and_stride(env):
    torch, lib, _lib = env['torch'], env['lib'], env['_lib']
    rng = np.random.default_rng(8)
    B, T, ldf = 5, 7, 132
    stride = T * ldf + 3 * ldf
    h = np.full((B, stride), 1e30, np.float32)                      # the gap between windows holds a LARGER value
    blk = rng.standard_normal((B, T * ldf)).astype(np.float32)
    blk[0] = -np.abs(blk[0]) - 1.0                                   # all negative (D in dB is)
    blk[1] = -80.0                                                   # all equal and negative
    blk[2, -1] = 99.0                                                # the maximum is the last element
    blk[3, 0] = 98.0                                                 # ... the first
    blk[4] = -np.abs(blk[4]) - 1.0
    blk[4, -1] = -0.5                                                # negative maximum in the last element
    h[:, :T * ldf] = blk
    d = torch.from_numpy(h).cuda()
    out = torch.full((B + 1,), SENT, device='cuda')
    assert lib.amt_window_max(_p(d), B, T, ldf, stride, _p(out), None) == _lib.AMT_OK
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[B] == SENT
    assert np.array_equal(o[:B].view(np.uint32), blk.max(axis=1).view(np.uint32))
    # default stride, one window, a long block (more than one workgroup per window)
    big = -np.abs(rng.standard_normal((2, 70 * 1028)).astype(np.float32)) - 1e-3
    big[1, -1] = -1e-4
    d = torch.from_numpy(big).cuda()
    assert lib.amt_window_max(_p(d), 2, 70, 1028, 70 * 1028, _p(out), None) == _lib.AMT_OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[:2].view(np.uint32), big.max(axis=1).view(np.uint32))


def test_refusals(env):
    """Host-side return codes; nothing is launched."""
    import ctypes as C
    torch, lib, _lib, audio = env['torch'], env['lib'], env['_lib'], env['audio']
    h = C.c_void_p()
    for hop in (0, -1, 257):
        assert lib.amt_stft_plan_create(C.byref(h), 256, hop, 1) == _lib.AMT_E_INVALID
    assert lib.amt_stft_plan_create(C.byref(h), 300, 75, 1) == _lib.AMT_E_INVALID
    n_fft, hop = 512, 128
    ldf = audio.ldf_of(n_fft)
    unc, cen = audio._plan(n_fft, hop, False), audio._plan(n_fft, hop, True)
    assert lib.amt_stft_frames(unc, n_fft - 1) == _lib.AMT_E_SHAPE and lib.amt_stft_frames(unc, n_fft) == 1
    buf = torch.full((8, 4 * (ldf + 4) * 2), SENT, device='cuda')
    w = torch.zeros(8, 1024, device='cuda')
    a = (_p(buf), None, None)
    assert lib.amt_stft_mag(unc, _p(w), 1, n_fft - 1, 1024, *a, 1, ldf, ldf, None) == _lib.AMT_E_SHAPE
    assert lib.amt_stft_mag(cen, _p(w), 1, n_fft // 2, 1024, *a, 3, ldf, 3 * ldf, None) == _lib.AMT_E_SHAPE
    T = 1 + 1024 // hop
    assert lib.amt_stft_mag(cen, _p(w), 1, 1024, 1024, *a, T, ldf + 2, T * (ldf + 2), None) == _lib.AMT_E_SHAPE
    assert lib.amt_stft_mag(cen, _p(w), 1, 1024, 1024, *a, T, ldf - 4, T * ldf, None) == _lib.AMT_E_SHAPE
    assert lib.amt_stft_mag(cen, _p(w), 1, 1024, 1024, *a, T + 1, ldf, (T + 1) * ldf, None) == _lib.AMT_E_SHAPE
    assert lib.amt_stft_mag(cen, _p(w), 2, 1024, 1023, *a, T, ldf, T * ldf, None) == _lib.AMT_E_SHAPE
    assert lib.amt_stft_mag(cen, _p(w), 2, 1024, 1024, *a, T, ldf, T * ldf - 1, None) == _lib.AMT_E_SHAPE
    # iSTFT: 3 frames -> 256 samples centred, 768 uncentred
    assert lib.amt_istft(cen, _p(buf), _p(buf), 1, 3, ldf, 3 * ldf, _p(w), 255, None) == _lib.AMT_E_SHAPE
    assert lib.amt_istft(unc, _p(buf), _p(buf), 1, 3, ldf, 3 * ldf, _p(w), 767, None) == _lib.AMT_E_SHAPE
    assert lib.amt_istft(cen, _p(buf), _p(buf), 1, 1, ldf, ldf, _p(w), 1024, None) == _lib.AMT_E_SHAPE
    assert lib.amt_istft(cen, _p(buf), _p(buf), 2, 3, ldf, 3 * ldf - 1, _p(w), 1024, None) == _lib.AMT_E_SHAPE
    # complex input: the stride counts floats -- one window is 2 * T * ldf, and it is even
    assert lib.amt_istft(cen, _p(buf), None, 2, 3, ldf, 3 * ldf, _p(w), 1024, None) == _lib.AMT_E_SHAPE
    assert lib.amt_istft(cen, _p(buf), None, 2, 3, ldf, 6 * ldf + 1, _p(w), 1024, None) == _lib.AMT_E_SHAPE
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()) and bool((w == 0).all())
