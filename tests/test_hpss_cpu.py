"""CPU: harmonic/percussive separation without a GPU.  The reference of tests/hpss_reference.py against spectrograms split
by hand and against scipy's median filter; its float32 masks against its float64 ones; the core the kernel compiles
(csrc/amt_hpss_core.h) giving the reference's values in a stand-alone program built with the address and undefined-
behaviour sanitizers; the ABI, amt_saga.audio, amt_saga.transcribe and the command lines refusing bad arguments before a
GPU is touched."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpss_reference as R                                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')


def test_reference_splits_the_spectrograms_written_out_by_hand():
    # 3 x 3, kernel (3, 3): reflect repeats the edge value, so an end's window is (edge, edge, neighbour)
    S = np.array([[1, 5, 2], [4, 0, 8], [3, 9, 2]], np.float32)
    r = R.hpss(S, (3, 3), 1.0, (1.0, 1.0))
    Ht = [[1, 5, 2], [3, 5, 2], [3, 9, 2]]          # columns: med(1,1,4) med(1,4,3) med(4,3,3) | (5,5,0) (5,0,9) (0,9,9) | ...
    Pf = [[1, 2, 2], [4, 4, 8], [3, 3, 2]]          # rows: med(1,1,5) med(1,5,2) med(5,2,2) | (4,4,0) (4,0,8) (0,8,8) | ...
    assert r['Ht'].tolist() == Ht and r['Pf'].tolist() == Pf
    f = np.float32
    want_h = [[f(1) / f(2), f(1) / (f(1) + f(2) / f(5)), f(1) / f(2)],
              [(f(3) / f(4)) / (f(3) / f(4) + f(1)), f(1) / (f(1) + f(4) / f(5)), (f(2) / f(8)) / (f(2) / f(8) + f(1))],
              [f(1) / f(2), f(1) / (f(1) + f(3) / f(9)), f(1) / f(2)]]
    assert r['mask_h'].tolist() == [[float(v) for v in row] for row in want_h]
    assert r['Sh'].tolist() == (S * np.array(want_h, np.float32)).tolist()
    hard = R.hpss(S, (3, 3), INF, (1.0, 1.0))
    assert hard['mask_h'].tolist() == [[1, 1, 1], [0, 1, 0], [1, 1, 1]]            # a tie is harmonic
    assert hard['mask_p'].tolist() == [[0, 0, 0], [1, 0, 1], [0, 0, 0]]
    assert (hard['Sh'] + hard['Sp']).tolist() == S.tolist()
    wide = R.hpss(S, (3, 3), INF, (2.0, 2.0))
    assert wide['mask_h'].tolist() == [[0, 1, 0], [0, 0, 0], [0, 1, 0]]            # Ht >= 2 Pf
    assert wide['mask_p'].tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0]]            # Pf > 2 Ht
    # 1 x 5, kernel (5, 3): one frame reflects onto itself, so Ht = S whatever kt is
    S = np.array([[4, 0, 0, 2, 6]], np.float32)
    r = R.hpss(S, (5, 3), 2.0, (1.0, 1.0))
    assert r['Ht'].tolist() == S.tolist() and r['Pf'].tolist() == [[4, 0, 0, 2, 6]]
    assert r['mask_h'].tolist() == [[0.5, 0.5, 0.5, 0.5, 0.5]]                      # Z = 0 < FLT_MIN -> 0.5; equal -> 0.5
    r = R.hpss(S, (5, 5), 2.0, (1.0, 3.0))
    assert r['Pf'].tolist() == [[0, 2, 2, 2, 2]]     # (0,4,4,0,0) (4,4,0,0,2) (4,0,0,2,6) (0,0,2,6,6) (0,2,6,6,2)
    # mask_h = soft(Ht, Pf): (4,0) -> 1; (0,2) -> 0; (0,2) -> 0; (2,2) -> .5; (6,2) -> 1/(1+1/9)
    assert r['mask_h'].tolist() == [[1.0, 0.0, 0.0, 0.5, float(f(1) / (f(1) + (f(2) / f(6)) * (f(2) / f(6))))]]
    # mask_p = soft(Pf, 3 Ht): (0,12) (2,0) (2,0) (2,6) (2,18)
    assert r['mask_p'].tolist() == [[0.0, 1.0, 1.0, float((f(1) / f(3)) * (f(1) / f(3)) / ((f(1) / f(3)) * (f(1) / f(3)) + f(1))),
                                     float((f(2) / f(18)) * (f(2) / f(18)) / ((f(2) / f(18)) * (f(2) / f(18)) + f(1)))]]
    # silence: Z = 0 < FLT_MIN gives 0.5 only when both margins are 1
    quiet = np.zeros((2, 3), np.float32)
    assert R.hpss(quiet, (3, 3), 2.0, (1.0, 1.0))['mask_p'].tolist() == [[0.5] * 3] * 2
    assert R.hpss(quiet, (3, 3), 2.0, (1.0, 3.0))['mask_h'].tolist() == [[0.0] * 3] * 2
    assert R.reflect(np.arange(-5, 7), 3).tolist() == [1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0]
    assert R.reflect(np.arange(-3, 4), 1).tolist() == [0] * 7


def scipy_extends_by_the_rule(n, k):
    """scipy 1.15's own 'reflect' extension left the periodic rule, from run to run, on an axis of 2 with kernels >= 17, of
    3 with kernels 31 and 63 and of 5 with kernel 63 (once with a NaN that no input held); it agreed in every run
    elsewhere.  The direct comparison is made where the axis is at least a quarter of the kernel, which keeps clear of all
    of those.  Below that the rule is the definition, and scipy still does the median -- on an axis that numpy extended
    beforehand."""
    return 4 * n >= k


def test_reference_medians_equal_scipy_reflect():
    """Every (T, F, k), both axes, ties included: the reference equals scipy.ndimage.median_filter(mode='reflect')
    wherever scipy extends by the rule, and everywhere equals scipy's median of the axis extended by the periodic
    reflection (numpy's 'symmetric' padding)."""
    from scipy import ndimage
    rng = np.random.default_rng(3)
    for T in (1, 3, 5, 14, 31, 40):
        for F in (1, 7, 33, 129):
            for ties in (False, True):
                S = rng.integers(0, 6, (T, F)).astype(np.float32) if ties else rng.random((T, F), dtype=np.float32)
                for k in (3, 5, 17, 31, 63):
                    h = (k - 1) // 2
                    for axis, n in ((0, T), (1, F)):
                        size, pad = ((k, 1), ((h, h), (0, 0))) if axis == 0 else ((1, k), ((0, 0), (h, h)))
                        got = R.median_axis(S, k, axis)
                        if scipy_extends_by_the_rule(n, k):
                            assert np.array_equal(got, ndimage.median_filter(S, size=size, mode='reflect')), (T, F, k, axis)
                        wide = ndimage.median_filter(np.pad(S, pad, mode='symmetric'), size=size, mode='reflect')
                        crop = wide[h:h + T] if axis == 0 else wide[:, h:h + F]
                        assert np.array_equal(got, crop), (T, F, k, axis)


def test_float32_masks_against_float64():
    rng = np.random.default_rng(5)
    bar, worst, comp = 8 * 2.0 ** -24, 0.0, 0.0
    for kind in ('random', 'ties', 'zeros', 'huge'):
        S = R.content(kind, 40, 129, 9)
        Ht, Pf = R.medians(S, 31, 17)
        for power in (1.0, 2.0):
            for margin in R.MARGINS:
                m32, m64 = R.masks(Ht, Pf, power, margin), R.masks64(Ht, Pf, power, margin)
                for a, b in zip(m32, m64):
                    worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
                if margin == (1.0, 1.0):
                    comp = max(comp, float(np.abs(m32[0].astype(np.float64) + m32[1] - 1).max()))
        hard32, hard64 = R.masks(Ht, Pf, INF, (1.0, 1.0)), R.masks64(Ht, Pf, INF, (1.0, 1.0))
        assert np.array_equal(hard32[0], hard64[0]) and np.array_equal(hard32[0] + hard32[1], np.ones_like(Ht))
    print('float32 masks against float64: %.3g (bar %.3g); |mask_h + mask_p - 1| <= %.3g' % (worst, bar, comp))
    assert worst <= bar and comp <= bar
    assert rng is not None


def write_cases(path, cases):
    """cases: [(S [T, F], ldf, kernel, [(power, margin), ...])]."""
    blob = [b'HPSS', struct.pack('<i', len(cases))]
    for S, ldf, kernel, sets in cases:
        blob.append(struct.pack('<6i', S.shape[0], S.shape[1], ldf, kernel[0], kernel[1], len(sets)))
        for power, margin in sets:
            blob.append(struct.pack('<3f', power, margin[0], margin[1]))
        blob.append(R.padded(S, ldf).astype('<f4').tobytes())
    with open(path, 'wb') as f:
        f.write(b''.join(blob))


def test_core_in_a_sanitised_stand_alone_program(tmp_path):
    """amt_hpss_core.h, host only, under the address and undefined-behaviour sanitizers, over the whole corpus of the GPU
    tests -- every size, every kernel, all nine power / margin pairs per case: the reference's medians bit for bit and
    its masked components (the same float32 operations in the same order: equal), from arrays of exactly the live sizes,
    the input's pad columns set to 5 -- and no sanitizer report.  The core's second median (bisection, which the kernel
    does not use) gives the same bytes on the cases of at most 20 000 cells: its 32 passes are too slow under the
    sanitizers for the two large sizes, and it is no part of the product."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'hpss_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-Xarch_host',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'hpss_host_main.cpp'), '-o', exe], check=True)
    combos = [(p, m) for p in R.POWERS for m in R.MARGINS]
    corpus = R.corpus()
    assert {c[1] for c in corpus} == set(R.SIZES) and {c[2] for c in corpus} == set(R.KERNELS)
    cases = [(S, size[2], kernel, combos) for _, size, kernel, _, S in corpus]
    path = str(tmp_path / 'cases.bin')
    write_cases(path, cases)
    r = subprocess.run([exe, path], capture_output=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert b'runtime error' not in r.stderr
    at = 0

    def plane(T, F, ldf):
        nonlocal at
        got = np.frombuffer(r.stdout, '<f4', T * ldf, at).reshape(T, ldf)
        at += 4 * T * ldf
        assert not got[:, F:].any()
        return got[:, :F].view(np.uint32)
    for (name, _, _, _, _), (S, ldf, kernel, sets) in zip(corpus, cases):
        T, F = S.shape
        Ht, Pf = R.medians(S, *kernel)
        assert np.array_equal(plane(T, F, ldf), Ht.view(np.uint32)), (name, 'Ht')
        assert np.array_equal(plane(T, F, ldf), Pf.view(np.uint32)), (name, 'Pf')
        for power, margin in sets:
            want = R.finish(S, Ht, Pf, power, margin)
            assert np.array_equal(plane(T, F, ldf), want['Sh'].view(np.uint32)), (name, 'Sh', power, margin)
            assert np.array_equal(plane(T, F, ldf), want['Sp'].view(np.uint32)), (name, 'Sp', power, margin)
    assert at == len(r.stdout)
    # the core's other median, by bisection on the bit pattern: the same bytes
    small = [c for c in cases if c[0].size <= 20000]
    assert len(small) > 100
    write_cases(path, small)
    first, again = subprocess.run([exe, path], capture_output=True), subprocess.run([exe, path, 'bisect'], capture_output=True)
    assert first.returncode == 0 and again.returncode == 0 and again.stdout == first.stdout and len(first.stdout) > 0
    assert b'runtime error' not in again.stderr
    # parameters outside the limits are refused by the core's own check
    for bad in ((4, 3, 2.0, (1, 1)), (3, 65, 2.0, (1, 1)), (3, 3, 3.0, (1, 1)), (3, 3, 2.0, (0.5, 1)), (3, 3, 2.0, (1, 101))):
        write_cases(path, [(cases[0][0], cases[0][1], bad[:2], [combos[0], (bad[2], bad[3])])])
        r = subprocess.run([exe, path], capture_output=True)
        assert r.returncode == 3 and r.stdout == b'' and b'limits' in r.stderr, bad


def test_prototypes_in_the_header_and_the_binding():
    from amt_saga import _lib, audio
    header = open(os.path.join(ROOT, 'include', 'amt_saga.h')).read()
    assert 'amt_hpss_ragged' in _lib.PROTOTYPES
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int\s+amt_hpss_ragged\(', header, flags=re.S)
    assert m and all(cite in m.group(1) for cite in ('util_audio.py:843', 'util_train_test.py:83', 'util_train_test.py:159'))
    fields = re.search(r'typedef struct amt_hpss_args \{(.*?)\} amt_hpss_args;', header, flags=re.S).group(1)
    fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
    names = [n for n in re.findall(r'\*?\b([a-z_0-9A-Z]+)\s*[,;]', fields)]
    assert names == [f[0] for f in audio.HpssArgs._fields_]
    build = open(os.path.join(ROOT, 'amt-saga_amd', 'build.py')).read()
    assert build.count("'amt_hpss.hip'") == 2 and "'amt_hpss.hip': NO_PK" in build


def test_abi_refuses_bad_arguments_before_any_hip_call():
    from amt_saga import _lib, audio
    lib = _lib.load()
    p = 64                                                             # never dereferenced: checks come first

    def call(**kw):
        a = dict(mag=p, out_h=2 * p, out_p=3 * p, out_r=None, med_t=None, med_f=None, frame_base=p, t_frames=p, n=2,
                 pool_frames=10, max_frames=5, ldf=8, F=5, kt=31, kf=31, power=2.0, margin_h=1.0, margin_p=1.0)
        a.update(kw)
        return lib.amt_hpss_ragged(ctypes.byref(audio.hpss_args(**a)), None)
    assert lib.amt_hpss_ragged(None, None) == _lib.AMT_E_INVALID
    for k in ('mag', 'out_h', 'out_p', 'frame_base', 't_frames'):
        assert call(**{k: None}) == _lib.AMT_E_INVALID, k
    for k in ('out_h', 'out_p', 'out_r', 'med_t', 'med_f'):
        assert call(**{k: p}) == _lib.AMT_E_INVALID, k                 # an output that is the input
    assert call(out_p=2 * p) == call(med_t=5 * p, med_f=5 * p) == _lib.AMT_E_INVALID      # two outputs in one place
    for k in (0, 2, 30, 64, 65, -1):
        assert call(kt=k) == call(kf=k) == _lib.AMT_E_INVALID, k
    for power in (0.0, 1.5, 3.0, -INF, float('nan')):
        assert call(power=power) == _lib.AMT_E_INVALID, power
    for m in (0.999, 100.5, -1.0, INF, float('nan')):
        assert call(margin_h=m) == call(margin_p=m) == _lib.AMT_E_INVALID, m
    assert call(F=9) == call(F=0) == call(ldf=6, F=5) == call(ldf=7, F=5) == _lib.AMT_E_INVALID
    assert call(n=-1) == call(max_frames=-1) == call(pool_frames=-1) == _lib.AMT_E_INVALID
    # nothing to do, and nothing is launched: accepted without a device
    assert call(n=0) == call(max_frames=0) == _lib.AMT_OK
    for power in (1.0, 2.0, INF):
        assert call(n=0, power=power, kt=1, kf=63, margin_h=100.0, med_t=5 * p, med_f=6 * p, out_r=7 * p) == _lib.AMT_OK


def test_python_refuses_bad_arguments_before_the_gpu():
    import torch
    from amt_saga import audio, transcribe as tr
    for kw, match in ((dict(kernel=(30, 31)), 'kernel'), (dict(kernel=(31, 65)), 'kernel'), (dict(kernel=(31,)), 'kernel'),
                      (dict(kernel=31), 'kernel'), (dict(kernel=(3.0, 3)), 'kernel'), (dict(kernel=(True, 3)), 'kernel'),
                      (dict(power=3), 'power'), (dict(power='x'), 'power'), (dict(power=float('nan')), 'power'),
                      (dict(margin=(0.5, 1)), 'margin'), (dict(margin=(1, 101)), 'margin'), (dict(margin=2.0), 'margin'),
                      (dict(margin=(1, float('nan'))), 'margin')):
        with pytest.raises(ValueError, match=match):
            audio.hpss_params(**kw)
        with pytest.raises(ValueError, match=match):
            audio.hpss_spectra([], 1024, **kw)
        with pytest.raises(ValueError, match=match):
            audio.hpss([], **kw)
        with pytest.raises(ValueError, match=match):
            tr.transcribe(np.zeros(4096, np.float32), hpss=kw)
        with pytest.raises(ValueError, match=match):
            next(tr.iter_transcribe_songs([np.zeros(4096, np.float32)], hpss=kw))
    assert audio.hpss_params() == (31, 31, 2.0, 1.0, 1.0)
    assert audio.hpss_params((1, 63), INF, (100, 1)) == (1, 63, INF, 100.0, 1.0)
    for n_fft, hop in ((2048, 256), (512, 128), (8192, 2048), (1000, 250)):
        with pytest.raises(ValueError, match='n_fft'):
            audio.hpss([], n_fft=n_fft, hop=hop)
    with pytest.raises(ValueError, match='float32 device tensors'):
        audio.hpss([torch.zeros(4096)])                               # a host tensor
    with pytest.raises(ValueError, match='float32 device tensors'):
        audio.hpss_spectra([torch.zeros(4, 516)], 1024)
    assert audio.hpss_spectra([], 1024) == []
    with pytest.raises(ValueError, match='needs hpss'):
        tr.transcribe(np.zeros(4096, np.float32), percussive=True)
    with pytest.raises(ValueError, match='needs hpss'):
        next(tr.iter_transcribe_songs([np.zeros(4096, np.float32)], percussive=True))
    with pytest.raises(ValueError, match='hpss: True, or a dict'):
        tr.transcribe(np.zeros(4096, np.float32), hpss=dict(kernal=(3, 3)))
    with pytest.raises(ValueError, match='hpss: True, or a dict'):
        tr.transcribe(np.zeros(4096, np.float32), hpss=31)
    with pytest.raises(ValueError, match='one .* pair of paths'):
        audio.save_hpss([torch.zeros(4096)], ['a.flac'], 16000)


def test_command_lines_refuse_bad_hpss_options_before_any_file_is_read(tmp_path):
    from amt_saga import transcribe as tr
    flac = str(tmp_path / 'missing.flac')
    single, songs = [flac, str(tmp_path / 'o.mid')], ['--songs', flac, '--out-dir', str(tmp_path / 'o')]
    with pytest.raises(SystemExit, match='--percussive / --percussive-dir needs --hpss'):
        tr.main(single + ['--percussive', str(tmp_path / 'p.flac')])
    with pytest.raises(SystemExit, match='--percussive / --percussive-dir needs --hpss'):
        tr.main(songs + ['--percussive-dir', str(tmp_path / 'p')])
    for argv in (single, songs):
        for bad in ('31', '31x', '30x31', '31x65', 'axb', '3x3x3', '3.5x3'):
            with pytest.raises(SystemExit, match='^--hpss-kernel: ') as e:
                tr.main(argv + ['--hpss', '--hpss-kernel', bad])
            assert '--hpss-margin' not in str(e.value)
        for bad in ('1', '1,', '0.5,1', '1,101', 'a,b', '1,1,1'):
            with pytest.raises(SystemExit, match='^--hpss-margin: ') as e:
                tr.main(argv + ['--hpss', '--hpss-margin', bad])
            assert '--hpss-kernel' not in str(e.value)
        with pytest.raises(SystemExit):                                # argparse's own refusal of the choice
            tr.main(argv + ['--hpss', '--hpss-power', '3'])
    assert not os.path.exists(str(tmp_path / 'o')) and not os.path.exists(str(tmp_path / 'p'))
    for argv in (single + ['--percussive', str(tmp_path / 'p.flac')], songs + ['--percussive-dir', str(tmp_path / 'p2')]):
        with pytest.raises(FileNotFoundError):                         # accepted: the input file is what fails
            tr.main(argv + ['--hpss', '--hpss-kernel', '63x1', '--hpss-power', 'inf', '--hpss-margin', '2,3.5'])
    assert not os.path.exists(str(tmp_path / 'p.flac'))
