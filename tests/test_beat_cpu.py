"""CPU: beat tracking without a GPU.  The reference of tests/beat_reference.py against envelopes written out by hand and
on the click songs (fed by a numpy STFT); the core the kernels compile (csrc/amt_beat_core.h) and the beat layout of
amt_scratch.h giving the reference's bytes in a stand-alone program built with the address and undefined-behaviour
sanitizers; the ABI and amt_saga.beat refusing bad arguments before a GPU is touched; the tempo map of events.write_midi."""
import ctypes
import math
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beat_reference as R                                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the reference by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_on_envelopes_written_out_by_hand():
    # an impulse train, 20 frames apart at 40 frames a second (120 bpm, the prior's centre): its period, every impulse
    lag_lo, lag_hi = 5, 40
    prior, pen = R.lag_tables(lag_lo, lag_hi, 40.0)
    assert int(np.argmax(prior)) == 20 - lag_lo and prior[20 - lag_lo] == 32767 and pen[20 - lag_lo][20] == 0
    assert pen[20 - lag_lo][40] == pen[20 - lag_lo][10] == round(100 * 1024 * np.log(2.0) ** 2) == 49198
    e = R.impulses(200, 20, first=7)
    r = R.track(e, lag_lo, lag_hi, prior, pen)
    assert r['period'] == 20 and r['beats'] == list(range(7, 200, 20))
    # ls = (1000, 2000, 1000) around an impulse; on the impulses C grows by 2000 a beat, the penalty of tau = P being 0
    assert [r['C'][b] for b in r['beats']] == [2000 * (k + 1) for k in range(10)]
    assert [r['back'][b] for b in r['beats']] == [-1] + r['beats'][:-1]
    assert r['C'][6] == 1000 and r['back'][6] == -1 and r['C'][0] == 0
    # the autocorrelation divides by the pairs there are: 9 pairs of 10^6 over 180 places
    a = R.autocorrelation(e, lag_hi)
    assert a[20] == 9 * 10 ** 6 // 180 and a[40] == 8 * 10 ** 6 // 160 and a[19] == 0 and a[80] == 6 * 10 ** 6 // 120 and a[81] == 0
    # zeros, one spike, one frame, fewer frames than the shortest lag: no beats
    for quiet in (np.zeros(50, int), R.impulses(50, 10 ** 6, first=9), [7], [5, 5, 5, 5], []):
        assert R.track(quiet, lag_lo, lag_hi, prior, pen) == dict(period=0, beats=[], C=[0] * len(quiet), back=[-1] * len(quiet))
    # a constant envelope and tables written out by hand: every tie rule
    prior, pen = np.array([5, 5, 5], np.int32), np.zeros((3, 9), np.int32)
    pen[0][1], pen[0][2] = 30, 20                    # P = 2: H = 1, tau in 1..2
    r = R.track([10, 10, 10], 2, 4, prior, pen)      # ls = 30, 40, 30; a[L] = 100 for L < 3
    assert r['period'] == 2                          # s[2] = 5 (2 a[2] + a[4]) = 1000, s[3] = s[4] = 0
    assert r['C'] == [30, 40, 40]
    # t = 1: C[0] - pen[1] = 0: the 0 wins the tie.  t = 2: C[1] - pen[1] = 10 = C[0] - pen[2]: the smaller tau, frame 1
    assert r['back'] == [-1, -1, 1]
    assert r['beats'] == [1]                         # C[1] = C[2] over the last P frames: the smaller frame starts
    pen[0][1], pen[0][2] = 0, 0
    r = R.track([10] * 9, 2, 4, prior, pen)         # a[L] = 100 for every L < 9: s[2] = s[3] = s[4] = 1500, the smaller lag
    assert r['period'] == 2 and r['C'] == [30] + [30 + 40 * t for t in range(1, 8)] + [340]
    assert r['back'] == [-1] + list(range(8)) and r['beats'] == list(range(9))
    assert R.bound(100, 21) == 100 // 11 + 1 and R.bound(0, 1) == 1


def test_reference_envelope_by_hand():
    f = np.float32
    S = np.array([[0, 4, 1], [4, 4, 0.25], [1, 16, 4], [1, 0, 4]], np.float32)
    c = R.compress(S, f(4))
    assert c.tolist() == [[0, 1024, 512], [1024, 1024, 256], [512, 1024, 1024], [512, 0, 1024]]      # 16 / 4 is held at 1
    flux, e = R.envelope(S, f(4), 1)
    assert flux == [0, 1024, 768, 0]
    # means over [t - 1, t + 1] inside the song: 512, 597, 597, 384; d = 0, 427, 171, 0; q = isqrt((427^2 + 171^2) / 4)
    q = int(np.sqrt((427 ** 2 + 171 ** 2) // 4))
    assert q == 229 and e == [0, 427 * 256 // 229, 171 * 256 // 229, 0]
    assert R.envelope(S, f(4), 0)[1] == [0, 0, 0, 0]                       # w = 0: the mean is the value, d = 0, q = 0
    assert R.envelope(S, f(4), 1000)[1] == R.envelope(S, f(4), 3)[1]        # every window is the song
    assert R.envelope(S, f(0), 1) == ([0] * 4, [0] * 4) and R.envelope(S, f('nan'), 1) == ([0] * 4, [0] * 4)
    assert R.compress(np.array([[-1.0, np.nan, np.inf, 1e-30]], np.float32), f(1)).tolist() == [[0, 0, 1024, 0]]
    big = R.envelope_from_flux([0] * 9999 + [2 ** 21], 0)                  # w = 0 again: all zero
    assert not any(big)
    e = R.envelope_from_flux([0] * 99999 + [2 ** 21], 5)                   # one excess in 10^5 frames: held at 65535
    assert e[-1] == R.E_MAX and not any(e[:-1])


def test_click_songs_on_the_reference():
    """The conditions the GPU test asks of beat.beat_track, on the reference alone with a numpy STFT: 44100 Hz, n_fft
    2048, hop 512.  Periods found 86, 57, 43, 39, 30; counts 18, 26, 35, 39, 51; worst beat error 15.1 ms (two hops are
    23.2 ms).  200 bpm is the octave behaviour of the default prior: the half tempo, period 52, 29 beats, each on a gold
    beat."""
    worst = 0.0
    for bpm, period, count in ((60, 86, 18), (90, 57, 26), (120, 43, 35), (133, 39, 39), (174, 30, 51)):
        y, gold = R.click_song(bpm, seed=bpm)
        r = R.beat_track_mag(R.stft_mag(y), 44100, 512)
        assert r['period'] == period and len(r['beats']) == count == len(gold), (bpm, r['period'], len(r['beats']))
        R.click_conditions(r['times'], r['period'], gold, bpm)
        worst = max(worst, max(np.abs(gold - t).min() for t in r['times']))
    for bpm, kw in ((100, dict(jitter_s=0.01)), (120, dict(slow=0.002)), (75, dict(jitter_s=0.01, slow=0.002))):
        y, gold = R.click_song(bpm, seed=bpm, **kw)
        r = R.beat_track_mag(R.stft_mag(y), 44100, 512)
        assert len(r['beats']) == len(gold), (bpm, len(r['beats']), len(gold))
        two_hops = 2 * 512 / 44100
        assert all(np.abs(gold - t).min() <= two_hops for t in r['times']), bpm
        assert all(np.abs(np.asarray(r['times']) - g).min() <= two_hops for g in gold), bpm
    y, gold = R.click_song(200, seed=200)
    r = R.beat_track_mag(R.stft_mag(y), 44100, 512)
    assert r['period'] == 52 and len(r['beats']) == 29 and len(gold) == 58
    R.click_conditions(r['times'], r['period'], gold, 200, count=29, half=True)
    print('click songs: worst beat error %.1f ms' % (1e3 * worst))
    assert worst <= 2 * 512 / 44100


# ---------------------------------------------------------------------------------------------------------------------
# the core in a sanitised program
# ---------------------------------------------------------------------------------------------------------------------
def env_group(S, ldf, ref, w):
    pad = np.full((S.shape[0], ldf), 5.0, np.float32)                  # junk in the pad columns
    pad[:, :S.shape[1]] = S
    return struct.pack('<5i', 0, S.shape[0], S.shape[1], ldf, w) + np.float32(ref).tobytes() + pad.astype('<f4').tobytes()


def track_group(lag_lo, lag_hi, prior, pen, envs):
    blob = [struct.pack('<4i', 1, lag_lo, lag_hi, len(envs)), prior.astype('<i4').tobytes(), np.ascontiguousarray(pen).astype('<i4').tobytes()]
    for e in envs:
        blob += [struct.pack('<i', len(e)), np.asarray(e).astype('<u2').tobytes()]
    return b''.join(blob)


def run_groups(exe, path, groups):
    with open(path, 'wb') as f:
        f.write(b'BEAT' + struct.pack('<i', len(groups)) + b''.join(groups))
    return subprocess.run([exe, path], capture_output=True)


def test_core_in_a_sanitised_stand_alone_program(tmp_path):
    """amt_beat_core.h and amt_beat_make_layout, host only, under the address and undefined-behaviour sanitizers, over
    the whole corpus of the GPU tests -- every F x T with every w, every track envelope under the three lag ranges: the
    reference's flux, envelope, period, count, beats, C and back byte for byte, from arrays of exactly the live sizes
    and a scratch of exactly the bytes the layout counts -- and no sanitizer report."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'beat_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-Xarch_host',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'beat_host_main.cpp'), '-o', exe], check=True)
    path = str(tmp_path / 'cases.bin')
    corpus = R.env_corpus()
    assert {c[1].shape[1] for c in corpus} >= set(R.ENV_F) and {c[1].shape[0] for c in corpus} >= set(R.ENV_T)
    cases = [(name, S, ref, ldf, w) for name, S, ref, ldf in corpus for w in R.ENV_W]
    r = run_groups(exe, path, [env_group(S, ldf, ref, w) for _, S, ref, ldf, w in cases])
    assert r.returncode == 0, r.stderr[-3000:]
    assert b'runtime error' not in r.stderr
    at = 0
    for name, S, ref, ldf, w in cases:
        T = S.shape[0]
        flux, e = R.envelope(S, ref, w)
        assert np.frombuffer(r.stdout, '<i4', T, at).tolist() == flux, (name, w, 'flux')
        assert np.frombuffer(r.stdout, '<u2', T, at + 4 * T).tolist() == e, (name, w, 'e')
        at += 6 * T
    assert at == len(r.stdout)
    for name, (lag_lo, lag_hi, fps), kw, envs in R.track_corpus():
        prior, pen = R.lag_tables(lag_lo, lag_hi, fps, **kw)
        r = run_groups(exe, path, [track_group(lag_lo, lag_hi, prior, pen, envs)])
        assert r.returncode == 0, r.stderr[-3000:]
        assert b'runtime error' not in r.stderr
        at, periods = 0, set()
        for i, e in enumerate(envs):
            want, T = R.track(e, lag_lo, lag_hi, prior, pen), len(e)
            period, count = struct.unpack_from('<2i', r.stdout, at)
            assert (period, count) == (want['period'], len(want['beats'])), (name, i)
            assert np.frombuffer(r.stdout, '<i4', count, at + 8).tolist() == want['beats'], (name, i)
            at += 8 + 4 * count
            assert np.frombuffer(r.stdout, '<i8', T, at).tolist() == want['C'], (name, i, 'C')
            assert np.frombuffer(r.stdout, '<i4', T, at + 8 * T).tolist() == want['back'], (name, i, 'back')
            at += 12 * T
            assert count <= R.bound(T, lag_lo)
            periods.add(period)
        assert at == len(r.stdout)
        if 'flat' in name:
            assert periods == set(range(lag_lo, lag_hi + 1)), name              # every lag of the range is a period
    # parameters outside the limits are refused by the core's own checks
    S = corpus[0][1]
    for F, ldf, w in ((0, 4, 1), (2050, 2052, 1), (3, 2, 1), (1, 4, -1)):
        blob = struct.pack('<5i', 0, 1, F, ldf, w) + np.float32(1).tobytes() + np.zeros(ldf, '<f4').tobytes()
        r = run_groups(exe, path, [blob])
        assert r.returncode == 3 and r.stdout == b'' and b'limits' in r.stderr, (F, ldf, w)
    for lo, hi in ((0, 4), (5, 4), (2, 1025)):
        r = run_groups(exe, path, [struct.pack('<4i', 1, lo, hi, 0)])
        assert r.returncode == 3 and r.stdout == b'' and b'limits' in r.stderr, (lo, hi)
    assert S is not None


# ---------------------------------------------------------------------------------------------------------------------
# the ABI and the Python layer, before any device
# ---------------------------------------------------------------------------------------------------------------------
def test_prototypes_in_the_header_and_the_binding():
    from amt_saga import _lib, beat
    header = open(os.path.join(ROOT, 'include', 'amt_saga.h')).read()
    for name, struct_name, cls in (('amt_beat_envelope', 'amt_beat_env_args', beat.EnvArgs),
                                   ('amt_beat_track', 'amt_beat_track_args', beat.TrackArgs)):
        assert name in _lib.PROTOTYPES
        m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int\s+%s\(' % name, header, flags=re.S)
        assert m and 'util_audio.py:594-639' in m.group(1)
        fields = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct_name, struct_name), header, flags=re.S).group(1)
        fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
        assert re.findall(r'\*?\b([a-z_0-9A-Z]+)\s*[,;]', fields) == [f[0] for f in cls._fields_]
    assert 'amt_beat_scratch_bytes' in _lib.PROTOTYPES
    build = open(os.path.join(ROOT, 'amt-saga_amd', 'build.py')).read()
    assert build.count("'amt_beat.hip'") == 2 and "'amt_beat.hip': NO_PK" in build
    assert 'ffp-contract=fast' not in build.split("'amt_beat.hip'")[1].split('\n')[0]


def test_abi_refuses_bad_arguments_before_any_hip_call():
    from amt_saga import _lib, beat
    lib = _lib.load()
    p = 64                                                             # never dereferenced: checks come first
    big = 1 << 40

    def env(**kw):
        a = dict(mag=p, ref=p, frame_base=p, t_frames=p, env=p, flux=None, scratch=p, scratch_bytes=big, n=2,
                 pool_frames=10, max_frames=5, ldf=8, F=5, w=3)
        a.update(kw)
        return lib.amt_beat_envelope(ctypes.byref(beat.env_args(**a)), None)

    def track(**kw):
        a = dict(env=p, frame_base=p, t_frames=p, prior=p, pen=p, beat_base=p, period=p, count=p, beats=p, C=None,
                 back=None, scratch=p, scratch_bytes=big, n=2, pool_frames=10, beats_total=12, max_frames=5, lag_lo=2,
                 lag_hi=4)
        a.update(kw)
        return lib.amt_beat_track(ctypes.byref(beat.track_args(**a)), None)
    assert lib.amt_beat_envelope(None, None) == lib.amt_beat_track(None, None) == _lib.AMT_E_INVALID
    for k in ('mag', 'ref', 'frame_base', 't_frames', 'env', 'scratch'):
        assert env(**{k: None}) == _lib.AMT_E_INVALID, k
    for k in ('env', 'frame_base', 't_frames', 'prior', 'pen', 'beat_base', 'period', 'count', 'beats', 'scratch'):
        assert track(**{k: None}) == _lib.AMT_E_INVALID, k
    assert env(scratch=p + 8) == track(scratch=p + 4) == _lib.AMT_E_INVALID
    assert env(F=0) == env(F=2050, ldf=2052) == env(F=9) == env(w=-1) == env(max_frames=1 << 20) == _lib.AMT_E_INVALID
    assert env(n=-1) == env(pool_frames=-1) == env(max_frames=-1) == env(scratch_bytes=-1) == _lib.AMT_E_INVALID
    assert env(n=(1 << 24) + 1) == track(n=(1 << 24) + 1) == _lib.AMT_E_INVALID
    for lo, hi in ((0, 4), (5, 4), (2, 1025), (-1, -1)):
        assert track(lag_lo=lo, lag_hi=hi) == _lib.AMT_E_INVALID, (lo, hi)
    assert track(max_frames=1 << 20) == track(n=-1) == track(pool_frames=-1) == track(beats_total=-1) == _lib.AMT_E_INVALID
    need = lib.amt_beat_scratch_bytes(2, 10, 0, 0)
    assert need > 0 and env(scratch_bytes=need - 1) == _lib.AMT_E_SHAPE
    need = lib.amt_beat_scratch_bytes(2, 10, 4, 12)
    assert need > lib.amt_beat_scratch_bytes(2, 10, 0, 0) and track(scratch_bytes=need - 1) == _lib.AMT_E_SHAPE
    # the layout's own arithmetic: 16-byte regions of int64 [10], int64 [2 * 10], int32 [10], int32 [10], int32 [12]
    assert need == 80 + 160 + 48 + 48 + 48
    assert lib.amt_beat_scratch_bytes(-1, 10, 4, 12) < 0 and lib.amt_beat_scratch_bytes(2, 10, 1025, 12) < 0
    assert lib.amt_beat_scratch_bytes(2, -1, 4, 12) < 0 and lib.amt_beat_scratch_bytes(2, 1 << 62, 4, 12) < 0
    # nothing to do, and nothing is launched: accepted without a device
    assert env(n=0, scratch_bytes=big) == env(max_frames=0) == track(n=0) == _lib.AMT_OK
    assert env(F=2049, ldf=2049, w=2 ** 31 - 1, max_frames=(1 << 20) - 1, n=0, flux=2 * p) == _lib.AMT_OK
    assert track(lag_lo=1, lag_hi=1024, n=0, C=2 * p, back=3 * p) == _lib.AMT_OK


def test_params_and_python_refusals_before_the_gpu():
    import torch
    from amt_saga import beat
    p = beat.params(44100, 512)
    lag_lo, lag_hi, w, prior, pen = p
    assert (lag_lo, lag_hi, w) == (21, 130, 43) and p is beat.params(44100, 512) and abs(p.fps - 44100 / 512) < 1e-12
    want = R.tables(44100, 512)
    assert want[:3] == (21, 130, 43) and np.array_equal(prior, want[3]) and np.array_equal(pen, want[4])
    assert prior.dtype == np.int32 and pen.dtype == np.int32 and pen.shape == (110, 261) and prior.max() <= 32767
    assert int(np.argmax(prior)) == 43 - 21                             # 43 frames: 120.2 bpm
    q = beat.params(22050, 256, bpm=(60, 200), tightness=400, mean_s=0.25, centre=100.0, octaves=0.5)
    want = R.tables(22050, 256, bpm=(60, 200), tightness=400, mean_s=0.25, centre=100.0, octaves=0.5)
    assert tuple(q[:3]) == want[:3] and np.array_equal(q[3], want[3]) and np.array_equal(q[4], want[4])
    r = beat.params_for_lags(2, 4, 10.0)
    assert np.array_equal(r[3], R.lag_tables(2, 4, 10.0)[0]) and np.array_equal(r[4], R.lag_tables(2, 4, 10.0)[1])
    for kw, match in ((dict(bpm=(0, 240)), 'bpm'), (dict(bpm=(240, 40)), 'bpm'), (dict(bpm=120), 'bpm'),
                      (dict(bpm=(40, float('nan'))), 'bpm'), (dict(bpm=(1, 240)), 'slowest tempo'),
                      (dict(tightness=0), 'tightness'), (dict(tightness='x'), 'tightness'), (dict(tightness=1e6), 'tightness'),
                      (dict(mean_s=-1), 'mean_s'), (dict(centre=0), 'centre'), (dict(octaves=-1), 'centre, octaves'),
                      (dict(octaves=float('inf')), 'octaves')):
        with pytest.raises(ValueError, match=match):
            beat.params(44100, 512, **kw)
        with pytest.raises(ValueError, match=match):
            beat.beat_track([], 44100, **kw)
        with pytest.raises(ValueError, match=match):
            beat.track([], **kw)
    for sr, hop in ((0, 512), (44100, 0), (44100, 512.5), ('x', 512)):
        with pytest.raises(ValueError, match='sr must be'):
            beat.params(sr, hop)
    for lo, hi in ((0, 4), (5, 4), (2, 1025), (2.0, 4)):
        with pytest.raises(ValueError, match='lags'):
            beat.params_for_lags(lo, hi, 10.0)
    with pytest.raises(ValueError, match='w must be'):
        beat.params_for_lags(2, 4, 10.0, w=-1)
    with pytest.raises(ValueError, match='w must be'):
        beat.onset_envelopes([], w=-1)
    with pytest.raises(ValueError, match='does not exist'):
        beat.track([], tightnes=3)
    with pytest.raises(ValueError, match='params given together'):
        beat.track([], params=p, tightness=3)
    with pytest.raises(ValueError, match='float32 device tensors'):
        beat.onset_envelopes([torch.zeros(4, 516)])                    # a host tensor
    with pytest.raises(ValueError, match='uint16 device tensors'):
        beat.track([torch.zeros(40, dtype=torch.uint16)])
    with pytest.raises(ValueError, match='float32 device tensors'):
        beat.beat_track([torch.zeros(4096)], 44100)
    with pytest.raises(ValueError, match='n_fft'):
        beat.beat_track([], 44100, n_fft=8192, hop=2048)
    assert beat.onset_envelopes([]) == [] and beat.track([]) == []


# ---------------------------------------------------------------------------------------------------------------------
# the tempo map of the MIDI writer
# ---------------------------------------------------------------------------------------------------------------------
def some_notes(n=60, seed=3, span=30.0):
    rng = np.random.default_rng(seed)
    notes = []
    for i in range(n):
        start = float(rng.random() * span)
        notes.append(dict(pitch=30 + i, program=int(rng.choice([0, 24, 40])), velocity=int(rng.integers(1, 128)),
                          start=start, end=start + float(0.02 + rng.random())))
    notes.sort(key=lambda n: (n['start'], n['pitch'], n['program']))
    return notes


def drifting_beats(first, interval, n, drift=0.003, seed=0):
    rng = np.random.default_rng(seed)
    gaps = interval * (1.0 + drift) ** np.arange(n - 1) + rng.normal(0, 0.004, n - 1)
    return [float(t) for t in first + np.concatenate([[0.0], np.cumsum(gaps)])]


def test_write_midi_without_beats_is_unchanged(tmp_path):
    from amt_saga import events
    notes = some_notes()
    # the fixed-tempo file, restated from the format: what write_midi(notes, path) wrote before it knew beats
    chans = [c for c in range(16) if c != 9]
    tracks = [b'\x00\xff\x51\x03\x07\xa1\x20\x00\xff\x2f\x00']
    for i, prog in enumerate(sorted({n['program'] for n in notes})):
        ch, evs = chans[i], []
        for n in notes:
            if n['program'] == prog:
                on = int(round(n['start'] * 960.0))
                evs.append((on, 1, bytes([0x90 | ch, n['pitch'], n['velocity']])))
                evs.append((max(int(round(n['end'] * 960.0)), on + 1), 0, bytes([0x80 | ch, n['pitch'], 0])))
        evs.sort(key=lambda e: (e[0], e[1]))
        data, last = b'\x00' + bytes([0xC0 | ch, prog]), 0
        for t, _, msg in evs:
            data, last = data + events._vlq(t - last) + msg, t
        tracks.append(data + b'\x00\xff\x2f\x00')
    want = b'MThd' + struct.pack('>IHHH', 6, 1, len(tracks), 480) + b''.join(b'MTrk' + struct.pack('>I', len(t)) + t for t in tracks)
    for i, kw in enumerate((dict(), dict(beats=None), dict(beats=[]), dict(beats=[1.25]), dict(beats=None, quantize=4),
                            dict(beats=[0.5], quantize=4))):
        path = str(tmp_path / ('plain%d.mid' % i))
        events.write_midi(notes, path, **kw)
        assert open(path, 'rb').read() == want, kw
    with pytest.raises(ValueError, match='quantize'):
        events.write_midi(notes, str(tmp_path / 'q.mid'), beats=[1.0, 2.0], quantize=5)
    for bad in ([1.0, 1.0], [2.0, 1.0], [-0.5, 1.0], [0.5, float('nan')], [0.0, 100.0]):
        with pytest.raises(ValueError, match='beat'):
            events.write_midi(notes, str(tmp_path / 'b.mid'), beats=bad)
    assert not os.path.exists(str(tmp_path / 'q.mid')) and not os.path.exists(str(tmp_path / 'b.mid'))


def test_tempo_anchors():
    from amt_saga import events
    a = events.tempo_anchors([2.0, 2.5, 3.0, 3.6])
    assert a == [(0.0, 0), (2.0, 1920), (2.5, 2400), (3.0, 2880), (3.6, 3360)]          # round(2.0 / 0.5) = 4 quarters lead in
    assert events.tempo_anchors([0.2, 0.7, 1.2]) == [(0.0, 0), (0.7, 480), (1.2, 960)]  # 0.2 < 0.25: dropped as a grid point
    assert events.tempo_anchors([0.25, 0.75, 1.25]) == [(0.0, 0), (0.25, 480), (0.75, 960), (1.25, 1440)]   # max(1, round(0.5))
    assert events.tempo_anchors([0.0, 0.5]) == [(0.0, 0), (0.5, 480)]
    assert events.tempo_anchors([0.7, 1.2])[1] == (0.7, 480)                             # round(1.4) = 1
    assert events.tempo_anchors([0.8, 1.3])[1] == (0.8, 960)                             # round(1.6) = 2
    for bad in ([], [1.0], [1.0, 1.0], [3.0, 2.0], [-1.0, 2.0]):
        with pytest.raises(ValueError):
            events.tempo_anchors(bad)


def tempo_track(path):
    """[(tick, us per quarter)] of the file's first track."""
    from amt_saga import events
    data = open(path, 'rb').read()
    assert data[:4] == b'MThd' and data[14:18] == b'MTrk'
    ln = struct.unpack('>I', data[18:22])[0]
    trk, i, t, out = data[22:22 + ln], 0, 0, []
    while i < len(trk):
        d, i = events._read_vlq(trk, i)
        t += d
        assert trk[i] == 0xFF
        typ, n = trk[i + 1], trk[i + 2]
        if typ == 0x51:
            out.append((t, int.from_bytes(trk[i + 3:i + 6], 'big')))
        i += 3 + n
    return out


@pytest.mark.parametrize('first,interval', [(0.7, 0.5), (0.1, 0.5), (2.3, 0.345), (0.0, 1.0), (1.4, 0.93)])
def test_write_midi_tempo_map_round_trip(tmp_path, first, interval):
    """Every beat but a dropped first on a multiple of 480 ticks; one set-tempo event per anchor; read_midi(full=True)
    returns every note time within half a tick of the slowest segment plus half a microsecond per quarter before it."""
    from amt_saga import events
    beats = drifting_beats(first, interval, 40, seed=int(interval * 1000))
    notes = some_notes(span=beats[-1] + 3.0)                           # notes behind the last beat too: the last segment extended
    path = str(tmp_path / 'map.mid')
    events.write_midi(notes, path, beats=beats)
    anchors = events.tempo_anchors(beats)
    assert anchors[0] == (0.0, 0) and all(k % 480 == 0 for _, k in anchors)
    kept = beats[1:] if beats[0] < (beats[1] - beats[0]) / 2 else beats
    assert [s for s, _ in anchors[1:]] == kept and (len(kept) == len(beats)) == (first >= interval / 2)
    assert [k for _, k in anchors[1:]] == [anchors[1][1] + 480 * i for i in range(len(kept))]
    tempos = tempo_track(path)
    assert [t for t, _ in tempos] == [k for _, k in anchors]
    seg = [(s1 - s0) * 1e6 * 480 / (k1 - k0) for (s0, k0), (s1, k1) in zip(anchors, anchors[1:])]
    assert [us for _, us in tempos] == [int(round(u)) for u in seg] + [int(round(seg[-1]))]
    back = events.read_midi(path, full=True)
    assert len(back) == len(notes)
    iota_max = max(seg) * 1e-6                                         # seconds per quarter of the slowest segment
    secs = np.asarray([s for s, _ in anchors])
    want = sorted(notes, key=lambda n: (n['pitch'], n['program'], n['start']))
    got = sorted(back, key=lambda n: (n['pitch'], n['program'], n['start']))
    worst = 0.0
    for w, g in zip(want, got):
        assert (w['pitch'], w['program'], w['velocity']) == (g['pitch'], g['program'], g['velocity'])
        # quarters before the note: its place under the written map, a begun quarter counted whole
        k = min(max(int(np.searchsorted(secs, w['start'], side='right')) - 1, 0), len(anchors) - 2)
        quarters = math.ceil(anchors[k][1] / 480 + (w['start'] - anchors[k][0]) / (seg[k] * 1e-6))
        bound = iota_max / 960 + 0.5e-6 * quarters
        assert abs(g['start'] - w['start']) <= bound, (w['start'], g['start'], bound)
        worst = max(worst, abs(g['start'] - w['start']) / bound)
    print('round trip: worst error %.3f of its bound' % worst)
    # the beats themselves, written as notes, come back on their ticks
    clicks = [dict(pitch=60, program=0, velocity=100, start=b, end=b + 0.05) for b in kept]
    events.write_midi(clicks, path, beats=beats)
    data = events.read_midi(path, full=True)
    assert len(data) == len(kept) and max(abs(n['start'] - b) for n, b in zip(data, kept)) <= 0.5e-6 * (len(kept) + anchors[1][1] / 480 + 1)


@pytest.mark.parametrize('div', [1, 2, 3, 4, 6, 8, 12])
def test_write_midi_quantize_puts_onsets_on_the_grid(tmp_path, div):
    from amt_saga import events
    beats = drifting_beats(0.7, 0.5, 30)
    notes = some_notes(span=beats[-1])
    path, plain = str(tmp_path / 'q.mid'), str(tmp_path / 'p.mid')
    events.write_midi(notes, path, beats=beats, quantize=div)
    events.write_midi(notes, plain, beats=beats)
    assert tempo_track(path) == tempo_track(plain)

    def ticks(p):
        """(pitch, program, on tick, off tick) of every note: the file without its tempo track and with a division of 1,
        where the reader's default tempo makes a tick half a second."""
        data = bytearray(open(p, 'rb').read())
        n = struct.unpack('>I', data[18:22])[0]
        body = b'MThd' + bytes(data[4:10]) + struct.pack('>H', struct.unpack('>H', data[10:12])[0] - 1) + b'\x00\x01' + bytes(data[22 + n:])
        q = p + '.ticks'
        open(q, 'wb').write(body)
        return sorted((n['pitch'], n['program'], int(round(n['start'] * 2)), int(round(n['end'] * 2)))
                      for n in events.read_midi(q))
    got, was = ticks(path), ticks(plain)
    grid = 480 // div
    assert len(got) == len(was) == len(notes)
    assert all(on % grid == 0 and off - on >= 1 for _, _, on, off in got)
    by_key = {}
    for pitch, prog, on, off in was:
        by_key.setdefault((pitch, prog), []).append((on, off))
    moved = 0
    for pitch, prog, on, off in got:
        cands = by_key[(pitch, prog)]
        best = min(cands, key=lambda c: abs(c[0] - on))
        assert abs(best[0] - on) * 2 <= grid and off - on == best[1] - best[0]
        moved += best[0] != on
    assert moved > 0


# ---------------------------------------------------------------------------------------------------------------------
# the entry points, before any file is read
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_beat_options_before_the_gpu(tmp_path):
    from amt_saga import transcribe as tr
    quiet = np.zeros(4096, np.float32)
    for bad, match in ((3, 'beats: True, or a dict'), (dict(tightnes=1), 'beats: True, or a dict'),
                       (dict(bpm=(240, 40)), 'bpm'), (dict(tightness=0), 'tightness'), (dict(bpm=(1, 240)), 'slowest tempo')):
        with pytest.raises(ValueError, match=match):
            tr.transcribe(quiet, beats=bad)
        with pytest.raises(ValueError, match=match):
            next(tr.iter_transcribe_songs([quiet], beats=bad))
    flac = str(tmp_path / 'missing.flac')
    single, songs = [flac, str(tmp_path / 'o.mid')], ['--songs', flac, '--out-dir', str(tmp_path / 'o')]
    for argv in (single, songs):
        with pytest.raises(SystemExit, match='--quantize needs --tempo-map'):
            tr.main(argv + ['--quantize', '4'])
        with pytest.raises(SystemExit):                                # argparse's own refusal of the choice
            tr.main(argv + ['--tempo-map', '--quantize', '5'])
    with pytest.raises(SystemExit, match='--quantize needs --tempo-map'):
        tr.main(single + ['--quantize', '4', '--beats-out', str(tmp_path / 'b.txt')])
    with pytest.raises(SystemExit, match='--quantize needs --tempo-map'):
        tr.main(songs + ['--quantize', '4', '--beats-dir', str(tmp_path / 'b')])
    assert not os.path.exists(str(tmp_path / 'o')) and not os.path.exists(str(tmp_path / 'b'))
    for argv in (single + ['--beats-out', str(tmp_path / 'b.txt')], songs + ['--beats-dir', str(tmp_path / 'b2')]):
        with pytest.raises(FileNotFoundError):                         # accepted: the input file is what fails
            tr.main(argv + ['--tempo-map', '--quantize', '12'])
    assert not os.path.exists(str(tmp_path / 'b.txt'))
    tr.write_beats(str(tmp_path / 'beats.txt'), dict(beats=[0.5, 1.0000004, 2.25]))
    assert open(str(tmp_path / 'beats.txt')).read() == '0.500000\n1.000000\n2.250000\n'
