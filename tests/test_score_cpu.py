"""CPU: scoring without a GPU.  The reference of tests/score_reference.py against exhaustive search and against answers
worked out by hand; first fit shown to fall short; the core the kernel compiles (csrc/amt_score_core.h) prints the same
counts in a stand-alone program built with the address and undefined-behaviour sanitizers; the host side of
amt_saga.score, the tempo map of events.read_midi(full=True), and the ABI and the command lines refusing bad arguments
before a GPU is touched.  Nothing here has a tolerance: every number is a count."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_reference as R                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def corpus():
    return R.corpus()


@pytest.fixture(scope='module')
def expected(corpus):
    """{name: the reference's ten counts under the identity table}, computed once."""
    return {name: R.score(est, ref) for name, est, ref in corpus}


def as_dicts(notes):
    return [dict(pitch=p, program=g, start=on / 1e6, end=off / 1e6) for p, g, on, off in notes]


def exhaustive(est, ref, offset, program, group=R.IDENTITY):
    """The largest matching over ALL matchings: every reference in turn stays alone or takes any unused estimate it
    matches; the sets of used estimates are enumerated (memoised by set)."""
    adj = [[i for i, e in enumerate(est) if R.matched(e, r, offset, program, group)] for r in ref]
    memo = {}

    def best(j, used):
        if j == len(adj):
            return 0
        if (j, used) not in memo:
            memo[(j, used)] = max([best(j + 1, used)] + [1 + best(j + 1, used | (1 << i)) for i in adj[j] if not used >> i & 1])
        return memo[(j, used)]
    return best(0, 0)


def test_reference_equals_exhaustive_search_on_the_random_pairs(corpus, expected):
    n = 0
    for name, est, ref in corpus:
        if not name.startswith('random'):
            continue
        assert len(est) <= 12 and len(ref) <= 12 and {x[0] for x in est + ref} <= {60, 62}
        assert [exhaustive(est, ref, o, p) for o, p in R.VARIANTS] == expected[name][2:6], name
        n += 1
    assert n == 200


def test_by_hand_answers(corpus, expected):
    by = {name: (est, ref) for name, est, ref in corpus}
    assert expected['augment'] == R.AUGMENT_ROW == [2, 2, 2, 2, 2, 2, 100, 10, 0, 110]
    assert R.first_fit(*by['augment'], offset=True) == 1
    assert expected['tolerance_edges'][:6] == R.TOLERANCE_EDGES_NOTES == [10, 10, 9, 5, 9, 5]
    est, ref = by['tolerance_edges']
    per_pitch = {}
    for e, r in zip(est, ref):
        per_pitch[e[0]] = (R.max_matching([e], [r]), R.max_matching([e], [r], offset=True))
    assert per_pitch == {60: (1, 1), 61: (0, 0), 62: (1, 1), 63: (1, 0), 64: (1, 1), 65: (1, 0), 66: (1, 1), 67: (1, 0),
                         68: (1, 1), 69: (1, 0)}
    assert expected['frame_edges'] == R.FRAME_EDGES_ROW == [5, 4, 2, 2, 2, 2, 3, 2, 105, 101]
    assert R.FRAME_EDGES_ROW[9] % 64
    assert expected['empty_both'] == [0] * 10
    assert expected['empty_est'] == [0, 2, 0, 0, 0, 0, 0, 0, 115, 90]          # 50 + 65 cells, none of them found
    assert expected['empty_ref'] == [2, 0, 0, 0, 0, 0, 0, 115, 0, 90]
    # programs: equal notes that differ in program, under the identity and under a table that merges 40 with 48
    assert expected['program_split'][2:6] == [5, 5, 3, 3]
    assert R.score(*by['program_split'], group=R.MERGED)[2:6] == [5, 5, 4, 4]
    # the dense cluster: every reference has more than 64 candidates
    est, ref = by['dense_cluster']
    assert len(est) == len(ref) == 70 and len({x[0] for x in est + ref}) == 1
    assert max(x[2] for x in est + ref) - min(x[2] for x in est + ref) <= 40000
    # the long chain needs augmenting paths hundreds of references long
    est, ref = by['long_chain']
    paths = []
    assert len(est) == len(ref) == 3000 and R.max_matching(est, ref, offset=True, paths=paths) == 3000
    assert sorted(paths)[-R.CHAIN_SEGMENTS:] == [R.CHAIN_LENGTH] * R.CHAIN_SEGMENTS
    assert R.first_fit(est, ref, offset=True) == 3000 - R.CHAIN_SEGMENTS
    assert max(x[3] for x in by['late'][0]) > 2 ** 32 and expected['late'][2:6] == [2, 2, 2, 2]
    assert {x[0] for x in by['pitch_edges'][0]} == {0, 127}


def test_first_fit_falls_short_of_the_maximum(corpus, expected):
    short = short_on = 0
    for name, est, ref in corpus:
        if name.startswith('random'):
            ff, ff_on = R.first_fit(est, ref, offset=True), R.first_fit(est, ref)
            assert ff <= expected[name][3] and ff_on <= expected[name][2]
            short += ff < expected[name][3]
            short_on += ff_on < expected[name][2]
    print('first fit below the maximum: onset + offset %d of 200, onset %d of 200' % (short, short_on))
    assert short >= 5


def test_summary_on_zero_denominators_and_by_hand():
    from amt_saga import score
    s = score.summary(np.zeros((2, 10), np.int64))
    for entry in s['pairs'] + [s['micro']]:
        for key in ('onset', 'onset_offset', 'onset_program', 'onset_offset_program', 'frame'):
            assert entry[key] == dict(precision=0.0, recall=0.0, f=0.0)
    s = score.summary([[4, 2, 2, 1, 0, 0, 30, 10, 20, 99], [0, 6, 0, 0, 0, 0, 0, 0, 60, 70]])
    assert s['pairs'][0]['onset'] == dict(precision=0.5, recall=1.0, f=2 * 0.5 / 1.5)
    assert s['pairs'][0]['onset_offset'] == dict(precision=0.25, recall=0.5, f=2 * 0.25 * 0.5 / 0.75)
    assert s['pairs'][0]['onset_program'] == dict(precision=0.0, recall=0.0, f=0.0)
    assert s['pairs'][0]['frame'] == dict(precision=0.75, recall=0.6, f=2 * 0.75 * 0.6 / 1.35)
    assert s['pairs'][1]['onset'] == dict(precision=0.0, recall=0.0, f=0.0)           # no estimate at all
    assert s['micro']['onset'] == dict(precision=0.5, recall=0.25, f=2 * 0.5 * 0.25 / 0.75)
    assert s['micro']['frame'] == dict(precision=0.75, recall=30 / 110, f=2 * 0.75 * (30 / 110) / (0.75 + 30 / 110))
    assert s['micro']['counts']['n_ref'] == 8 and s['pairs'][0]['counts']['n_frames'] == 99


def test_pack_sorts_rounds_and_refuses_bad_notes(corpus):
    from amt_saga import score
    pitch, program, on, off = score.pack([dict(pitch=61, program=3, start=0.25, end=0.5),
                                          dict(pitch=60, start=1.0000004, end=2.0000006),
                                          dict(pitch=60, program=9, start=1.0, end=2.0),
                                          dict(pitch=60, program=2, start=1.0, end=2.0)])
    assert (pitch.dtype, program.dtype, on.dtype, off.dtype) == (np.int32, np.int32, np.int64, np.int64)
    assert pitch.tolist() == [60, 60, 60, 61] and program.tolist() == [2, 9, 0, 3]       # (pitch, on, off, program)
    assert on.tolist() == [1000000, 1000000, 1000000, 250000] and off.tolist() == [2000000, 2000000, 2000001, 500000]
    for name, est, ref in corpus[:11]:                                  # seconds and back: every corpus time survives
        p = score.pack(as_dicts(est))
        assert list(zip(p[0].tolist(), p[1].tolist(), p[2].tolist(), p[3].tolist())) == \
            [(a, b, c, d) for a, b, c, d in sorted(est, key=R.sort_key)], name
    empty = score.pack([])
    assert [a.shape for a in empty] == [(0,)] * 4
    for bad in (dict(pitch=128, start=0, end=1), dict(pitch=-1, start=0, end=1), dict(pitch=5, program=128, start=0, end=1),
                dict(pitch=5, program=-1, start=0, end=1), dict(pitch=5, start=float('nan'), end=1),
                dict(pitch=5, start=0, end=float('inf'))):
        with pytest.raises(ValueError):
            score.pack([dict(pitch=60, start=0, end=1), bad])
    with pytest.raises(ValueError, match='128 entries'):
        score.group_table(np.arange(112))
    with pytest.raises(ValueError, match='as many'):
        score.score_pairs([[]], [])
    assert score.score_pairs([], []).shape == (0, 10)


def _vlq(v):
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(reversed(out))


def two_tempo_file(path):
    """Format 1, 480 ticks per quarter.  Track 0: 500 000 us per quarter at tick 0, 250 000 at tick 960.  Track 1:
    program 24 on channel 0, a note from tick 480 to tick 1440 and one from 960 to 1920; a drum note on channel 9."""
    t0 = b'\x00\xff\x51\x03' + (500000).to_bytes(3, 'big') + _vlq(960) + b'\xff\x51\x03' + (250000).to_bytes(3, 'big') + \
        b'\x00\xff\x2f\x00'
    t1 = (b'\x00\xc0\x18' + _vlq(480) + b'\x90\x40\x50' + _vlq(0) + b'\x99\x24\x60' + _vlq(480) + b'\x90\x43\x51' +
          _vlq(480) + b'\x80\x40\x00' + _vlq(0) + b'\x89\x24\x00' + _vlq(480) + b'\x80\x43\x00' + b'\x00\xff\x2f\x00')
    with open(path, 'wb') as f:
        f.write(b'MThd' + struct.pack('>IHHH', 6, 1, 2, 480))
        for t in (t0, t1):
            f.write(b'MTrk' + struct.pack('>I', len(t)) + t)


def test_read_midi_full_honours_every_tempo_and_the_default_is_unchanged(tmp_path):
    from amt_saga import events, score
    path = str(tmp_path / 'two_tempo.mid')
    two_tempo_file(path)
    # by hand: a tick is 500000 / 480 us up to tick 960 (1.0 s), 250000 / 480 us after it
    full = events.read_midi(path, full=True)
    assert [(n['pitch'], n['program'], n['channel'], n['velocity']) for n in full] == \
        [(0x24, 0, 9, 0x60), (0x40, 24, 0, 0x50), (0x43, 24, 0, 0x51)]
    assert [(n['start'], n['end']) for n in full] == [(0.5, 1.25), (0.5, 1.25), (1.0, 1.5)]
    # the default: the first tempo for the whole file, no channel -- what it always returned
    plain = events.read_midi(path)
    assert plain == events.read_midi(path, full=False)
    assert plain == [dict(pitch=0x24, program=0, velocity=0x60, start=0.5, end=1.5),
                     dict(pitch=0x40, program=24, velocity=0x50, start=0.5, end=1.5),
                     dict(pitch=0x43, program=24, velocity=0x51, start=1.0, end=2.0)]
    assert [n['pitch'] for n in score.read_gold(path)] == [0x40, 0x43]                # channel 9 dropped
    # a file the project writes has one tempo: both modes agree on it to the last bit of a microsecond
    notes = [dict(pitch=60 + k, program=k, velocity=90, start=0.37 * k, end=0.37 * k + 0.5) for k in range(5)]
    own = str(tmp_path / 'own.mid')
    events.write_midi(notes, own)
    a, b = events.read_midi(own), events.read_midi(own, full=True)
    assert [score.pack(a)[k].tolist() for k in range(4)] == [score.pack(b)[k].tolist() for k in range(4)]
    assert all('channel' not in n for n in a) and all(n['channel'] != 9 for n in b)


def test_abi_refuses_bad_arguments_before_any_hip_call():
    from amt_saga import _lib, score
    lib = _lib.load()
    p = 64                                                             # never dereferenced: checks come first
    ok_off = (ctypes.c_longlong * 3)(0, 2, 5)

    def call(offsets=ok_off, ref_offsets=ok_off, n_pairs=2, **kw):
        a = dict(est_pitch=p, est_program=p, est_on=p, est_off=p, ref_pitch=p, ref_program=p, ref_on=p, ref_off=p,
                 est_offsets_host=ctypes.addressof(offsets) if offsets is not None else None,
                 ref_offsets_host=ctypes.addressof(ref_offsets) if ref_offsets is not None else None,
                 est_offsets=p, ref_offsets=p, group=p, scratch=p, scratch_bytes=1 << 20, out=p, n_pairs=n_pairs)
        a.update(kw)
        return lib.amt_score_pairs(ctypes.byref(score.score_args(**a)), None)
    assert lib.amt_score_pairs(None, None) == _lib.AMT_E_INVALID
    for k in ('est_pitch', 'est_program', 'est_on', 'est_off', 'ref_pitch', 'ref_program', 'ref_on', 'ref_off',
              'est_offsets', 'ref_offsets', 'group', 'scratch', 'out'):
        assert call(**{k: None}) == _lib.AMT_E_INVALID, k
    assert call(offsets=None) == call(ref_offsets=None) == _lib.AMT_E_INVALID
    assert call(n_pairs=-1) == _lib.AMT_E_INVALID and call(scratch_bytes=-1) == _lib.AMT_E_INVALID
    assert call(scratch=72) == _lib.AMT_E_INVALID                                     # not 16-byte aligned
    for bad in ((0, 3, 2), (-1, 2, 5), (0, 1 << 31, 1 << 31), (2, 1, 1)):
        off = (ctypes.c_longlong * 3)(*bad)
        assert call(offsets=off) == _lib.AMT_E_INVALID and call(ref_offsets=off) == _lib.AMT_E_INVALID, bad
    need = lib.amt_score_scratch_bytes(5, 5)
    assert need == 16 + 8 * 32 + 10 * 32                               # eight arrays per estimate, ten per reference
    assert call(scratch_bytes=need - 1) == _lib.AMT_E_SHAPE
    assert call(n_pairs=0) == _lib.AMT_OK                              # nothing to do, and nothing is launched
    assert lib.amt_score_scratch_bytes(-1, 0) == lib.amt_score_scratch_bytes(0, -1) == _lib.AMT_E_INVALID
    assert lib.amt_score_scratch_bytes(0, 0) == 16 and lib.amt_score_scratch_bytes((1 << 40) + 1, 0) == _lib.AMT_E_INVALID
    # the host-visible check of pitches and programs
    good = np.array([0, 127, 60], np.int32)
    for bad in (128, -1):
        worse = np.array([0, bad, 60], np.int32)
        assert lib.amt_score_check_notes(worse.ctypes.data, good.ctypes.data, 3) == _lib.AMT_E_INVALID
        assert lib.amt_score_check_notes(good.ctypes.data, worse.ctypes.data, 3) == _lib.AMT_E_INVALID
    assert lib.amt_score_check_notes(good.ctypes.data, good.ctypes.data, 3) == _lib.AMT_OK
    assert lib.amt_score_check_notes(None, None, 0) == _lib.AMT_OK
    assert lib.amt_score_check_notes(None, good.ctypes.data, 3) == lib.amt_score_check_notes(good.ctypes.data, good.ctypes.data, -1) \
        == _lib.AMT_E_INVALID


def test_command_lines_refuse_bad_arguments_before_the_gpu(tmp_path):
    from amt_saga import score, transcribe as tr
    mid = str(tmp_path / 'a.mid')
    two_tempo_file(mid)
    missing = str(tmp_path / 'missing.mid')
    with pytest.raises(SystemExit, match='files come in pairs'):
        score.main([])
    with pytest.raises(SystemExit, match='files come in pairs'):
        score.main([mid, mid, mid])
    with pytest.raises(SystemExit, match='no such file'):
        score.main([mid, missing])
    with pytest.raises(SystemExit, match='go together'):
        score.main(['--est-dir', str(tmp_path)])
    with pytest.raises(SystemExit, match='not both'):
        score.main([mid, mid, '--est-dir', str(tmp_path), '--gold-dir', str(tmp_path)])
    with pytest.raises(SystemExit, match='not a directory'):
        score.main(['--est-dir', str(tmp_path), '--gold-dir', missing])
    os.makedirs(str(tmp_path / 'none'))
    with pytest.raises(SystemExit, match='has a gold file'):
        score.main(['--est-dir', str(tmp_path), '--gold-dir', str(tmp_path / 'none')])
    assert score.pair_by_stem(str(tmp_path), str(tmp_path / 'none')) == [('a', mid, None)]
    assert score.loop_groups().tolist() == R.MERGED
    flac = str(tmp_path / 'missing.flac')
    with pytest.raises(SystemExit, match='--gold: .*no such file'):
        tr.main([flac, str(tmp_path / 'o.mid'), '--gold', missing])
    with pytest.raises(SystemExit, match='--gold-dir: .*not a directory'):
        tr.main(['--songs', flac, '--out-dir', str(tmp_path / 'o'), '--gold-dir', missing])
    assert not os.path.exists(str(tmp_path / 'o'))
    for argv in ([flac, str(tmp_path / 'o.mid'), '--gold', mid], ['--songs', flac, '--out-dir', str(tmp_path / 'o'),
                                                                  '--gold-dir', str(tmp_path)]):
        with pytest.raises(FileNotFoundError):                         # accepted: the input file is what fails
            tr.main(argv)


def test_core_in_a_sanitised_stand_alone_program(corpus, expected, tmp_path):
    """amt_score_core.h, host only, under the address and undefined-behaviour sanitizers: the counts of every corpus pair
    (and of program_split under the merging table) from arrays of exactly the stated sizes -- and no sanitizer report (a
    report aborts the program: a nonzero exit)."""
    from amt_saga import score
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'score_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'score_host_main.cpp'), '-o', exe], check=True)
    by = {name: (est, ref) for name, est, ref in corpus}
    cases = [(est, ref, R.IDENTITY, expected[name]) for name, est, ref in corpus]
    cases.append(by['program_split'] + (R.MERGED, R.score(*by['program_split'], group=R.MERGED)))
    blob = [b'SCOR', struct.pack('<i', len(cases))]
    for est, ref, group, _ in cases:
        blob.append(struct.pack('<ii', len(est), len(ref)) + np.asarray(group, '<i4').tobytes())
        for notes in (est, ref):
            p = score.pack(as_dicts(notes))
            blob += [p[0].astype('<i4').tobytes(), p[1].astype('<i4').tobytes(), p[2].astype('<i8').tobytes(),
                     p[3].astype('<i8').tobytes()]
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        f.write(b''.join(blob))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr
    lines = r.stdout.strip().split('\n')
    assert len(lines) == len(cases)
    for k, (line, case) in enumerate(zip(lines, cases)):
        head, _, numbers = line.partition(':')
        assert head == 'case %d' % k and [int(v) for v in numbers.split()] == case[3], (k, line, case[3])
