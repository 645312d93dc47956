"""CPU: piano rolls without a GPU.  The reference of tests/roll_reference.py against images drawn by hand and against
its own word-by-word form; its class counts against the frame counts of tests/score_reference.py; the corpus of the GPU
tests inside the geometry limits; the core the kernel compiles (csrc/amt_roll_core.h) writing the same bytes in a
stand-alone program built with the address and undefined-behaviour sanitizers; the host side of amt_saga.roll, the ABI
and the command lines refusing bad arguments before a GPU is touched; the 'roll' palette.  Nothing here has a
tolerance: every number is a pixel value or a count."""
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
import roll_reference as R                                         # noqa: E402
import score_reference as SR                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def corpus():
    return R.corpus()


@pytest.fixture(scope='module')
def expected(corpus):
    """{name: the reference's image}, computed once."""
    return {c['name']: R.draw(c) for c in corpus}


def as_dicts(notes):
    return [dict(pitch=p, program=g, start=on / 1e6, end=off / 1e6) for p, g, on, off in notes]


def test_reference_draws_the_images_written_out_by_hand(expected):
    cases = R.by_hand()
    assert sorted(c['name'] for c in cases) == sorted(R.EXPECTED)
    for c in cases:
        want = np.array(R.EXPECTED[c['name']], dtype=np.uint8)
        assert want.shape == (R.height(c), c['W']), c['name']
        assert R.draw_slow(c).tolist() == want.tolist(), c['name']
        assert expected[c['name']].tolist() == want.tolist(), c['name']
    # a pair with an empty gold list is not a single list
    assert R.EXPECTED['pair_empty_gold'] != R.EXPECTED['single_of_the_same']
    assert R.tick_hit(-2500, -1500, 2000) and not R.tick_hit(-1500, -500, 2000) and R.tick_hit(-1500, -500, 1500)
    assert not R.tick_hit(500, 1500, 1500) and R.tick_hit(0, 1, 7) and not R.tick_hit(1, 7, 7) and not R.tick_hit(0, 9, 0)


def test_fast_reference_equals_the_word_by_word_one_off_the_grid(corpus, expected):
    """Also `covered` against "some note of the pitch intersects the column": side_slow asserts it at every pixel."""
    small = [c for c in corpus if c['W'] * (c['pitch_hi'] - c['pitch_lo'] + 1) * (len(c['est']) + len(c['gold'] or [])) <= 400000]
    assert len(small) >= 30 and {'w1', 'w63', 'w64', 'w65', 'odd_w_px5', 'late'} <= {c['name'] for c in small}
    for c in small:
        assert R.draw_slow(c).tolist() == expected[c['name']].tolist(), c['name']
    rng = np.random.default_rng(11)
    for k in range(40):
        t0 = int(rng.integers(-10 ** 6, 10 ** 6))
        W = int(rng.integers(1, 40))
        t1 = t0 + int(rng.integers(W, 50 * W))
        notes = [R.random_notes(rng, int(rng.integers(0, 25)), 60, 62, t0, t1) for _ in range(2)]
        c = R.case('off_grid%d' % k, notes[0], notes[1] if k % 2 else None, W=W, row_px=1 + k % 3, lo=59, hi=63, t0=t0,
                   t1=t1, tick=int(rng.integers(0, 4 * W)), group=R.FOLD)
        assert R.inside_limits(c) and R.draw_slow(c).tolist() == R.draw(c).tolist(), k


def test_class_counts_equal_the_frame_counts_of_the_scoring_rule():
    """A column per 10 ms frame, every pitch, no ticks: both / estimate only / gold only = frame_tp / fp / fn."""
    pairs = R.grid_pairs(60, seed=7, pitches=(0, 59, 60, 61, 127), most=20, frames=90)
    assert sum(1 for e, g in pairs if not e or not g) >= 1
    for k, (est, gold) in enumerate(pairs):
        c = R.grid_case('g%d' % k, est, gold)
        want = SR.frame_counts(est, gold)
        assert c['W'] == max(1, want[3]) and R.class_counts(R.draw(c)) == want[:3], k


def test_corpus_stays_inside_the_geometry_limits(corpus, expected):
    names = [c['name'] for c in corpus]
    assert len(set(names)) == len(names)
    for c in corpus:
        assert R.inside_limits(c), c['name']
        assert expected[c['name']].shape == (R.height(c), c['W']) and expected[c['name']].dtype == np.uint8
    by = {c['name']: c for c in corpus}
    assert by['widest']['W'] == R.MAX_DIM and R.height(by['tallest']) == R.MAX_DIM and by['tallest']['row_px'] == 128
    assert len(by['many_notes']['est']) == 70000 > 2 ** 16 and {n[0] for n in by['many_notes']['est']} == {64}
    assert len(by['long_under_many']['est']) == 20001
    # the long note is drawn between the short ones, and is found although 20 000 notes began after it
    row = expected['long_under_many'][0]
    assert set(row.tolist()) == {R.SINGLE + 2 * 1, R.SINGLE + 2 * 2, R.SINGLE + 2 * 2 + 1}
    total = sum(R.height(c) * c['W'] for c in corpus)
    assert total < 4 << 20, total                                      # the GPU tests stay small


def write_cases(path, cases):
    from amt_saga import score
    blob = [b'ROLL', struct.pack('<i', len(cases))]
    for c in cases:
        meta = [c['W'], c['row_px'], c['pitch_lo'], c['pitch_hi'], c['t0'], c['t1'], c['tick'], int(c['gold'] is not None), 0, 0]
        blob.append(np.asarray(meta, '<i8').tobytes() + np.asarray(c['group'], '<i4').tobytes())
        blob.append(struct.pack('<ii', len(c['est']), len(c['gold'] or [])))
        for notes in (c['est'], c['gold'] or []):
            p = score.pack(as_dicts(notes))
            blob += [p[0].astype('<i4').tobytes(), p[1].astype('<i4').tobytes(), p[2].astype('<i8').tobytes(),
                     p[3].astype('<i8').tobytes()]
    with open(path, 'wb') as f:
        f.write(b''.join(blob))


def test_pack_keeps_every_corpus_time(corpus):
    from amt_saga import score
    for c in corpus:
        for notes in (c['est'], c['gold'] or []):
            p = score.pack(as_dicts(notes))
            assert list(zip(p[0].tolist(), p[1].tolist(), p[2].tolist(), p[3].tolist())) == sorted(notes, key=R.sort_key)


def test_core_in_a_sanitised_stand_alone_program(corpus, expected, tmp_path):
    """amt_roll_core.h, host only, under the address and undefined-behaviour sanitizers: the bytes of every corpus image
    from arrays of exactly the stated sizes -- and no sanitizer report (a report aborts the program: a nonzero exit)."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'roll_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'roll_host_main.cpp'), '-o', exe], check=True)
    path = str(tmp_path / 'cases.bin')
    write_cases(path, corpus)
    r = subprocess.run([exe, path], capture_output=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert b'runtime error' not in r.stderr
    want = b''.join(expected[c['name']].tobytes() for c in corpus)
    assert len(r.stdout) == len(want)
    at = 0
    for c in corpus:
        n = R.height(c) * c['W']
        assert r.stdout[at:at + n] == want[at:at + n], c['name']
        at += n
    # a geometry outside the limits is refused by the core's own check
    bad = dict(corpus[0], W=R.MAX_DIM + 1, t1=corpus[0]['t0'] + 10 ** 6)
    write_cases(path, [bad])
    r = subprocess.run([exe, path], capture_output=True)
    assert r.returncode == 3 and r.stdout == b'' and b'geometry' in r.stderr


def test_piano_rolls_refuses_bad_arguments_before_the_gpu(tmp_path):
    from amt_saga import roll
    one = [dict(pitch=60, program=3, start=0.5, end=1.0)]
    for kw, match in ((dict(width=0), 'width'), (dict(width=16385), 'width'), (dict(width=1.5), 'width'),
                      (dict(row_px=0), 'row_px'), (dict(row_px=True), 'row_px'), (dict(row_px=187), 'row_px <='),
                      (dict(pitch=(61, 60)), 'lowest pitch <='), (dict(pitch=(-1, 60)), 'lowest pitch'),
                      (dict(pitch=(0, 128)), 'highest pitch'), (dict(pitch=60), 'pitch ='),
                      (dict(span=(0.0, 0.001)), 'a span of'), (dict(span=(1.0, 0.5)), 'a span of'),
                      (dict(span=(0.0, 2.0 ** 41 / 1e6)), 'a span of'), (dict(span=(-2.0 ** 62 / 1e6 + 1, 0)), 'a span of'),
                      (dict(span=(0.0, float('nan'))), 'finite'), (dict(span=[(0, 1), (0, 1)]), 'one per image'),
                      (dict(span=(0, 1, 2)), 'one per image'),
                      (dict(tick=-1.0), 'tick'), (dict(tick=float('inf')), 'finite'), (dict(tick=2.0 ** 41 / 1e6), 'tick'),
                      (dict(group=np.arange(100)), '128 entries')):
        with pytest.raises(ValueError, match=match):
            roll.piano_rolls([one], **kw)
    with pytest.raises(ValueError, match='as many gold lists'):
        roll.piano_rolls([one], [one, one])
    with pytest.raises(ValueError, match='a list of note lists'):
        roll.piano_rolls(roll._score.pack(one))
    with pytest.raises(ValueError):                                    # a note the packer refuses
        roll.piano_rolls([[dict(pitch=128, start=0, end=1)]])
    with pytest.raises(ValueError, match='one path per image'):
        roll.save_piano_rolls([one], [str(tmp_path / 'a.png'), str(tmp_path / 'b.png')])
    assert not os.listdir(str(tmp_path))
    assert roll.piano_rolls([]) == [] and roll.piano_roll_png([], None) == []
    # the default span: up to a whole second, at least one
    packed = roll._score.pack
    assert roll._default_span(packed([]), None) == (0, 1000000)
    assert roll._default_span(packed(one), packed([dict(pitch=1, start=0, end=2.000001)])) == (0, 3000000)
    assert roll._default_span(packed(one), None) == (0, 1000000)
    assert roll.geometry(2, 100, 2, (21, 108), (0.5, 1.5), 0.25) == (100, 2, 21, 108, 176, 250000, [(500000, 1500000)] * 2)
    # the legend names exactly the values the rule can produce
    leg = roll.legend()
    assert sorted(leg) == [0, 1, 2, 3] + list(range(16, 48)) + [68, 69, 72, 74, 76, 77, 78, 79]
    assert roll.CLASS_NAMES == {1: 'estimate only', 2: 'gold only', 3: 'both'} and leg[74] == 'gold only, gold onset'
    produced = set()
    for c in R.by_hand() + R.shapes()[:8]:
        produced |= set(np.unique(R.draw(c)).tolist())
    assert produced <= set(leg) and len(produced) > 20


def test_roll_palette():
    from amt_saga import png, roll
    assert 'roll' in png.PALETTES and png.PALETTES[:2] == ('cubehelix', 'gray')
    table = png.palette('roll')
    assert table.shape == (256, 3) and table.dtype == np.uint8
    used = sorted(roll.legend())
    colours = {tuple(table[v].tolist()) for v in used}
    assert len(colours) == len(used) and (0, 0, 0) not in colours
    rest = [v for v in range(256) if v not in used]
    assert not table[rest].any()
    for g in range(16):                                                # an onset is the darker variant of its hue
        assert table[17 + 2 * g].astype(int).sum() < table[16 + 2 * g].astype(int).sum()
    assert table[0].astype(int).sum() > table[1].astype(int).sum() > table[2].astype(int).sum() > table[3].astype(int).sum()


def test_prototypes_in_the_header_and_the_binding():
    from amt_saga import _lib, roll
    header = open(os.path.join(ROOT, 'include', 'amt_saga.h')).read()
    for name in ('amt_roll_scratch_bytes', 'amt_roll_draw'):
        assert name in _lib.PROTOTYPES
        m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*(?:long long|int)\s+' + name + r'\(', header, flags=re.S)
        assert m and 'main.py:7' in m.group(1), name                   # each says what it stands for
    fields = re.search(r'typedef struct amt_roll_args \{(.*?)\} amt_roll_args;', header, flags=re.S).group(1)
    fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
    names = [n for n in re.findall(r'\*?\b([a-z_0-9]+)\s*[,;]', fields)]
    assert names == [f[0] for f in roll.RollArgs._fields_]
    build = open(os.path.join(ROOT, 'amt-saga_amd', 'build.py')).read()
    assert build.count("'amt_roll.hip'") == 2 and "'amt_roll.hip': NO_PK" in build


def test_abi_refuses_bad_arguments_before_any_hip_call():
    from amt_saga import _lib, roll
    lib = _lib.load()
    p = 64                                                             # never dereferenced: checks come first
    ok_off = (ctypes.c_longlong * 3)(0, 2, 5)
    good = [8, 2, 60, 61, 0, 8000, 1000, 0, 0, 0, 5, 1, 0, 127, -5, 5, 0, 1, 32, 0]

    def call(meta=good, est_host=ok_off, gold_host=ok_off, **kw):
        table = (ctypes.c_longlong * 20)(*meta)
        a = dict(est_pitch=p, est_program=p, est_on=p, est_off=p, gold_pitch=p, gold_program=p, gold_on=p, gold_off=p,
                 est_offsets_host=ctypes.addressof(est_host), gold_offsets_host=ctypes.addressof(gold_host),
                 est_offsets=p, gold_offsets=p, image_meta_host=ctypes.addressof(table), image_meta=p, group=p, scratch=p,
                 scratch_bytes=1 << 20, out=p, out_bytes=32 + 5 * 128, n_images=2)
        a.update(kw)
        return lib.amt_roll_draw(ctypes.byref(roll.roll_args(**a)), None)
    assert lib.amt_roll_draw(None, None) == _lib.AMT_E_INVALID
    for k in ('est_pitch', 'est_program', 'est_on', 'est_off', 'gold_pitch', 'gold_program', 'gold_on', 'gold_off',
              'est_offsets_host', 'gold_offsets_host', 'est_offsets', 'gold_offsets', 'image_meta_host', 'image_meta',
              'group', 'scratch', 'out'):
        assert call(**{k: None}) == _lib.AMT_E_INVALID, k
    assert call(n_images=-1) == call(n_images=(1 << 24) + 1) == call(scratch_bytes=-1) == call(out_bytes=-1) == _lib.AMT_E_INVALID
    assert call(scratch=72) == _lib.AMT_E_INVALID                                     # not 16-byte aligned
    for bad in ((0, 3, 2), (-1, 2, 5), (0, 1 << 31, 1 << 31), (2, 1, 1)):
        off = (ctypes.c_longlong * 3)(*bad)
        assert call(est_host=off) == _lib.AMT_E_INVALID and call(gold_host=off) == _lib.AMT_E_INVALID, bad
    for k, v in ((0, 0), (0, 16385), (1, 0), (1, 8193), (2, -1), (3, 59), (3, 128), (4, -(1 << 61) - 1), (5, 7), (5, 0),
                 (5, (1 << 40) + 1), (6, -1), (6, (1 << 40) + 1), (7, 2), (7, -1), (8, -1), (8, 641), (18, 33)):
        meta = list(good)
        meta[k] = v
        assert call(meta=meta) == _lib.AMT_E_INVALID, (k, v)
    assert call(out_bytes=32 + 5 * 128 - 1) == _lib.AMT_E_INVALID                     # the last image leaves out
    need = lib.amt_roll_scratch_bytes(5, 5)
    assert need == 16 + 2 * (48 + 32)                                  # per side int64 [5] and int32 [5], each from a 16-byte boundary
    assert call(scratch_bytes=need - 1) == _lib.AMT_E_SHAPE
    assert call(n_images=0) == _lib.AMT_OK                             # nothing to do, and nothing is launched
    assert lib.amt_roll_scratch_bytes(-1, 0) == lib.amt_roll_scratch_bytes(0, -1) == _lib.AMT_E_INVALID
    assert lib.amt_roll_scratch_bytes(0, 0) == 16 and lib.amt_roll_scratch_bytes((1 << 40) + 1, 0) == _lib.AMT_E_INVALID


def test_command_lines_refuse_bad_roll_options_before_any_file_is_read(tmp_path):
    from amt_saga import score, transcribe as tr
    flac = str(tmp_path / 'missing.flac')
    not_dir = str(tmp_path / 'file')
    with open(not_dir, 'w') as f:
        f.write('x')
    single, songs = [flac, str(tmp_path / 'o.mid')], ['--songs', flac, '--out-dir', str(tmp_path / 'o')]
    for argv in (single, songs):
        with pytest.raises(SystemExit, match='--roll-dir: .*not a directory'):
            tr.main(argv + ['--roll-dir', not_dir])
        for extra in (['--roll-width', '0'], ['--roll-width', '16385'], ['--roll-row-px', '0'], ['--roll-row-px', '187']):
            with pytest.raises(SystemExit, match='--roll-width / --roll-row-px'):
                tr.main(argv + ['--roll-dir', str(tmp_path / 'r')] + extra)
    assert not os.path.exists(str(tmp_path / 'o')) and not os.path.exists(str(tmp_path / 'r'))
    for argv in (single, songs):
        with pytest.raises(FileNotFoundError):                         # accepted: the input file is what fails
            tr.main(argv + ['--roll-dir', str(tmp_path / 'r2'), '--roll-width', '16384', '--roll-row-px', '186'])
    with pytest.raises(SystemExit, match='--roll-dir: .*not a directory'):
        score.main([flac, flac, '--roll-dir', not_dir])
    with pytest.raises(SystemExit, match='no such file'):
        score.main([flac, flac, '--roll-dir', str(tmp_path / 'r')])
    assert not os.path.exists(str(tmp_path / 'r'))
