"""GPU: the piano-roll rasteriser (amt_roll.hip) against the rule restated in tests/roll_reference.py -- every byte of
every corpus image, alone and in one call, the output prefilled with a sentinel, with gaps between the images and guard
bytes behind the output and the scratch -- then the Python surface on a non-default stream, the class counts against the
scoring kernel, the PNG files against zlib, and both command lines.  Nothing here has a tolerance."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_reference as P                                          # noqa: E402
import roll_reference as R                                         # noqa: E402
from oracle import synth as osynth                                 # noqa: E402

pytestmark = pytest.mark.gpu
SENT, GUARD, GAP = 0xEE, 64, 3                                     # (0xEE is no pixel value of the rule)


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import roll, score, _lib
    return dict(torch=torch, roll=roll, score=score, _lib=_lib, lib=_lib.load())


@pytest.fixture(scope='module')
def corpus():
    return R.corpus()


@pytest.fixture(scope='module')
def expected(corpus):
    """{name: the reference's image}, computed once."""
    return {c['name']: R.draw(c) for c in corpus}


def as_dicts(notes):
    return [dict(pitch=p, program=g, start=on / 1e6, end=off / 1e6) for p, g, on, off in notes]


def as_tuples(notes):
    """Note dicts -> the reference's tuples, the microseconds made here."""
    return [(int(n['pitch']), int(n['program']), int(np.rint(n['start'] * 1e6)), int(np.rint(n['end'] * 1e6))) for n in notes]


def _call(env, cases, group=None):
    """amt_roll_draw called directly on reference cases that share a group table: images GAP bytes apart in an output
    prefilled with a sentinel and followed by guard bytes, the scratch followed by guard bytes.  Returns the images;
    the gaps and the guards are asserted."""
    torch, lib, _lib, roll = env['torch'], env['lib'], env['_lib'], env['roll']
    from amt_saga.device import stream_ptr
    n = len(cases)
    group = cases[0]['group'] if group is None else group
    sides = []
    for key in ('est', 'gold'):
        lists = [sorted(c[key] or [], key=R.sort_key) for c in cases]
        flat = [x for notes in lists for x in notes]
        offsets = np.concatenate([[0], np.cumsum([len(notes) for notes in lists])]).astype(np.int64)
        cols = [np.array([x[k] for x in flat] + [0], dtype=dt) for k, dt in ((0, np.int32), (1, np.int32), (2, np.int64), (3, np.int64))]
        sides.append(dict(host=offsets, dev=[torch.from_numpy(a).cuda() for a in cols], off=torch.from_numpy(offsets).cuda()))
    meta, at = np.zeros((n, 10), np.int64), GAP
    for i, c in enumerate(cases):
        meta[i] = [c['W'], c['row_px'], c['pitch_lo'], c['pitch_hi'], c['t0'], c['t1'], c['tick'], int(c['gold'] is not None), at, 0]
        at += R.height(c) * c['W'] + GAP
    need = int(lib.amt_roll_scratch_bytes(int(sides[0]['host'][-1]), int(sides[1]['host'][-1])))
    assert need >= 16
    scratch = torch.full((need + GUARD,), SENT, dtype=torch.uint8).cuda()
    out = torch.full((at + GUARD,), SENT, dtype=torch.uint8).cuda()
    g = torch.from_numpy(np.asarray(group, np.int32)).cuda()
    d_meta = torch.from_numpy(meta.reshape(-1)).cuda()
    e, r = sides
    a = roll.roll_args(est_pitch=e['dev'][0], est_program=e['dev'][1], est_on=e['dev'][2], est_off=e['dev'][3],
                       gold_pitch=r['dev'][0], gold_program=r['dev'][1], gold_on=r['dev'][2], gold_off=r['dev'][3],
                       est_offsets_host=e['host'].ctypes.data, gold_offsets_host=r['host'].ctypes.data,
                       est_offsets=e['off'], gold_offsets=r['off'], image_meta_host=meta.ctypes.data, image_meta=d_meta,
                       group=g, scratch=scratch, scratch_bytes=need, out=out, out_bytes=at, n_images=n)
    assert lib.amt_roll_draw(ctypes.byref(a), stream_ptr()) == _lib.AMT_OK
    torch.cuda.synchronize()
    o, s = out.cpu().numpy(), scratch.cpu().numpy()
    assert np.all(s[need:] == SENT) and np.all(o[at:] == SENT)
    images, end = [], 0
    for i, c in enumerate(cases):
        start, size = int(meta[i, 8]), R.height(c) * c['W']
        assert np.all(o[end:start] == SENT), c['name']
        images.append(o[start:start + size].reshape(R.height(c), c['W']).copy())
        end = start + size
    assert np.all(o[end:at] == SENT)
    return images


@pytest.fixture(scope='module')
def alone(env, corpus):
    """{name: the image of the case drawn in a call of its own}."""
    return {c['name']: _call(env, [c])[0] for c in corpus}


def test_every_corpus_case_alone_equals_the_reference(corpus, expected, alone):
    """W = 1, one below / at / above a wave and the workgroup, 16384 columns, 16384 rows, unaligned row bases, empty
    sides, every edge case drawn by hand, 70 000 notes at one pitch, a long note under 20 000 short ones, times past 2^32."""
    for name, rows in R.EXPECTED.items():
        assert alone[name].tolist() == rows, name
    wrong = [c['name'] for c in corpus if not np.array_equal(alone[c['name']], expected[c['name']])]
    assert not wrong, wrong
    assert alone['pair_empty_gold'].tolist() != alone['single_of_the_same'].tolist()


def test_whole_corpus_in_one_shuffled_call_per_group_table(env, corpus, alone):
    order = np.random.default_rng(5).permutation(len(corpus))
    for table in (R.IDENTITY, R.FOLD, R.MERGED):
        cases = [corpus[int(k)] for k in order if corpus[int(k)]['group'] == table]
        assert len(cases) >= 1
        for c, img in zip(cases, _call(env, cases)):
            assert np.array_equal(img, alone[c['name']]), c['name']


def test_more_tasks_than_the_grid_cap_single_and_pair_images_mixed(env, corpus, alone):
    cases = [c for c in corpus if c['group'] == R.IDENTITY and len(c['est']) < 1000 and c['W'] < 1000]
    cases = cases + [c for c in cases if c['name'].startswith('grid')]
    tasks = sum(c['pitch_hi'] - c['pitch_lo'] + 1 for c in cases)
    assert tasks > R.GRID_CAP and 128 * len(cases) > R.GRID_CAP
    assert {c['gold'] is None for c in cases} == {True, False}
    for c, img in zip(cases, _call(env, cases)):
        assert np.array_equal(img, alone[c['name']]), c['name']


def test_python_surface_on_a_non_default_stream(env):
    """piano_rolls: one geometry, a span per image, single and pair images in one call, views of one allocation."""
    torch, roll = env['torch'], env['roll']
    rng = np.random.default_rng(17)
    spans = [(-0.25, 1.0), (0.0, 0.3), (2.0, 2.000257), (0.0, 5.0), (0.5, 0.9)]
    cases = []
    for k, (a, b) in enumerate(spans):
        t0, t1 = int(np.rint(a * 1e6)), int(np.rint(b * 1e6))
        est, gold = (R.random_notes(rng, 50, 57, 65, t0, t1) for _ in range(2))
        cases.append(R.case('s%d' % k, est, gold if k % 2 else None, W=257, row_px=2, lo=58, hi=64, t0=t0, t1=t1,
                            tick=50000, group=R.FOLD))
    assert all(R.inside_limits(c) for c in cases)
    est = [as_dicts(c['est']) for c in cases]
    gold = [None if c['gold'] is None else as_dicts(c['gold']) for c in cases]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        got = roll.piano_rolls(est, gold, width=257, row_px=2, pitch=(58, 64), span=spans, tick=0.05, group=np.asarray(R.FOLD))
        side.synchronize()
    assert len(got) == len(cases) and all(g.dtype == torch.uint8 and g.is_cuda and tuple(g.shape) == (14, 257) for g in got)
    assert got[1].data_ptr() - got[0].data_ptr() == 14 * 257
    for c, g in zip(cases, got):
        assert np.array_equal(g.cpu().numpy(), R.draw(c)), c['name']
    # packed lists, one span for all, the default pitch range and the default span
    one = roll.piano_rolls([env['score'].pack(est[3])], None, width=100, row_px=1, span=(0.0, 5.0), tick=0, group=np.asarray(R.FOLD))
    c = dict(cases[3], gold=None, W=100, row_px=1, pitch_lo=21, pitch_hi=108, tick=0)
    assert np.array_equal(one[0].cpu().numpy(), R.draw(c))
    notes = [(60, 0, 100000, 2300000)]
    auto = roll.piano_rolls([as_dicts(notes)], [[]], width=30, row_px=1, pitch=(60, 60), tick=1.0)
    assert np.array_equal(auto[0].cpu().numpy(), R.draw(R.case('auto', notes, [], W=30, lo=60, hi=60, t1=3000000, tick=1000000)))
    with pytest.raises(ValueError):                                    # a caller's own packing is checked on the host
        roll.piano_rolls([(np.array([128], np.int32), np.array([0], np.int32), np.array([0], np.int64),
                           np.array([1], np.int64))])


def test_class_counts_of_the_images_equal_the_frame_counts_of_the_scoring_kernel(env):
    roll, score = env['roll'], env['score']
    pairs = R.grid_pairs(16, seed=19, pitches=(0, 47, 60, 61, 127), most=18, frames=100)
    est, gold = [as_dicts(e) for e, _ in pairs], [as_dicts(g) for _, g in pairs]
    counts = score.score_pairs(est, gold)
    W = max(1, int(counts[:, 9].max()))                                # columns past a pair's last frame stay background
    images = roll.piano_rolls(est, gold, width=W, row_px=1, pitch=(0, 127), span=(0.0, W * 0.01), tick=0)
    for k, img in enumerate(images):
        assert R.class_counts(img.cpu().numpy()) == counts[k, 6:9].tolist(), k
    assert int(counts[:, 6].sum()) > 0 and int(counts[:, 7].sum()) > 0 and int(counts[:, 8].sum()) > 0


def test_png_files_inflate_to_the_pixels_with_the_roll_palette(env, corpus, expected):
    from amt_saga import png
    roll = env['roll']
    rng = np.random.default_rng(23)
    est = [R.random_notes(rng, 40, 60, 71, 0, 2000000) for _ in range(3)]
    gold = [None, R.random_notes(rng, 40, 60, 71, 0, 2000000), []]
    kw = dict(width=131, row_px=3, pitch=(60, 71), span=(0.0, 2.0), tick=0.5, group=np.asarray(R.MERGED))
    files = roll.piano_roll_png([as_dicts(e) for e in est], [None if g is None else as_dicts(g) for g in gold], **kw)
    table = png.palette('roll')
    for e, g, data in zip(est, gold, files):
        img, pal, chunks = P.decode(data)                              # (zlib.decompress and every CRC, in the test)
        want = R.draw(R.case('png', e, g, W=131, row_px=3, lo=60, hi=71, t1=2000000, tick=500000, group=R.MERGED))
        assert np.array_equal(img, want) and pal.tobytes() == table.tobytes() and chunks[1] == b'PLTE'


@pytest.mark.parametrize('cli', ['one_file', 'songs'])
def test_command_lines_write_the_named_files_at_the_requested_size(env, tmp_path, monkeypatch, capsys, cli):
    """A one-second synthetic song through python -m amt_saga.transcribe with and without --roll-dir, with and without
    gold, then python -m amt_saga.score --roll-dir on what was written.  Every image is the reference's for the notes
    of the files.  No quality is asserted: the synthetic heads decide what comes out."""
    from amt_saga import events, flac, png, transcribe as tr
    from amt_saga.hyperparams import Hyperparams
    score = env['score']
    p = Hyperparams(N=2048, window_size_note_time=1)
    monkeypatch.setattr(tr, 'Hyperparams', lambda **kw: Hyperparams(window_size_note_time=1, **kw))
    n = int(1.4 * p.H * (p.timing_frames - 1))
    known = [(j % 3, 60 + 2 * j, 100, 0.2 + 0.7 * j, 0.4) for j in range(int(n / p.sr / 0.7))]
    y = osynth.render_window(known, n, p.sr).numpy()
    gold = [dict(pitch=pitch, program=(0, 40, 24)[g], velocity=v, start=t0, end=t0 + d) for g, pitch, v, t0, d in known]
    gold_dir = str(tmp_path / 'gold')
    os.makedirs(gold_dir)
    events.write_midi(gold, os.path.join(gold_dir, 'clip_a.mid'))
    names = ['clip_a', 'clip_b'] if cli == 'songs' else ['clip_a']
    lens = {nm: len(y) - 3000 * k for k, nm in enumerate(names)}
    for nm in names:
        flac.save_float(y[:lens[nm]], str(tmp_path / (nm + '.flac')), p.sr)

    def run(out, extra):
        if cli == 'one_file':
            os.makedirs(out)
            tr.main([str(tmp_path / 'clip_a.flac'), os.path.join(out, 'clip_a.mid'), '--iters', '1', '--traversal', 'song',
                     '--gold', os.path.join(gold_dir, 'clip_a.mid')] + extra)
        else:
            tr.main(['--songs'] + [str(tmp_path / (nm + '.flac')) for nm in names] + ['--out-dir', out, '--slots', '2',
                    '--iters', '1', '--gold-dir', gold_dir] + extra)
    plain, rolled, rolls = str(tmp_path / 'plain'), str(tmp_path / 'rolled'), str(tmp_path / 'rolls')
    run(plain, [])
    run(rolled, ['--roll-dir', rolls, '--roll-width', '300', '--roll-row-px', '2'])
    # without --roll-dir: exactly the files as before; with it: the same files, and the rolls in their own directory
    assert sorted(os.listdir(plain)) == sorted(os.listdir(rolled)) == sorted(
        [nm + '.mid' for nm in names] + ['clip_a.score.json'] + (['scores.json'] if cli == 'songs' else []))
    assert sorted(os.listdir(rolls)) == sorted([nm + '.roll.png' for nm in names] + ['clip_a.roll.gold.png'])
    gold_read = as_tuples(score.read_gold(os.path.join(gold_dir, 'clip_a.mid')))
    table = png.palette('roll')
    for nm in names:
        written = as_tuples(events.read_midi(os.path.join(rolled, nm + '.mid'), full=True))
        t1 = int(np.rint(lens[nm] / float(p.sr) * 1e6))
        for suffix, g in (('.roll.png', None), ('.roll.gold.png', gold_read)):
            path = os.path.join(rolls, nm + suffix)
            if g is not None and nm != 'clip_a':
                assert not os.path.exists(path)
                continue
            img, pal, _ = P.decode(open(path, 'rb').read())
            assert img.shape == (88 * 2, 300) and pal.tobytes() == table.tobytes()
            want = R.draw(R.case(nm, written, g, W=300, row_px=2, lo=21, hi=108, t1=t1, tick=1000000, group=R.MERGED))
            assert np.array_equal(img, want), (nm, suffix)
    # the scoring command line: one pair-mode image per pair, at the default size over the default span
    capsys.readouterr()
    pair_dir = str(tmp_path / 'pairs')
    score.main([os.path.join(rolled, 'clip_a.mid'), os.path.join(gold_dir, 'clip_a.mid'), '--roll-dir', pair_dir])
    assert len(capsys.readouterr().out.strip().split('\n')) == 2       # the JSON lines, as without the option
    assert os.listdir(pair_dir) == ['clip_a.roll.png']
    img, pal, _ = P.decode(open(os.path.join(pair_dir, 'clip_a.roll.png'), 'rb').read())
    written = as_tuples(events.read_midi(os.path.join(rolled, 'clip_a.mid'), full=True))
    top = max([x[3] for x in written + gold_read] + [0])
    want = R.draw(R.case('pair', written, gold_read, W=1200, row_px=5, lo=21, hi=108, t1=max(1, -(-top // 10 ** 6)) * 10 ** 6,
                         tick=1000000, group=R.MERGED))
    assert img.shape == (440, 1200) and np.array_equal(img, want) and pal.tobytes() == table.tobytes()
