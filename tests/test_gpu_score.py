"""GPU: the scoring kernel (amt_score.hip) against the rule restated in tests/score_reference.py -- all ten integers of
every corpus pair, alone and in one call, outputs prefilled with a sentinel and followed by guard words -- then the
Python surface, a non-default stream, and a song through the queue and the command line.  Nothing here has a
tolerance."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_reference as R                                        # noqa: E402
from oracle import synth as osynth                                 # noqa: E402

pytestmark = pytest.mark.gpu
SENT, GUARD, OUT_SENT = 0xAB, 64, -7


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import score, _lib
    return dict(torch=torch, score=score, _lib=_lib, lib=_lib.load())


@pytest.fixture(scope='module')
def corpus():
    return R.corpus()


@pytest.fixture(scope='module')
def expected(corpus):
    """{name: the reference's ten counts under the identity table}, computed once."""
    return {name: R.score(est, ref) for name, est, ref in corpus}


def as_dicts(notes):
    return [dict(pitch=p, program=g, start=on / 1e6, end=off / 1e6) for p, g, on, off in notes]


def as_tuples(notes):
    """Note dicts -> the reference's tuples, the microseconds made here."""
    return [(int(n['pitch']), int(n['program']), int(np.rint(n['start'] * 1e6)), int(np.rint(n['end'] * 1e6))) for n in notes]


def _call(env, pairs, group=R.IDENTITY):
    """amt_score_pairs called directly on [(estimates, references)] of reference tuples: the output prefilled and
    followed by guard words, the scratch followed by guard bytes.  Returns the rows; the guards are asserted."""
    torch, lib, _lib, score = env['torch'], env['lib'], env['_lib'], env['score']
    from amt_saga.device import stream_ptr
    n = len(pairs)
    sides = []
    for k in range(2):
        lists = [sorted(p[k], key=R.sort_key) for p in pairs]
        flat = [x for notes in lists for x in notes]
        offsets = np.concatenate([[0], np.cumsum([len(notes) for notes in lists])]).astype(np.int64)
        cols = [np.array([x[c] for x in flat] + [0], dtype=dt) for c, dt in ((0, np.int32), (1, np.int32), (2, np.int64), (3, np.int64))]
        sides.append(dict(host=offsets, dev=[torch.from_numpy(c).cuda() for c in cols], off=torch.from_numpy(offsets).cuda()))
    need = int(lib.amt_score_scratch_bytes(int(sides[0]['host'][-1]), int(sides[1]['host'][-1])))
    assert need >= 16
    scratch = torch.full((need + GUARD,), SENT, dtype=torch.uint8).cuda()
    out = torch.full((n * 10 + 8,), OUT_SENT, dtype=torch.int64).cuda()
    g = torch.from_numpy(np.asarray(group, np.int32)).cuda()
    e, r = sides
    a = score.score_args(est_pitch=e['dev'][0], est_program=e['dev'][1], est_on=e['dev'][2], est_off=e['dev'][3],
                         ref_pitch=r['dev'][0], ref_program=r['dev'][1], ref_on=r['dev'][2], ref_off=r['dev'][3],
                         est_offsets_host=e['host'].ctypes.data, ref_offsets_host=r['host'].ctypes.data,
                         est_offsets=e['off'], ref_offsets=r['off'], group=g, scratch=scratch, scratch_bytes=need, out=out,
                         n_pairs=n)
    assert lib.amt_score_pairs(ctypes.byref(a), stream_ptr()) == _lib.AMT_OK
    torch.cuda.synchronize()
    o, s = out.cpu().numpy(), scratch.cpu().numpy()
    assert np.all(o[n * 10:] == OUT_SENT) and np.all(s[need:] == SENT)
    return o[:n * 10].reshape(n, 10).tolist()


@pytest.fixture(scope='module')
def alone(env, corpus):
    """{name: the row of the pair scored in a call of its own}."""
    return {name: _call(env, [(est, ref)])[0] for name, est, ref in corpus}


def test_every_corpus_pair_alone_equals_the_reference(corpus, expected, alone):
    """Empty sides, the augmenting example, the tolerance edges, programs, 70 candidates per reference, 3000-note chains
    whose maximum needs paths of 300 references, times past 2^32, pitches 0 and 127, the frame edges, 200 random pairs."""
    assert alone['augment'] == R.AUGMENT_ROW and alone['frame_edges'] == R.FRAME_EDGES_ROW
    assert alone['tolerance_edges'][:6] == R.TOLERANCE_EDGES_NOTES
    assert alone['long_chain'][:6] == [3000] * 6
    wrong = [(name, alone[name], expected[name]) for name, _, _ in corpus if alone[name] != expected[name]]
    assert not wrong, wrong[:5]


def test_whole_corpus_in_one_shuffled_call_with_empty_pairs_between(env, corpus, alone):
    order = np.random.default_rng(5).permutation(len(corpus))
    pairs, names = [], []
    for k in order:
        name, est, ref = corpus[int(k)]
        pairs += [(est, ref), ([], [])]
        names += [name, None]
    rows = _call(env, pairs)
    assert len(rows) == 2 * len(corpus)
    for name, row in zip(names, rows):
        assert row == (alone[name] if name else [0] * 10), name


def test_a_group_table_that_merges_programs(env, corpus, expected):
    by = {name: (est, ref) for name, est, ref in corpus}
    names = ['program_split', 'dense_cluster', 'pitch_edges'] + ['random%03d' % k for k in range(40)]
    rows = _call(env, [by[nm] for nm in names], group=R.MERGED)
    for nm, row in zip(names, rows):
        assert row == R.score(*by[nm], group=R.MERGED), nm
    # the table changes counts where it merges programs that meet: 40 with 48 in program_split, 0 with 127 in pitch_edges
    assert rows[0][2:6] == [5, 5, 4, 4] and expected['program_split'][2:6] == [5, 5, 3, 3]
    assert rows[2][2:6] == [2, 2, 2, 2] and expected['pitch_edges'][2:6] == [2, 2, 1, 1]


def test_python_surface_on_a_non_default_stream(env, corpus, expected):
    torch, score = env['torch'], env['score']
    some = [c for c in corpus if not c[0].startswith('random')] + corpus[-20:]
    est, ref = [as_dicts(c[1]) for c in some], [as_dicts(c[2]) for c in some]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        got = score.score_pairs(est, ref)
    assert got.dtype == np.int64 and got.shape == (len(some), 10)
    assert got.tolist() == [expected[c[0]] for c in some]
    packed = score.score_pairs([score.pack(e) for e in est], ref, group=np.asarray(R.MERGED))
    assert packed.tolist() == [R.score(c[1], c[2], group=R.MERGED) for c in some]
    s = score.summary(got)
    k = [c[0] for c in some].index('augment')
    assert s['pairs'][k]['onset_offset'] == dict(precision=1.0, recall=1.0, f=1.0)
    assert s['pairs'][k]['frame'] == dict(precision=100 / 110, recall=1.0, f=2 * (100 / 110) / (100 / 110 + 1.0))
    assert s['micro']['counts']['n_est'] == int(got[:, 0].sum())
    with pytest.raises(ValueError):                                    # a caller's own packing is checked on the host
        score.score_pairs([(np.array([128], np.int32), np.array([0], np.int32), np.array([0], np.int64),
                            np.array([1], np.int64))], [[]])


def test_a_rendered_song_through_the_queue_and_the_command_line(env, tmp_path, monkeypatch, capsys):
    """A short song rendered from a known note list at 86-frame windows: transcribe_songs -> score_pairs equals the
    reference on the same two lists; --songs ... --gold-dir writes the same counts the reference gives on the files.
    No quality is asserted: the synthetic heads decide what comes out."""
    from amt_saga import events, flac, transcribe as tr
    from amt_saga.hyperparams import Hyperparams
    score = env['score']
    p = Hyperparams(N=2048, window_size_note_time=1)
    assert p.timing_frames == 86
    n = int(1.4 * p.H * (p.timing_frames - 1))
    known = [(j % 3, 60 + 2 * j, 100, 0.2 + 0.7 * j, 0.4) for j in range(int(n / p.sr / 0.7))]
    y = osynth.render_window(known, n, p.sr).numpy()
    gold = [dict(pitch=pitch, program=(0, 40, 24)[g], velocity=v, start=t0, end=t0 + d) for g, pitch, v, t0, d in known]
    songs = [y, y[:len(y) - 5000]]
    got = tr.transcribe_songs(songs, p, slots=2, iters=1)
    est = [item[0] for item in got]
    counts = score.score_pairs(est, [gold, gold], group=score.loop_groups())
    assert counts.tolist() == [R.score(as_tuples(e), as_tuples(gold), group=R.MERGED) for e in est]
    assert counts[:, 1].tolist() == [len(gold)] * 2

    monkeypatch.setattr(tr, 'Hyperparams', lambda **kw: Hyperparams(window_size_note_time=1, **kw))
    gold_dir, out_dir = str(tmp_path / 'gold'), str(tmp_path / 'mid')
    os.makedirs(gold_dir)
    events.write_midi(gold, os.path.join(gold_dir, 'clip_a.mid'))
    for name, wf in zip(('clip_a', 'clip_b'), songs):
        flac.save_float(wf, str(tmp_path / (name + '.flac')), p.sr)
    capsys.readouterr()
    tr.main(['--songs', str(tmp_path / 'clip_a.flac'), str(tmp_path / 'clip_b.flac'), '--out-dir', out_dir, '--slots', '2',
             '--iters', '1', '--gold-dir', gold_dir])
    assert 'clip_b: no gold file' in capsys.readouterr().err
    assert sorted(os.listdir(out_dir)) == ['clip_a.mid', 'clip_a.score.json', 'clip_b.mid', 'scores.json']
    written = as_tuples(events.read_midi(os.path.join(out_dir, 'clip_a.mid'), full=True))
    gold_read = as_tuples([g for g in events.read_midi(os.path.join(gold_dir, 'clip_a.mid'), full=True) if g['channel'] != 9])
    assert len(gold_read) == len(gold)
    want = dict(zip(R.COLUMNS, R.score(written, gold_read, group=R.MERGED)))
    with open(os.path.join(out_dir, 'clip_a.score.json')) as f:
        one = json.load(f)
    with open(os.path.join(out_dir, 'scores.json')) as f:
        whole = json.load(f)
    assert one['counts'] == want and one['name'] == 'clip_a'
    assert whole['counts'] == want and whole['pairs'] == 1 and [s['name'] for s in whole['songs']] == ['clip_a']
    assert one['onset'] == score.summary([list(want.values())])['pairs'][0]['onset']
