#!/usr/bin/env python3
"""Test infrastructure: fixtures of the song walk (tests/song_oracle.py), computed on the CPU by the restatement and
committed as tests/golden/song_fixtures.npz.

    python tests/golden/gen_song_fixtures.py [full] [screen]        (default: both)

  full    the walk with the real 33-layer heads at the production window (516 frames, half = 258) on the two songs of
          song_oracle.FULL, on the restatement's OWN song-level normalisers: events, every pre-rounding head float, the
          final residual window as per-frame maxima and 20-band compression (util_audio.py:436-466).  A fixture cannot
          hand a near-tie over, so the script fails if any decision lies closer than 10 x its band to a rounding
          boundary.  tests/test_gpu_song_loop.py replays it.
  screen  the seeds of the live parity cases (song_oracle.WALK_CASES): the restatement ALONE, once with float32 and once
          with float64 heads; per case the live steps, the decisions inside their tie band and whether the two runs
          agree on every integer.  A case is usable when at most 1 step in 10 has a decision inside a band; the counts
          are stored and repeated beside WALK_CASES' use in the test.

The audio is re-rendered from seeded note lists (24-bit quantised for `full`); the script reads nothing outside the
repository.  Run time on 8 cores: full 101 s, screen 239 s."""
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, 'amt-saga_amd'), os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import song_oracle as so                                      # noqa: E402
from oracle import synth as osynth                            # noqa: E402
from oracle.compare import FLOAT_TOL                          # noqa: E402

OUT = os.path.join(HERE, 'song_fixtures.npz')
REF_KEYS = ('ref_mag', 'ref_C_1', 'ref_C_foc')
MARGIN = 10.0


def _oracle(p, guess, shift, dtype):
    from amt_saga import synth
    from amt_saga.loop import TranscriptionLoop
    lp = TranscriptionLoop(p, heads=so.HEADS, guess=guess)       # host side only: the seeded weights
    weights = {k: {n: v.copy() for n, v in net.weights.items()} for k, net in lp.nets.items()}
    if shift:
        weights['timing_start']['dense2/bias'] = weights['timing_start']['dense2/bias'] + np.float32(shift)
    table = synth.prog_group_table(p.instrument_classes)
    bank_len = int(round((1.0 + osynth.TAIL_SECONDS) * p.sr))

    def guess_fn(program, pitch, velocity, frames):
        dur = min(float(np.float32(frames) * np.float32(p.H / p.sr)), 1.0)
        return osynth.render_window([(int(table[program]), pitch, velocity if velocity > 0 else 100, 0.0, dur)],
                                    bank_len, p.sr).numpy()
    bank = osynth.guess_bank_waves((0,), p.pitch_low, p.pitch_high, sr=p.sr) if guess == 'bank' else None
    return so.SongOracle(p, so.HEADS, weights, bank_waves=bank, guess_fn=guess_fn if guess == 'render' else None,
                         dtype=dtype)


def _job(args):
    """One song through the restatement.  Returns (events, decisions, refs, final window)."""
    from amt_saga.hyperparams import Hyperparams
    n_fft, wsec, guess, shift, dtype, wave, max_notes, silence = args
    p = Hyperparams(N=n_fft, window_size_note_time=wsec) if wsec else Hyperparams(N=n_fft)
    orc = _oracle(p, guess, shift, np.float64 if dtype == 'f64' else np.float32)
    refs = orc.ref_levels(wave)
    ev, mag = orc.run_song(wave, {k: float(v) for k, v in refs.items()}, max_notes, silence)
    dec = [(name, it, np.asarray(y, np.float64).ravel(), margin) for name, it, y, margin, v, forced in orc.decisions]
    return ev, dec, np.array([refs[k] for k in REF_KEYS], np.float64), np.asarray(mag[:, :p.timing_frames], np.float32)


def gen_full(pool):
    from amt_saga.hyperparams import Hyperparams
    from oracle import audio as oa
    c = so.FULL
    p = Hyperparams(N=c['n_fft'])
    songs = so.make_songs(p, c['seed'], c['lengths'], gap=c['gap'], quantise=True)
    res = pool.map(_job, [(c['n_fft'], None, 'bank', 0, 'f32', w, c['max_notes'], c['silence']) for w in songs])
    out, kept = {}, []
    for cand, (ev, dec, refs, mag) in enumerate(res):
        worst = min(m / FLOAT_TOL[n] for n, _, _, m in dec)
        print('candidate %d: %d steps, worst margin %.1f bands' % (cand, len(ev), worst))
        if worst < MARGIN or len(kept) == c['keep']:
            continue
        j = len(kept)
        kept.append(cand)
        out['full_%d_events' % j] = ev
        out['full_%d_refs' % j] = refs
        out['full_%d_dec_name' % j] = np.array([n for n, _, _, _ in dec])
        out['full_%d_dec_step' % j] = np.array([it for _, it, _, _ in dec], np.int32)
        out['full_%d_dec_float' % j] = np.array([y[0] for _, _, y, _ in dec], np.float64)
        out['full_%d_fmax' % j] = mag.max(axis=0)
        out['full_%d_bands' % j] = oa.AudioCompleteOracle.compress_bands(mag, bands=p.timing_bands).astype(np.float32)
        out['full_%d_samples' % j] = np.int64(len(songs[cand]))
        out['full_%d_wave_sum' % j] = np.float64(np.abs(songs[cand].astype(np.float64)).sum())
        print('full song %d: %d steps, kinds %s, worst margin %.1f bands' % (j, len(ev), ev[:, 2].tolist(), worst))
    assert len(kept) == c['keep'], 'too few candidates without a near-tie: add lengths to song_oracle.FULL'
    out['full_kept'] = np.array(kept, np.int32)
    return out


def gen_screen(pool):
    from amt_saga.hyperparams import Hyperparams
    jobs, index = [], []
    for name, (n_fft, wsec, guess, seed, lengths, max_notes, silence, silent, shift) in so.WALK_CASES.items():
        songs = so.make_songs(Hyperparams(N=n_fft, window_size_note_time=wsec), seed, lengths, silent)
        for dtype in ('f32', 'f64'):
            for i, w in enumerate(songs):
                jobs.append((n_fft, wsec, guess, shift, dtype, w, max_notes, silence))
                index.append((name, dtype, i))
    res = pool.map(_job, jobs, chunksize=1)
    out = {}
    for name in so.WALK_CASES:
        row = []
        for dtype in ('f32', 'f64'):
            r = [res[k] for k, ix in enumerate(index) if ix[0] == name and ix[1] == dtype]
            live = sum(len(ev) for ev, _, _, _ in r)
            near = sum(int(m < FLOAT_TOL[n]) for _, dec, _, _ in r for n, _, _, m in dec)
            row += [live, near]
        a = [res[k][0] for k, ix in enumerate(index) if ix[0] == name and ix[1] == 'f32']
        b = [res[k][0] for k, ix in enumerate(index) if ix[0] == name and ix[1] == 'f64']
        same = int(all(np.array_equal(x, y) for x, y in zip(a, b)))
        out['screen_' + name] = np.array(row + [same], np.int32)
        print('screen %-12s f32: %d live steps, %d decisions in a band; f64: %d / %d; integers agree: %d' %
              (name, row[0], row[1], row[2], row[3], same))
        assert row[1] * 10 <= row[0] and row[3] * 10 <= row[2], name
    return out


if __name__ == '__main__':
    what = sys.argv[1:] or ['full', 'screen']
    t0 = time.time()
    new = {}
    with mp.Pool(min(16, len(os.sched_getaffinity(0)))) as pool:
        if 'full' in what:
            new.update(gen_full(pool))
        if 'screen' in what:
            new.update(gen_screen(pool))
    old = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    old.update(new)
    np.savez_compressed(OUT, **old)
    print('wrote %s (%d bytes) in %.0f s' % (OUT, os.path.getsize(OUT), time.time() - t0))
