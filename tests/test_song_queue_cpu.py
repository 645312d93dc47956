"""CPU: the host side of the song queue (TranscriptionLoop.run_song_queue) -- the admission policy and the pool's free
list against hand-written tables, and a scripted restatement of the queue (slots, polls, pool, the product's own
admission_plan and FramePool; the songs' steps from tests/song_oracle.py with scripted onsets) whose per-song records
must equal the walk of each song alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import song_oracle as so                                        # noqa: E402


def test_admission_policy_table():
    from amt_saga.loop import admission_plan
    assert admission_plan([0, 0, 0, 0], 7, 5) == []                                  # no finished slot
    assert admission_plan([1, 1, 0, 1], 3, 2) == [(0, 3), (1, 4)]                    # more finished slots than songs left
    assert admission_plan([1, 1, 1], 9, 0) == []                                     # empty queue
    assert admission_plan([0, 1, 0, 1, 1], 0, 10) == [(1, 0), (3, 1), (4, 2)]        # ascending slots, queue order
    assert admission_plan([1], 4, 1) == [(0, 4)]
    assert admission_plan([], 0, 3) == []


def test_pool_free_list():
    from amt_saga.loop import FramePool
    pool = FramePool(100)
    a, b, c = pool.alloc(30), pool.alloc(30), pool.alloc(30)
    assert (a, b, c) == (0, 30, 60)                                                  # first fit, ascending
    assert pool.alloc(20) is None                                                    # 10 frames left: wait
    assert pool.alloc(10) == 90
    pool.release(b)
    assert pool.alloc(40) is None                                                    # the hole is 30 frames: still waits
    assert pool.alloc(20) == 30 and pool.alloc(10) == 50                             # lowest fitting region first
    pool.release(a)
    pool.release(c)
    assert pool.alloc(31) is None and pool.alloc(30) == 0                            # first fit takes the lower hole
    with pytest.raises(ValueError, match='longer than the pool'):
        pool.alloc(101)
    # regions never overlap, everything returns: random traffic against a frame map
    rng = np.random.default_rng(3)
    pool, owner, live = FramePool(257), np.full(257, -1), {}
    for i in range(2000):
        if live and (rng.random() < 0.45 or len(live) > 12):
            k = list(live)[int(rng.integers(len(live)))]
            f, n = live.pop(k)
            assert np.all(owner[f:f + n] == k)
            owner[f:f + n] = -1
            pool.release(f)
        else:
            n = int(rng.integers(1, 80))
            f = pool.alloc(n)
            holes = [m for _, m in pool.free]
            if f is None:
                assert all(m < n for m in holes)
                continue
            assert np.all(owner[f:f + n] == -1), 'overlap'
            first_fit = next(s for s in range(257 - n + 1) if np.all(owner[s:s + n] == -1))
            assert f == first_fit
            owner[f:f + n] = i
            live[i] = (f, n)
    for f, _ in live.values():
        pool.release(f)
    assert pool.free == [(0, 257)] and not pool.used
    # wait-then-fit: the song that did not fit is admitted once a region has come back
    pool = FramePool(50)
    x = pool.alloc(40)
    assert pool.alloc(20) is None
    pool.release(x)
    assert pool.alloc(20) == 0
    with pytest.raises(ValueError):
        FramePool(0)


def _params():
    from amt_saga.hyperparams import Hyperparams
    return Hyperparams(N=2048, window_size_note_time=1)          # 86 frames, half = 43


def _alone(p, waves, scripts, max_notes):
    out = []
    for i, (w, sc) in enumerate(zip(waves, scripts)):
        orc = so.SongOracle(p, ('timing',), {}, subtract=False,
                            predict=lambda name, step, sc=sc: float(sc[step % len(sc)]) if name == 'timing_start' else 80.0)
        ev, _ = orc.run_song(w, {'ref_mag': 1.0}, max_notes=max_notes, silence=0.0, song_id=i)
        out.append(ev)
    return out


def _queue_restatement(p, alone, frames, slots, poll, pool_frames):
    """The queue's host logic on replayed songs: slot b plays the records of its song one per step, idles (kind FINISHED)
    when the song is over; every `poll` steps the chunk of records is split per song, finished songs are yielded and
    their regions released, free slots admit by the product's admission_plan and FramePool.  Returns ({song: records},
    finishing order, total steps, waits)."""
    from amt_saga.loop import FramePool, admission_plan
    pool = FramePool(pool_frames)
    slot_song, region, at, got, order = [-1] * slots, [None] * slots, [0] * slots, {}, []
    nxt, steps, waits, bound = 0, 0, 0, 0

    def admit():
        nonlocal nxt, waits, bound
        for slot, idx in admission_plan([s < 0 for s in slot_song], nxt, len(alone) - nxt):
            f0 = pool.alloc(frames[idx])
            if f0 is None:
                waits += 1
                break
            slot_song[slot], region[slot], at[slot], got[idx] = idx, f0, 0, []
            bound += len(alone[idx]) + 1
            nxt += 1
    admit()
    while any(s >= 0 for s in slot_song):
        chunk = np.full((poll, slots, 9), -1, np.int32)
        for r in range(poll):
            for b, idx in enumerate(slot_song):
                chunk[r, b, 2] = so.FINISHED
                if idx >= 0 and at[b] < len(alone[idx]):
                    chunk[r, b] = alone[idx][at[b]]
                    chunk[r, b, 1] = steps                          # the product records the global step
                    at[b] += 1
            steps += 1
        for b, idx in enumerate(slot_song):
            if idx < 0:
                continue
            rows = chunk[:, b]
            got[idx].append(rows[rows[:, 2] != so.FINISHED])
            if at[b] >= len(alone[idx]):
                ev = np.concatenate(got[idx])
                ev[:, 1] = np.arange(len(ev))
                got[idx] = ev
                order.append(idx)
                pool.release(region[b])
                slot_song[b] = -1
        admit()
        assert steps <= -(-bound // poll) * poll + poll
    assert nxt == len(alone) and pool.free == [(0, pool_frames)]
    return got, order, steps, waits


@pytest.mark.parametrize('slots,poll', [(2, 1), (2, 4), (3, 16), (8, 4), (16, 1)])
def test_scripted_queue_equals_each_song_alone(slots, poll):
    """Length mix where songs finish at different polls (0.3 ... 6.2 half windows, two songs of one hop), slots below
    and above the number of songs: every song's records from the queue restatement are the records of the song walked
    alone, in step order with steps renumbered from 0."""
    p = _params()
    half = p.timing_frames // 2
    rng = np.random.default_rng(5)
    hw = [2.3, 0.3, 6.2, 1.0, 4.4, 3.0, 5.1, 2.0, 3.7]
    lens = [int(h * half * p.H) for h in hw] + [p.H, p.H]         # one-hop songs: a single frame pair
    waves = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in lens]
    scripts = [[10, 12, 60], [60], [5, 70], [50], [3, 3, 3], [60, 10], [20, 61], [9, 9, 44], [70], [60], [1, 2]]
    alone = _alone(p, waves, scripts, max_notes=2)
    frames = [1 + n // p.H for n in lens]
    assert len({len(e) for e in alone}) >= 5                       # the songs take different numbers of steps
    got, order, steps, waits = _queue_restatement(p, alone, frames, slots, poll, pool_frames=slots * max(frames))
    assert sorted(order) == list(range(len(waves)))               # (first fit fragments: a wait is possible here too)
    for i, ev in enumerate(alone):
        assert np.array_equal(got[i], ev), (i, got[i].tolist(), ev.tolist())
        assert ev[:, 1].tolist() == list(range(len(ev))) and np.all(ev[:, 0] == i)
    if slots < len(waves):
        assert order != sorted(order) or poll >= 16                # short songs overtake long ones
    # a pool of one long song: songs wait for a region, the walk still ends with the same records
    got2, _, steps2, waits2 = _queue_restatement(p, alone, frames, slots, poll, pool_frames=max(frames))
    assert waits2 > 0 and steps2 >= steps
    for i, ev in enumerate(alone):
        assert np.array_equal(got2[i], ev), i


def test_song_queue_is_part_of_the_interface():
    from amt_saga import loop, transcribe
    assert callable(loop.TranscriptionLoop.run_song_queue) and callable(loop.TranscriptionLoop.iter_song_queue)
    assert callable(transcribe.transcribe_songs)
    with pytest.raises(SystemExit):
        transcribe.main(['--songs'])                                # the many-files mode parses its own arguments
