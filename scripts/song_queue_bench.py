"""Song queue against fixed batches, the ragged STFT against one call per song, and the admit kernel in GB/s.

    python scripts/song_queue_bench.py [songs] [slots] [result.json] [--mix short|wide|both] [--repeats 3] [--only kernels]

Workload family of scripts/song_loop_bench.py: N = 2048, 516-frame windows, timing + pitch + velocity, max_notes = 4.
Mix 'short': songs of 3-6 half windows; mix 'wide': 3-60 half windows.
  end to end   run_song_queue over all songs (set-up included) against successive run_songs calls of `slots` songs each
               -- the only way to walk more songs than one batch before the queue -- same process, order alternated.
  set-up       amt_stft_mag_ragged on `slots` songs in one launch against one AudioBatch.stft call per song; GB/s on
               compulsory bytes (samples in, magnitudes + phases out).
  admit        every slot admitting; compulsory bytes per slot: timing_frames x ldf x 12 B read and as many written."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd')]
import ctypes as C
import numpy as np
import torch
from amt_saga import _lib, synth
from amt_saga.audio import AudioBatch, _plan, ldf_of
from amt_saga.hyperparams import Hyperparams
from amt_saga.loop import SONG_DETECT, SONG_FINISHED, TranscriptionLoop

args = [a for a in sys.argv[1:] if not a.startswith('--')]
opts = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i].startswith('--')}
for v in opts.values():
    args.remove(v)
n_songs = int(args[0]) if len(args) > 0 else 1024
slots = int(args[1]) if len(args) > 1 else 256
mixes = {'short': ['short'], 'wide': ['wide'], 'both': ['short', 'wide']}[opts.get('--mix', 'both')]
repeats = int(opts.get('--repeats', 3))
p = Hyperparams(N=2048)
tf, half, ldf = p.timing_frames, p.timing_frames // 2, ldf_of(p.N)
lib = _lib.load()
out = {'songs': n_songs, 'slots': slots, 'n_fft': p.N, 'timing_frames': tf, 'max_notes': 4}
L = p.H * (tf - 1)


def events_timed(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(v):
    return dict(min=min(v), max=max(v), all=v)


def make_songs(lens_hw, seed0):
    """Songs cut from one bank of synthetic windows (three notes per window); device tensors, for both ways alike."""
    bank = synth.make_windows(64, L, seed=seed0, notes_per_window=(3, 3), max_onset=0.8 * 6, device='cuda')[0]
    songs = []
    for i, hw in enumerate(lens_hw):
        n = int(hw) * half * p.H
        k = -(-n // L)
        rows = [(i * 7 + j) % 64 for j in range(k)]
        songs.append(bank[rows].reshape(-1)[:n].contiguous())
    return songs


# ---- admit kernel alone ------------------------------------------------------------------------------------------
B = slots
dev = 'cuda'
T_song = 6 * half
s_mag = torch.rand(B * T_song, ldf, device=dev)
s_ph = torch.rand(B * T_song, ldf, 2, device=dev)
w_mag, w_ph = torch.rand(B, tf, ldf, device=dev), torch.rand(B, tf, ldf, 2, device=dev)
i32 = lambda v: torch.as_tensor(v, dtype=torch.int32, device=dev).contiguous()
i64 = lambda v: torch.as_tensor(v, dtype=torch.int64, device=dev).contiguous()
fb, ts = i64(np.arange(B) * T_song), i32(np.full(B, T_song))
admit, zero64, song = i32(np.arange(1, B + 1)), i64(np.zeros(B)), i32(np.arange(B))
state = {k: i32(np.zeros(B)) for k in ('t_song', 'slot_song', 'offset', 'count', 'finished', 'clean')}
state64 = {k: i64(np.zeros(B)) for k in ('frame_base', 'sample_base')}
a = _lib.song_admit_args(w_mag=w_mag, w_ph=w_ph, s_mag=s_mag, s_ph=s_ph, admit=admit, new_frame_base=fb, new_t_song=ts,
                         new_sample_base=zero64, new_song=song, w_stride=tf * ldf, B=B, n_new=B, T=tf, ldf=ldf, K=0, S=0,
                         **state, **state64)
off, cnt, fin, ones = i32(np.zeros(B)), i32(np.zeros(B)), i32(np.zeros(B)), i32(np.ones(B))


def admit_all():
    _lib.check(lib.amt_song_admit(C.byref(a), None))


def slide_all():
    off.zero_()                                                    # every launch slides from offset 0 (timed alone below)
    _lib.check(lib.amt_song_slide(w_mag.data_ptr(), w_ph.data_ptr(), B, tf, ldf, tf * ldf, s_mag.data_ptr(),
                                  s_ph.data_ptr(), fb.data_ptr(), ts.data_ptr(), ones.data_ptr(), off.data_ptr(),
                                  cnt.data_ptr(), fin.data_ptr(), None))


bytes_admit = B * tf * ldf * 12 * 2
bytes_slide = B * half * ldf * 12 * 4
ms_a, ms_s = [], []
ms_z = []
for _ in range(3):
    ms_a.append(events_timed(admit_all, 200)); ms_s.append(events_timed(slide_all, 200))
    ms_z.append(events_timed(off.zero_, 200))
# the slide yardstick carries one offset reset per launch that the admit side does not have: slide_net_* takes the
# reset's own time (launched back to back, an upper bound of what it adds) off again
out['admit'] = dict(offset_reset_ms=ms_z, slide_net_GBps=bytes_slide / (min(ms_s) - min(ms_z)) / 1e6,compulsory_MB=bytes_admit / 1e6, admit_ms=ms_a, admit_GBps=bytes_admit / min(ms_a) / 1e6,
                    admit_GBps_spread=[bytes_admit / m / 1e6 for m in ms_a],
                    slide_ms=ms_s, slide_GBps=bytes_slide / min(ms_s) / 1e6)
print('admit', json.dumps(out['admit']), flush=True)
del s_mag, s_ph, w_mag, w_ph
if opts.get('--only') == 'kernels':
    print(json.dumps(out))
    sys.exit(0)

# ---- set-up: ragged STFT of `slots` songs in one launch against one call per song ---------------------------------------
rng = np.random.default_rng(0)
lens_hw = rng.integers(3, 7, slots)
songs_dev = make_songs(lens_hw, 1000)
lens = [int(s.numel()) for s in songs_dev]
t_song = [1 + n // p.H for n in lens]
fbase = np.concatenate(([0], np.cumsum(t_song)))
pool = int(fbase[-1])
samples = torch.zeros(pool * p.H, device=dev)
for s, f0 in zip(songs_dev, fbase[:-1]):
    samples[int(f0) * p.H:int(f0) * p.H + s.numel()] = s
pm, pp, rm = torch.empty(pool, ldf, device=dev), torch.empty(pool, ldf, 2, device=dev), torch.empty(slots, device=dev)
d_fb, d_sb, d_len = i64(fbase[:-1]), i64(fbase[:-1] * p.H), i32(lens)
plan = _plan(p.N, p.H, True)


def ragged():
    _lib.check(lib.amt_stft_mag_ragged(plan, samples.data_ptr(), d_sb.data_ptr(), d_len.data_ptr(), slots, max(lens),
                                       samples.numel(), sum(lens), pm.data_ptr(), pp.data_ptr(), rm.data_ptr(),
                                       d_fb.data_ptr(), pool, ldf, None))


def per_song():
    for s in songs_dev:
        AudioBatch(s[None, :], p.N, p.H).stft(with_phase=True)


bytes_stft = sum(lens) * 4 + pool * ldf * 12
ms_r, ms_p = [], []
for _ in range(3):
    ms_r.append(events_timed(ragged, 20)); ms_p.append(events_timed(per_song, 3))
one = AudioBatch(songs_dev[0][None, :], p.N, p.H).stft(with_phase=True)
out['stft_setup'] = dict(songs=slots, compulsory_MB=bytes_stft / 1e6, ragged_ms=ms_r, per_song_ms=ms_p,
                         ragged_GBps=bytes_stft / min(ms_r) / 1e6, per_song_GBps=bytes_stft / min(ms_p) / 1e6,
                         bit_identical_song0=bool(torch.equal(pm[:t_song[0]], one.mag[0]) and torch.equal(pp[:t_song[0]], one.ph[0])))
print('stft', json.dumps(out['stft_setup']), flush=True)
del samples, pm, pp, songs_dev

# ---- end to end ------------------------------------------------------------------------------------------------------
lp = TranscriptionLoop(p, heads=('timing', 'pitch', 'velocity'), iters=4).setup_device()


def by_queue(songs):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    evs = lp.run_song_queue(iter(songs), slots, max_notes=4, silence=1e-3, poll=16)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    ss = lp.queue_stats['slot_steps']
    tot = float(sum(ss))
    return dict(seconds=dt, steps=lp.queue_stats['steps'], notes=int(sum((e[:, 2] == SONG_DETECT).sum() for e in evs)),
                idle=ss[3] / tot, sliding=(ss[1] + ss[2]) / tot, detecting=ss[0] / tot, waits=lp.queue_stats['waits'],
                admissions=lp.queue_stats['admissions'])


def by_batches(songs):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    kinds, steps = np.zeros(4), 0
    for b0 in range(0, len(songs), slots):
        ev, _ = lp.run_songs(songs[b0:b0 + slots], max_notes=4, silence=1e-3, poll=16, song0=b0)
        e = ev.cpu().numpy()
        kinds += np.bincount(e[..., 2].ravel(), minlength=4)
        steps += e.shape[0]
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    tot = float(kinds.sum())
    return dict(seconds=dt, steps=steps, notes=int(kinds[0]), idle=kinds[3] / tot, sliding=(kinds[1] + kinds[2]) / tot,
                detecting=kinds[0] / tot)


warm = make_songs([3] * 8, 900)
lp.run_songs(warm, max_notes=4); lp.run_song_queue(warm, 8, max_notes=4); torch.cuda.synchronize()
out['end_to_end'] = {}
for mix in mixes:
    rng = np.random.default_rng(1)
    lens_hw = rng.integers(3, 7, n_songs) if mix == 'short' else rng.integers(3, 61, n_songs)
    songs = make_songs(lens_hw, 2000)
    q, f = [], []
    for r in range(repeats):
        for which in (('q', 'f') if r % 2 == 0 else ('f', 'q')):
            (q if which == 'q' else f).append(by_queue(songs) if which == 'q' else by_batches(songs))
            print(mix, which, json.dumps((q if which == 'q' else f)[-1]), flush=True)
    assert len({x['notes'] for x in q + f}) == 1, 'the two ways found different notes'
    res = dict(half_windows=[int(lens_hw.min()), int(lens_hw.max())], queue=q, batches=f,
               queue_notes_per_s=spread([x['notes'] / x['seconds'] for x in q]),
               batches_notes_per_s=spread([x['notes'] / x['seconds'] for x in f]),
               queue_seconds=spread([x['seconds'] for x in q]), batches_seconds=spread([x['seconds'] for x in f]))
    res['queue_faster_beyond_spread'] = res['queue_seconds']['max'] < res['batches_seconds']['min']
    res['speedup_min_over_min'] = res['batches_seconds']['min'] / res['queue_seconds']['min']
    out['end_to_end'][mix] = res
print(json.dumps(out))
if len(args) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(args[2])), exist_ok=True)
    with open(args[2], 'w') as fh:
        json.dump(out, fh, indent=1)
