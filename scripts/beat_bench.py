"""Beat tracking, measured: `songs` click songs of five minutes at 44100 Hz, n_fft 2048, hop 512 (25 840 frames of 1 025
bins each, tempi spread over 70 .. 170 bpm): amt_beat_envelope alone on their spectrograms, amt_beat_track alone on their
envelopes (all songs, and one song alone: what one workgroup's DP costs), beat.beat_track end to end, and
tests/beat_reference.py on ONE song on the host, fed the device's magnitudes.  One run: five rounds of each device
measurement after a warm-up at the timed shape.

    python scripts/beat_bench.py [songs] [result.json]

The JSON result is printed; with a second argument it is also written to that file.  The DP of a song runs in one
workgroup, one barrier per chunk of ceil(period / 2) frames and one per 1024 local scores swept into LDS: the barrier
counts are reported beside the times."""
import ctypes
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from amt_saga import _lib, beat

songs = int(sys.argv[1]) if len(sys.argv) > 1 else 16
N, hop, sr, seconds = 2048, 512, 44100, 300
n_samples = seconds * sr
T = 1 + n_samples // hop
lib = _lib.load()
p = beat.params(sr, hop)
out = dict(songs=songs, n_fft=N, hop=hop, sr=sr, frames_per_song=T, lags=[int(p[0]), int(p[1])], w=int(p[2]),
           device=torch.cuda.get_device_name(0))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(fn, reps):
    for _ in range(3):                                             # warm up at the timed shape
        fn()
    torch.cuda.synchronize()
    ms = [timed(fn, reps) for _ in range(5)]
    return dict(ms=ms, repetitions_per_round=reps, best_ms=min(ms), median_ms=sorted(ms)[2])


# ---- the songs: a decaying tone and a noise click per beat, made on the device ------------------------------------------
gen = torch.Generator(device='cuda').manual_seed(0)
bpms = [70.0 + 100.0 * i / max(1, songs - 1) for i in range(songs)]
waves = []
at = torch.arange(n_samples, device='cuda', dtype=torch.float32)
for bpm in bpms:
    period = 60.0 * sr / bpm
    since = torch.remainder(at, period) / sr                       # seconds since the last beat
    tone = torch.sin(2 * np.pi * 220.0 * since) * torch.exp(-since / 0.08)
    click = (torch.rand(n_samples, device='cuda', generator=gen) * 2 - 1) * torch.exp(-since / 0.003)
    waves.append((0.5 * tone + 0.4 * click + 0.01 * (torch.rand(n_samples, device='cuda', generator=gen) * 2 - 1)).contiguous())
del at, since, tone, click
out['bpm'] = bpms

keep = {}
found = beat.beat_track(waves, sr, n_fft=N, hop=hop, keep=keep)
mag, refs, env, bases, frames = keep['mag'], keep['refs'], keep['env'], keep['frame_base'], keep['frames']
pool_frames, ldf, F = int(mag.shape[0]), int(mag.shape[1]), N // 2 + 1
out['periods'] = [r['period'] for r in found]
out['beats_found'] = [len(r['beats']) for r in found]
out['tempo_found'] = [r['tempo'] for r in found]


def dp_barriers(frames_, period):
    """Barriers of one song's DP: one per chunk of ceil(period / 2) frames, one per sweep of 1024 local scores into LDS."""
    if not period:
        return 0
    H, loaded_to, count = (period + 1) // 2, 0, 0
    for t0 in range(0, frames_, H):
        t1 = min(t0 + H, frames_)
        if t1 > loaded_to:
            loaded_to, count = min(t0 + 1024, frames_), count + 1
        count += 1
    return count


out['dp_barriers_per_song'] = [dp_barriers(T, r['period']) for r in found]

# ---- each call alone ----------------------------------------------------------------------------------------------------
d_fb = torch.tensor(bases, dtype=torch.int64).cuda()
d_tf = torch.tensor(frames, dtype=torch.int32).cuda()
bounds = [t // ((int(p[0]) + 1) // 2) + 1 for t in frames]
bbase = np.concatenate([[0], np.cumsum(bounds)]).astype(np.int64)
total = int(bbase[-1])
need = lib.amt_beat_scratch_bytes(songs, pool_frames, int(p[1]), total)
scratch = torch.empty((need,), dtype=torch.uint8, device='cuda')
e_out = torch.zeros((pool_frames,), dtype=torch.int16, device='cuda').view(torch.uint16)
res = torch.zeros((2 * songs + total,), dtype=torch.int32, device='cuda')
prior, pen = torch.from_numpy(p[3]).cuda(), torch.from_numpy(np.ascontiguousarray(p[4])).cuda()
d_bb = torch.from_numpy(bbase[:-1].copy()).cuda()
ea = beat.env_args(mag=mag, ref=refs, frame_base=d_fb, t_frames=d_tf, env=e_out, scratch=scratch, scratch_bytes=need, n=songs,
                   pool_frames=pool_frames, max_frames=max(frames), ldf=ldf, F=F, w=int(p[2]))


def track_args(n):
    return beat.track_args(env=env, frame_base=d_fb, t_frames=d_tf, prior=prior, pen=pen, beat_base=d_bb, period=res[:songs],
                           count=res[songs:2 * songs], beats=res[2 * songs:], scratch=scratch, scratch_bytes=need, n=n,
                           pool_frames=pool_frames, beats_total=total, max_frames=max(frames), lag_lo=int(p[0]),
                           lag_hi=int(p[1]))


ta, ta1 = track_args(songs), track_args(1)
out['envelope'] = rounds(lambda: _lib.check(lib.amt_beat_envelope(ctypes.byref(ea), None)), 20)
out['envelope']['GBps_on_4_B_per_cell'] = 4.0 * songs * T * F / out['envelope']['best_ms'] / 1e6
assert torch.equal(e_out.view(torch.int16), env.view(torch.int16))
out['track'] = rounds(lambda: _lib.check(lib.amt_beat_track(ctypes.byref(ta), None)), 10)
out['track_one_song'] = rounds(lambda: _lib.check(lib.amt_beat_track(ctypes.byref(ta1), None)), 10)
out['track_one_song']['period'] = found[0]['period']
out['track_one_song']['dp_barriers'] = out['dp_barriers_per_song'][0]
out['track_one_song']['us_per_barrier_at_most'] = out['track_one_song']['best_ms'] * 1e3 / max(1, out['dp_barriers_per_song'][0])

# ---- beat.beat_track end to end -----------------------------------------------------------------------------------------
for _ in range(2):
    beat.beat_track(waves, sr, n_fft=N, hop=hop)
e2e = []
for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        beat.beat_track(waves, sr, n_fft=N, hop=hop)
    e2e.append((time.perf_counter() - t0) * 1e3 / 5)
out['beat_track'] = dict(ms=e2e, calls_per_round=5, best_ms=min(e2e), median_ms=sorted(e2e)[2], seconds_of_audio=songs * seconds,
                         audio_seconds_per_second=songs * seconds / min(e2e) * 1e3)

# ---- the reference on the host, one song, fed the device's magnitudes ---------------------------------------------------
import beat_reference as R                                         # noqa: E402
S, ref = mag[bases[0]:bases[0] + frames[0], :F].cpu().numpy(), np.float32(refs[0].item())
t0 = time.perf_counter()
_, e = R.envelope(S, ref, int(p[2]))
t1 = time.perf_counter()
want = R.track(e, int(p[0]), int(p[1]), p[3], p[4])
t2 = time.perf_counter()
out['reference_one_song'] = dict(envelope_ms=(t1 - t0) * 1e3, track_ms=(t2 - t1) * 1e3,
                                 same_envelope=bool(env[bases[0]:bases[0] + frames[0]].cpu().tolist() == e),
                                 same_period_and_beats=bool(want['period'] == found[0]['period'] and
                                                            want['beats'] == found[0]['frames']))
print(json.dumps(out))
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], 'w') as f:
        json.dump(out, f, indent=1)
