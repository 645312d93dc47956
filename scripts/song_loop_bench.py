"""run_songs: steps/s and notes/s for a batch of synthetic songs, against run() iterations on as many windows from the
same process; and the slide kernel alone in GB/s on the bytes it must move, against the same movement composed from
amt_gather_frames (shift + fetch into a second buffer).

    python scripts/song_loop_bench.py [B] [n_fft] [window_seconds] [result.json]

The JSON result is printed; with a fourth argument it is also written to that file.

Compulsory bytes of a slide: per sliding song half x ldf x (4 B magnitude + 8 B phase), read twice, written twice."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd')]
import numpy as np
import torch
from amt_saga import _lib, synth
from amt_saga.audio import gather_frames, ldf_of
from amt_saga.hyperparams import Hyperparams
from amt_saga.loop import SONG_DETECT, SONG_FINISHED, TranscriptionLoop

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
wsec = int(sys.argv[3]) if len(sys.argv) > 3 else 6
p = Hyperparams(N=N, window_size_note_time=wsec)
tf, half, ldf = p.timing_frames, p.timing_frames // 2, ldf_of(N)
lib = _lib.load()
out = {'B': B, 'n_fft': N, 'timing_frames': tf}


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- the slide kernel alone: every song slides, alternating with the composition, same process ----------------------
T_song = 6 * half
dev = 'cuda'
s_mag = torch.rand(B * T_song, ldf, device=dev)
s_ph = torch.rand(B * T_song, ldf, 2, device=dev)
w_mag, w_ph = torch.rand(B, tf, ldf, device=dev), torch.rand(B, tf, ldf, 2, device=dev)
fb = (torch.arange(B, device=dev, dtype=torch.int64) * T_song).contiguous()
ts = torch.full((B,), T_song, dtype=torch.int32, device=dev)
ones = torch.ones(B, dtype=torch.int32, device=dev)
off, cnt, fin = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))


def fused():
    off.zero_()
    _lib.check(lib.amt_song_slide(w_mag.data_ptr(), w_ph.data_ptr(), B, tf, ldf, tf * ldf, s_mag.data_ptr(), s_ph.data_ptr(),
                                  fb.data_ptr(), ts.data_ptr(), ones.data_ptr(), off.data_ptr(), cnt.data_ptr(),
                                  fin.data_ptr(), None))


shift = torch.arange(half, tf, dtype=torch.int32, device=dev)
fetch = torch.arange(tf, tf + half, dtype=torch.int32, device=dev)
S3m, S3p = s_mag.view(B, T_song, ldf), s_ph.view(B, T_song, ldf, 2)


def composed():
    # what the entry points before amt_song_slide offer, in place: two gathers per attribute into fresh halves, then
    # two copies back into the window (the most expensive composition: it moves the bytes twice)
    for w, s, el in ((w_mag, S3m, 1), (w_ph, S3p, 2)):
        a = gather_frames(w, shift, N // 2 + 1, el)
        b = gather_frames(s, fetch, N // 2 + 1, el)
        w[:, :half].copy_(a); w[:, half:].copy_(b)


def composed_pingpong():
    # the cheapest composition: the same two gathers per attribute and NO copy back, as a caller that kept two window
    # buffers and swapped them every slide could do it (the halves land in fresh tensors)
    return [gather_frames(x, idx, N // 2 + 1, el)
            for w, s, el in ((w_mag, S3m, 1), (w_ph, S3p, 2)) for x, idx in ((w, shift), (s, fetch))]


bytes_slide = B * half * ldf * 12 * 4
ms_f, ms_c, ms_p = [], [], []
for _ in range(3):                                                 # alternated; 200 launches = ~0.15-0.3 s per timing
    ms_f.append(timed(fused, 200)); ms_c.append(timed(composed, 200)); ms_p.append(timed(composed_pingpong, 200))
# fused_ms includes the offset reset before and the state-advance launch after the slide kernel
out['slide'] = dict(compulsory_MB=bytes_slide / 1e6, fused_ms=ms_f, composed_ms=ms_c, composed_pingpong_ms=ms_p,
                    fused_GBps=bytes_slide / min(ms_f) / 1e6, composed_GBps=bytes_slide / min(ms_c) / 1e6,
                    composed_pingpong_GBps=bytes_slide / min(ms_p) / 1e6)

# ---- the walk against run() ----------------------------------------------------------------------------------------
heads = ('timing', 'pitch', 'velocity')
lp = TranscriptionLoop(p, heads=heads, iters=4).setup_device()
L = p.H * (tf - 1)
rng = np.random.default_rng(0)
lens = rng.integers(3, 7, B)                                      # 3..6 half windows per song
songs = []
for i in range(B):
    n = int(lens[i]) * half * p.H
    k = -(-n // L)
    w = synth.make_windows(k, L, seed=1000 + i, notes_per_window=(3, 3), max_onset=0.8 * wsec, device='cuda')[0]
    songs.append(w.reshape(-1)[:n].contiguous())
wave = torch.stack([s[:L] if s.numel() >= L else torch.nn.functional.pad(s, (0, L - s.numel())) for s in songs])
lp.run(wave); torch.cuda.synchronize()
run_ms = []
for _ in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    lp.run(wave); torch.cuda.synchronize()
    run_ms.append((time.perf_counter() - t0) * 1e3 / lp.iters)
lp.run_songs(songs[:8], max_notes=4); torch.cuda.synchronize()
walk = []
for _ in range(2):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    st = lp.prepare_songs(songs)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    ev = lp.walk_songs(st, max_notes=4, silence=1e-3, poll=16)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    e = ev.cpu().numpy()
    walk.append(dict(setup_ms=(t1 - t0) * 1e3, walk_ms=(t2 - t1) * 1e3, steps=int(e.shape[0]),
                     ms_per_step=(t2 - t1) * 1e3 / e.shape[0], steps_per_s=e.shape[0] / (t2 - t1),
                     notes=int((e[..., 2] == SONG_DETECT).sum()),
                     notes_per_s=float((e[..., 2] == SONG_DETECT).sum() / (t2 - t1)),
                     idle_slots=float((e[..., 2] == SONG_FINISHED).mean()),
                     sliding_slots=float(((e[..., 2] == 1) | (e[..., 2] == 2)).mean())))
out['run_iteration_ms'] = run_ms
out['walk'] = walk
out['step_over_run_iteration'] = min(w['ms_per_step'] for w in walk) / min(run_ms)
print(json.dumps(out))
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    with open(sys.argv[4], 'w') as f:
        json.dump(out, f, indent=1)
