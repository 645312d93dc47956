"""The instrument stems of a song walk, measured: amt_subtract_span_stems against amt_subtract_span on the same windows
and guesses, and the whole walk with and without stems=True, all from one process.

    python scripts/song_stems_bench.py [B] [n_fft] [window_seconds] [result.json]

The JSON result is printed; with a fourth argument it is also written to that file.

Compulsory bytes: the span step reads and writes the residual's guess_frames x ldf floats per window and reads as many of
the guess (3 ldf floats per row); keeping the stems adds one read and one write of the stem's row (5 ldf): the bytes' ratio
is 5 / 3.  Both timings include the frames_max launch that follows the span kernel."""
import ctypes
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd')]
import numpy as np
import torch
from amt_saga import _lib, synth
from amt_saga.audio import ldf_of
from amt_saga.hyperparams import Hyperparams
from amt_saga.loop import SONG_DETECT, TranscriptionLoop

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
wsec = int(sys.argv[3]) if len(sys.argv) > 3 else 6
p = Hyperparams(N=N, window_size_note_time=wsec)
tf, half, ldf, hop, F = p.timing_frames, p.timing_frames // 2, ldf_of(N), p.H, N // 2 + 1
lib = _lib.load()
out = {'B': B, 'n_fft': N, 'timing_frames': tf}
dev = 'cuda'


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- the two span steps on the same inputs, alternated ---------------------------------------------------------------
Tg, G, n_guess = 173, 3, 88                                       # the loop's guess: 173 frames (1 s + the tail)
T_song = 4 * half
resid = torch.rand(B, tf, ldf, device=dev)
guess = torch.rand(n_guess, Tg, ldf, device=dev)                  # (values do not matter to an HBM-bound pass)
fmax = resid[:, :, :F].amax(dim=2).contiguous()
rmax, gmax = fmax.amax(dim=1).contiguous(), guess[:, :, :F].amax(dim=(1, 2)).contiguous()
rng = np.random.default_rng(0)
gidx = torch.from_numpy(rng.integers(0, n_guess, B).astype(np.int32)).cuda()
onset = torch.from_numpy(rng.integers(0, half, B).astype(np.int32)).cuda()
gfr = torch.full((B,), Tg, dtype=torch.int32, device=dev)
new_max = torch.empty(B, device=dev)
stems = torch.zeros(G, B * T_song, ldf, device=dev)
fb = (torch.arange(B, device=dev, dtype=torch.int64) * T_song).contiguous()
off = torch.full((B,), half, dtype=torch.int32, device=dev)
ts = torch.full((B,), T_song, dtype=torch.int32, device=dev)
program = torch.from_numpy(rng.integers(0, p.instrument_classes, B).astype(np.int32)).cuda()
table = torch.from_numpy((synth.prog_group_table(p.instrument_classes) % G).astype(np.int32)).cuda()
a = _lib.SubtractArgs()
a.resid, a.resid_max, a.guess, a.guess_max = resid.data_ptr(), rmax.data_ptr(), guess.data_ptr(), gmax.data_ptr()
a.guess_index, a.guess_frames, a.offset_frames, a.new_max = gidx.data_ptr(), gfr.data_ptr(), onset.data_ptr(), new_max.data_ptr()
a.resid_stride, a.guess_stride = tf * ldf, Tg * ldf
a.B, a.T, a.ldf, a.F = B, tf, ldf, F
a.guess_frames_all, a.normalize, a.relu, a.overkill_factor = 0, 1, 1, 1.0
s = _lib.stem_args(stems=stems, frame_base=fb, offset=off, t_song=ts, program=program, prog_group=table,
                   n_prog=int(table.numel()), G=G, pool_frames=B * T_song)


def span():
    _lib.check(lib.amt_subtract_span(ctypes.byref(a), fmax.data_ptr(), Tg, None))


def span_stems():
    _lib.check(lib.amt_subtract_span_stems(ctypes.byref(a), fmax.data_ptr(), Tg, ctypes.byref(s), None))


ms_p, ms_s = [], []
for _ in range(3):                                                 # alternated; 200 launches per timing
    ms_p.append(timed(span, 200)); ms_s.append(timed(span_stems, 200))
bytes_span, bytes_stems = B * Tg * ldf * 3 * 4, B * Tg * ldf * 5 * 4
out['span'] = dict(span_MB=bytes_span / 1e6, stems_MB=bytes_stems / 1e6, span_ms=ms_p, stems_ms=ms_s,
                   span_GBps=bytes_span / min(ms_p) / 1e6, stems_GBps=bytes_stems / min(ms_s) / 1e6,
                   stems_over_span=[k / q for k, q in zip(ms_s, ms_p)], bytes_ratio=5 / 3)
del resid, guess, stems

# ---- the whole walk with and without the stems ------------------------------------------------------------------------
lp = TranscriptionLoop(p, heads=('timing', 'pitch', 'instrument', 'velocity'), groups=(0, 1, 2), iters=4).setup_device()
L = hop * (tf - 1)
lens = rng.integers(3, 7, B)                                      # 3..6 half windows per song
songs = []
for i in range(B):
    n = int(lens[i]) * half * hop
    k = -(-n // L)
    w = synth.make_windows(k, L, seed=1000 + i, notes_per_window=(3, 3), max_onset=0.8 * wsec, device='cuda')[0]
    songs.append(w.reshape(-1)[:n].contiguous())
lp.run_songs(songs[:8], max_notes=4, stems=True); torch.cuda.synchronize()
walk = {'plain': [], 'stems': []}
events = {}
for _ in range(2):                                                 # alternated
    for name, keep in (('plain', False), ('stems', True)):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        st = lp.prepare_songs(songs, keep_stems=keep)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        ev = lp.walk_songs(st, max_notes=4, silence=1e-3, poll=16)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        if keep:
            waves = st.stem_waves(list(range(B)))
        torch.cuda.synchronize(); t3 = time.perf_counter()
        e = events[name] = ev.cpu().numpy()
        walk[name].append(dict(setup_ms=(t1 - t0) * 1e3, walk_ms=(t2 - t1) * 1e3, stem_waves_ms=(t3 - t2) * 1e3,
                               steps=int(e.shape[0]), ms_per_step=(t2 - t1) * 1e3 / e.shape[0],
                               steps_per_s=e.shape[0] / (t2 - t1), notes=int((e[..., 2] == SONG_DETECT).sum())))
out['walk'] = walk
out['walk_events_identical'] = bool(np.array_equal(events['plain'], events['stems']))
out['walk_stems_over_plain'] = min(w['walk_ms'] for w in walk['stems']) / min(w['walk_ms'] for w in walk['plain'])
out['stem_seconds_of_audio'] = float(sum(int(w.numel()) for w in waves) / p.sr)
print(json.dumps(out))
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    with open(sys.argv[4], 'w') as f:
        json.dump(out, f, indent=1)
