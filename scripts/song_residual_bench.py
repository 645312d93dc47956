"""The residual of a song walk, measured: amt_song_slide_keep against amt_song_slide (every song sliding), one
amt_istft_ragged launch against a loop of single amt_istft calls on the same regions, and the whole walk with and without
residual=True, all from one process.

    python scripts/song_residual_bench.py [B] [n_fft] [window_seconds] [result.json]

The JSON result is printed; with a fourth argument it is also written to that file.

Compulsory bytes: a slide moves half x ldf x (4 B magnitude + 8 B phase) per sliding song, read twice and written twice
(12 ldf floats per row); keeping the outgoing half adds one read and one write of the magnitudes (14 ldf).  The inverse
transform reads T x ldf x 12 B per song and writes hop x (T - 1) x 4 B."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd')]
import numpy as np
import torch
from amt_saga import _lib, synth
from amt_saga.audio import _plan, ldf_of
from amt_saga.hyperparams import Hyperparams
from amt_saga.loop import SONG_DETECT, TranscriptionLoop

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
wsec = int(sys.argv[3]) if len(sys.argv) > 3 else 6
p = Hyperparams(N=N, window_size_note_time=wsec)
tf, half, ldf, hop = p.timing_frames, p.timing_frames // 2, ldf_of(N), p.H
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


# ---- the two slides, every song sliding, alternated -----------------------------------------------------------------
T_song = 6 * half
s_mag = torch.rand(B * T_song, ldf, device=dev)
s_ph = torch.rand(B * T_song, ldf, 2, device=dev)
w_mag, w_ph = torch.rand(B, tf, ldf, device=dev), torch.rand(B, tf, ldf, 2, device=dev)
fb = (torch.arange(B, device=dev, dtype=torch.int64) * T_song).contiguous()
ts = torch.full((B,), T_song, dtype=torch.int32, device=dev)
ones = torch.ones(B, dtype=torch.int32, device=dev)
off, cnt, fin = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))


def slide_with(fn):
    def run():
        off.zero_()
        _lib.check(fn(w_mag.data_ptr(), w_ph.data_ptr(), B, tf, ldf, tf * ldf, s_mag.data_ptr(), s_ph.data_ptr(),
                      fb.data_ptr(), ts.data_ptr(), ones.data_ptr(), off.data_ptr(), cnt.data_ptr(), fin.data_ptr(), None))
    return run


plain, keep = slide_with(lib.amt_song_slide), slide_with(lib.amt_song_slide_keep)
ms_s, ms_k = [], []
for _ in range(3):                                                 # alternated; 200 launches per timing
    ms_s.append(timed(plain, 200)); ms_k.append(timed(keep, 200))
bytes_slide, bytes_keep = B * half * ldf * 12 * 4, B * half * ldf * 14 * 4
# (both timings include the offset reset before and the state-advance launch after the kernel)
out['slide'] = dict(slide_MB=bytes_slide / 1e6, keep_MB=bytes_keep / 1e6, slide_ms=ms_s, keep_ms=ms_k,
                    slide_GBps=bytes_slide / min(ms_s) / 1e6, keep_GBps=bytes_keep / min(ms_k) / 1e6,
                    keep_over_slide=[k / s for k, s in zip(ms_k, ms_s)], bytes_ratio=14 / 12)
del w_mag, w_ph

# ---- one ragged inverse transform against a loop of single calls ----------------------------------------------------
rng = np.random.default_rng(0)
lens = rng.integers(3, 7, B)                                      # 3..6 half windows per song
frames = [int(k) * half + 1 for k in lens]
base = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
o_len = [hop * (t - 1) for t in frames]
o_base = np.concatenate([[0], np.cumsum(o_len)]).astype(np.int64)
plan = _plan(N, hop, True)
pool = int(base[-1])
mag, ph = s_mag[:pool], s_ph[:pool]
y_r = torch.zeros(int(o_base[-1]), device=dev)
y_l = torch.zeros(int(o_base[-1]), device=dev)
d_fb, d_ob = torch.from_numpy(base[:-1].copy()).cuda(), torch.from_numpy(o_base[:-1].copy()).cuda()
d_t = torch.from_numpy(np.asarray(frames, np.int32)).cuda()


def ragged():
    _lib.check(lib.amt_istft_ragged(plan, mag.data_ptr(), ph.data_ptr(), d_fb.data_ptr(), d_t.data_ptr(), B, max(frames),
                                    pool, ldf, y_r.data_ptr(), d_ob.data_ptr(), y_r.numel(), None))


def loop_of_singles():
    for i in range(B):
        f0, t = int(base[i]), frames[i]
        _lib.check(lib.amt_istft(plan, mag.data_ptr() + f0 * ldf * 4, ph.data_ptr() + f0 * ldf * 8, 1, t, ldf, t * ldf,
                                 y_l.data_ptr() + int(o_base[i]) * 4, o_len[i], None))


ms_r, ms_l = [], []
for _ in range(3):
    ms_r.append(timed(ragged, 20)); ms_l.append(timed(loop_of_singles, 20))
bytes_istft = sum(t * ldf * 12 + n * 4 for t, n in zip(frames, o_len))
out['istft'] = dict(songs=B, frames=int(sum(frames)), compulsory_MB=bytes_istft / 1e6, ragged_ms=ms_r, loop_ms=ms_l,
                    ragged_GBps=bytes_istft / min(ms_r) / 1e6, loop_GBps=bytes_istft / min(ms_l) / 1e6,
                    loop_over_ragged=min(ms_l) / min(ms_r), bit_identical=bool(torch.equal(y_r, y_l)))
del s_mag, s_ph, mag, ph, y_r, y_l

# ---- the whole walk with and without the residual ---------------------------------------------------------------------
lp = TranscriptionLoop(p, heads=('timing', 'pitch', 'velocity'), iters=4).setup_device()
L = hop * (tf - 1)
songs = []
for i in range(B):
    n = int(lens[i]) * half * hop
    k = -(-n // L)
    w = synth.make_windows(k, L, seed=1000 + i, notes_per_window=(3, 3), max_onset=0.8 * wsec, device='cuda')[0]
    songs.append(w.reshape(-1)[:n].contiguous())
lp.run_songs(songs[:8], max_notes=4, residual=True); torch.cuda.synchronize()
walk = {'plain': [], 'residual': []}
events = {}
for _ in range(2):                                                 # alternated
    for name, res in (('plain', False), ('residual', True)):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        st = lp.prepare_songs(songs, keep_residual=res)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        ev = lp.walk_songs(st, max_notes=4, silence=1e-3, poll=16)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        if res:
            waves = st.residual_waves(list(range(B)))
        torch.cuda.synchronize(); t3 = time.perf_counter()
        e = events[name] = ev.cpu().numpy()
        walk[name].append(dict(setup_ms=(t1 - t0) * 1e3, walk_ms=(t2 - t1) * 1e3, residual_waves_ms=(t3 - t2) * 1e3,
                               steps=int(e.shape[0]), ms_per_step=(t2 - t1) * 1e3 / e.shape[0],
                               notes=int((e[..., 2] == SONG_DETECT).sum())))
out['walk'] = walk
out['walk_events_identical'] = bool(np.array_equal(events['plain'], events['residual']))
out['walk_residual_over_plain'] = min(w['walk_ms'] for w in walk['residual']) / min(w['walk_ms'] for w in walk['plain'])
out['residual_seconds_of_audio'] = float(sum(int(w.numel()) for w in waves) / p.sr)
print(json.dumps(out))
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    with open(sys.argv[4], 'w') as f:
        json.dump(out, f, indent=1)
