"""Harmonic/percussive separation, measured: one amt_hpss_ragged launch over `songs` songs of five minutes at n_fft 2048
(25 840 frames of 1 025 bins each); audio.hpss end to end on the same number of five-minute waveforms; and, for scale,
scipy.ndimage.median_filter on one song on the host.  Five rounds of each, every round about half a second of device
work, after a warm-up at the timed shape.

    python scripts/hpss_bench.py [songs] [kernel] [result.json]

The JSON result is printed; with a third argument it is also written to that file.  Compulsory bytes: 12 per cell (S read
once, Sh and Sp written)."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd')]
import ctypes
import numpy as np
import torch
from amt_saga import _lib, audio

songs = int(sys.argv[1]) if len(sys.argv) > 1 else 16
k = int(sys.argv[2]) if len(sys.argv) > 2 else 31
N, hop, sr, seconds = 2048, 512, 44100, 300
F, ldf = N // 2 + 1, audio.ldf_of(N)
n_samples = seconds * sr
T = 1 + n_samples // hop
lib = _lib.load()
out = dict(songs=songs, n_fft=N, frames_per_song=T, bins=F, kernel=[k, k], power=2.0, margin=[1.0, 1.0],
           device=torch.cuda.get_device_name(0))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- the launch alone ---------------------------------------------------------------------------------------------------
gen = torch.Generator(device='cuda').manual_seed(0)
pool = torch.rand(songs * T, ldf, device='cuda', generator=gen)
pool[:, F:] = 5.0
res = [torch.empty_like(pool), torch.empty_like(pool)]
d_fb = (torch.arange(songs, device='cuda', dtype=torch.int64) * T).contiguous()
d_tf = torch.full((songs,), T, dtype=torch.int32, device='cuda')


def launch():
    a = audio.hpss_args(mag=pool, out_h=res[0], out_p=res[1], frame_base=d_fb, t_frames=d_tf, n=songs,
                        pool_frames=songs * T, max_frames=T, ldf=ldf, F=F, kt=k, kf=k, power=2.0, margin_h=1.0,
                        margin_p=1.0)
    _lib.check(lib.amt_hpss_ragged(ctypes.byref(a), None))


cells = songs * T * F
for _ in range(3):                                                 # warm up at the timed shape
    launch()
torch.cuda.synchronize()
ms = [timed(launch, 40) for _ in range(5)]
best = min(ms)
out['launch'] = dict(ms=ms, repetitions_per_round=40, best_ms=best, median_ms=sorted(ms)[2], cells_per_s=cells / best * 1e3,
                     GBps_on_12_B_per_cell=12 * cells / best / 1e6)
out['cells'] = cells
one_song = pool[:T, :F].cpu().numpy()
check = dict(h=res[0][:T, :F].cpu().numpy(), p=res[1][:T, :F].cpu().numpy())
del pool, res
torch.cuda.empty_cache()

# ---- audio.hpss end to end ----------------------------------------------------------------------------------------------
waves = [torch.rand(n_samples, device='cuda', generator=gen) * 2 - 1 for _ in range(songs)]
for _ in range(2):                                                 # warm up at the timed shape
    audio.hpss(waves, n_fft=N, hop=hop, kernel=(k, k))
torch.cuda.synchronize()
e2e = []
for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        parts = audio.hpss(waves, n_fft=N, hop=hop, kernel=(k, k))
        del parts
    torch.cuda.synchronize()
    e2e.append((time.perf_counter() - t0) * 1e3 / 20)
out['audio_hpss'] = dict(ms=e2e, calls_per_round=20, best_ms=min(e2e), median_ms=sorted(e2e)[2], seconds_of_audio=songs * seconds,
                         audio_seconds_per_second=songs * seconds / min(e2e) * 1e3)
del waves

# ---- scipy on the host, one song, for scale -----------------------------------------------------------------------------
try:
    from scipy import ndimage
    t0 = time.perf_counter()
    Ht = ndimage.median_filter(one_song, size=(k, 1), mode='reflect')
    Pf = ndimage.median_filter(one_song, size=(1, k), mode='reflect')
    host_ms = (time.perf_counter() - t0) * 1e3
    Z = np.maximum(Ht, Pf)
    a, b = Ht / Z, Pf / Z
    a, b = a * a, b * b
    mh, mp = a / (a + b), b / (a + b)
    out['scipy_median_filter_one_song'] = dict(ms=host_ms, cells_per_s=T * F / host_ms * 1e3,
                                               same_components=bool(np.array_equal(one_song * mh, check['h']) and
                                                                    np.array_equal(one_song * mp, check['p'])))
except ImportError:
    out['scipy_median_filter_one_song'] = 'not measured: scipy is not installed'
print(json.dumps(out))
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
    with open(sys.argv[3], 'w') as f:
        json.dump(out, f, indent=1)
