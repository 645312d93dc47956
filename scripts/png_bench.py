"""The spectrogram-image stages, measured against the host route, all from one process.

    python scripts/png_bench.py [B] [result.json]

B (default 256) images of 1200 x 500 from synthetic spectra: [T, ldf] magnitudes at N = 2048 (T = 2000 frames), decaying
harmonic partials over a noise floor, so that the level images have the runs and the texture of a real spectrogram.
Legs, three repeats each, alternated after a warm-up of every shape:
  levels   audio.spectrogram_levels (one amt_spec_levels_ragged launch): ms, GB/s on the pixels written, GB/s on the
           magnitudes read.
  encode   audio.png_encode up to the finished bytes on the host (the table upload, three kernels, the copy of the
           sizes, the copy of the files): ms by the host clock, GB/s on the pixels; and audio.png_encode_streams, the
           same call without the two copies back, by device events.
  host     the route the stage replaces: the level images copied back (.cpu()), then per image zlib.compress of the
           unfiltered scanlines at level 1 and at level 6 (on `host_images` of them, scaled): ms, and the bytes.
  sizes    summed PNG bytes of the device files against both zlib results and the raw pixels."""
import json
import os
import sys
import time
import zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from amt_saga import audio, png
from amt_saga.audio import ldf_of

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
W, H, N, T, SR = 1200, 500, 2048, 2000, 44100
F, ldf = N // 2 + 1, ldf_of(N)
host_images = min(B, 16)
gen = torch.Generator(device='cuda').manual_seed(0)


def spectrum(i):
    """[T, ldf] float32: a note every 40 frames, eight partials each, decaying; a noise floor 70 dB below."""
    t = torch.arange(T, device='cuda', dtype=torch.float32)[:, None]
    f = torch.arange(ldf, device='cuda', dtype=torch.float32)[None, :]
    onset = (t // 40) * 40
    f0 = 8.0 + ((onset / 40 + i) * 7 % 48)
    mag = torch.zeros((T, ldf), device='cuda')
    for h in range(1, 9):
        mag += torch.exp(-0.5 * ((f - f0 * h) / 1.2) ** 2) * torch.exp(-(t - onset) / 25.0) / h
    return (mag + 3e-4 * torch.rand((T, ldf), device='cuda', generator=gen)).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


mags = [spectrum(i) for i in range(B)]
refs = torch.stack([m.max() for m in mags])
kw = dict(size=(W, H), axis='log', sr=SR, n_fft=N)
images = audio.spectrogram_levels(mags, refs, **kw)
files = audio.png_encode(images)
torch.cuda.synchronize()
pixels = B * W * H
t_levels, t_encode, t_kernels, t_copy = [], [], [], []
for _ in range(3):
    ms, images = timed(lambda: audio.spectrogram_levels(mags, refs, **kw))
    t_levels.append(ms)
    ms, files = wall(lambda: audio.png_encode(images))
    t_encode.append(ms)
    ms, _ = timed(lambda: audio.png_encode_streams(images))
    t_kernels.append(ms)
    ms, host = wall(lambda: [im.cpu().numpy() for im in images[:host_images]])
    t_copy.append(ms * B / host_images)
z = {}
for level in (1, 6):
    t0 = time.perf_counter()
    sizes = [len(zlib.compress(b''.join(b'\0' + row.tobytes() for row in im), level)) for im in host]
    z[level] = dict(ms=1e3 * (time.perf_counter() - t0) * B / host_images, bytes=int(sum(sizes) * B / host_images))
med = lambda v: float(sorted(v)[len(v) // 2])
import png_reference as R
assert files[0] == R.encode(images[0].cpu().numpy(), png.palette('cubehelix')), 'the device file is not the rule\'s'
out = {
    'B': B, 'size': [W, H], 'frames': T, 'n_fft': N,
    'levels_ms': med(t_levels), 'levels_GBps_pixels': pixels / med(t_levels) / 1e6,
    'levels_GBps_magnitudes_read': B * T * F * 4 / med(t_levels) / 1e6,
    'encode_ms_with_copies': med(t_encode), 'encode_GBps_pixels': pixels / med(t_encode) / 1e6,
    'encode_ms_device_only': med(t_kernels), 'encode_device_only_GBps_pixels': pixels / med(t_kernels) / 1e6,
    'png_bytes': int(sum(len(f) for f in files)), 'pixel_bytes': pixels,
    'host_copy_back_ms': med(t_copy), 'host_zlib1_ms': z[1]['ms'], 'host_zlib1_bytes': z[1]['bytes'],
    'host_zlib6_ms': z[6]['ms'], 'host_zlib6_bytes': z[6]['bytes'], 'host_images_measured': host_images,
    'device': torch.cuda.get_device_name(0),
}
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        json.dump(out, f, indent=1)
