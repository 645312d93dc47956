"""The device FLAC encoder, measured against the host writer, all from one process.

    python scripts/flac_encode_bench.py [B] [result.json] [host_seconds] [--predictor fixed|lpc|both]

Legs, three repeats each, alternated:
  encode   audio.flac_encode_streams of B signals of 3 .. 6 half windows at N = 2048 (the shape of song_stems_bench.py):
           decaying tones plus noise.  Time per call (all five kernels, MD5 included), samples/s, GB/s on the bytes the
           call has to move (4 B per sample in, the emitted bytes out).  --predictor (default fixed) names the
           predictors of this leg; `both` alternates fixed and lpc calls, the fixed figures under 'encode' as before,
           the others under 'encode_lpc'.  The other legs use the fixed predictors.
  host     flac.save_float on a `host_seconds` excerpt of the same audio (default 10 s), scaled by length to the whole
           set: the writer is a per-sample loop, its time is proportional to the samples.
  ratio    emitted bytes over the VERBATIM size, per signal class of tests/flac_encode_reference.signals().
  song     one 5-minute song with three stems [3, samples] standing for a finished stem_waves result (a tone with
           noise, a sparse stem, a silent one): audio.save_flac against .cpu() + flac.save_float (host leg on the
           excerpt, scaled).
Kernel-by-kernel times (the MD5 kernel on its own) come from a kernel trace of this script with `encode_only` as the
third argument, which runs the encode leg alone."""
import json
import os
import sys
import tempfile
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
import flac_encode_reference as R
from amt_saga import audio, flac
from amt_saga.hyperparams import Hyperparams

predictor = 'fixed'
if '--predictor' in sys.argv:
    at = sys.argv.index('--predictor')
    predictor = sys.argv[at + 1]
    del sys.argv[at:at + 2]
if predictor not in ('fixed', 'lpc', 'both'):
    sys.exit('--predictor: fixed, lpc or both')
legs = ('fixed', 'lpc') if predictor == 'both' else (predictor,)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
encode_only = len(sys.argv) > 3 and sys.argv[3] == 'encode_only'
host_seconds = float(sys.argv[3]) if len(sys.argv) > 3 and not encode_only else 10.0
p = Hyperparams(N=2048, window_size_note_time=6)
half, hop, sr = p.timing_frames // 2, p.H, p.sr
out = {'B': B, 'n_fft': 2048, 'blocksize': 4096, 'bps': 24}
rng = np.random.default_rng(0)
gen = torch.Generator(device='cuda').manual_seed(0)


def tone_noise(n, f0, noise):
    t = torch.arange(n, device='cuda', dtype=torch.float32)
    y = 0.5 * torch.exp(-(t % 44100.0) / 20000.0) * torch.sin(2 * np.pi * f0 / sr * t)
    return (y + noise * torch.randn(n, device='cuda', generator=gen)).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def host_time(y):
    """Seconds flac.save_float takes per second of audio, on the first host_seconds of y."""
    n = min(len(y), int(host_seconds * sr))
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        flac.save_float(y[:n], os.path.join(d, 'h.flac'), sr=sr)
        return (time.perf_counter() - t0) / (n / sr)


# ---- the batch -------------------------------------------------------------------------------------------------------
lens = rng.integers(3, 7, B) * half * hop
songs = [tone_noise(int(n), 110.0 * 2 ** (i % 36 / 12), 1e-3) for i, n in enumerate(lens)]
samples = int(lens.sum())
for leg in legs:
    audio.flac_encode_streams(songs[:4], predictor=leg); torch.cuda.synchronize()
times, emitted, host = {leg: [] for leg in legs}, {}, []
y0 = songs[0].cpu().numpy()
for _ in range(3):
    for leg in legs:
        ms, res = timed(lambda: audio.flac_encode_streams(songs, predictor=leg))
        emitted[leg] = int(res[1][-1])
        times[leg].append(ms)
        del res
    if not encode_only:
        host.append(host_time(y0))
for leg in legs:
    e = emitted[leg]
    out['encode' if leg == legs[0] else 'encode_' + leg] = dict(
        predictor=leg, signals=B, samples=samples, seconds_of_audio=samples / sr, ms=times[leg], emitted_bytes=e,
        ratio_to_verbatim=e / (samples * 3), samples_per_s=samples / (min(times[leg]) * 1e-3),
        GBps=(4 * samples + e) / (min(times[leg]) * 1e-3) / 1e9)
enc = times[legs[0]]
if encode_only:
    print(json.dumps(out))
    sys.exit(0)
out['host'] = dict(excerpt_seconds=host_seconds, s_per_second_of_audio=host,
                   scaled_s_for_the_set=min(host) * samples / sr,
                   device_speedup=min(host) * samples / sr / (min(enc) * 1e-3))

# ---- compression by signal class --------------------------------------------------------------------------------------
sig = R.signals()
dev = [torch.from_numpy(v).cuda() for v in sig.values()]
_, off, _, _, _ = audio.flac_encode_streams(dev)
off = off.cpu().numpy()
out['ratio_by_class'] = {k: float((off[i + 1] - off[i]) / (len(v) * 3)) for i, (k, v) in enumerate(sig.items())}
if 'lpc' in legs:
    off = audio.flac_encode_streams(dev, predictor='lpc')[1].cpu().numpy()
    out['ratio_by_class_lpc'] = {k: float((off[i + 1] - off[i]) / (len(v) * 3)) for i, (k, v) in enumerate(sig.items())}

# ---- one 5-minute song, three stems -------------------------------------------------------------------------------------
n = 300 * sr // hop * hop
stems = torch.stack([tone_noise(n, 220.0, 1e-3),
                     tone_noise(n, 330.0, 0.0) * (torch.arange(n, device='cuda') % (10 * sr) < sr),
                     torch.zeros(n, device='cuda')])
song = {'device_save_flac_s': [], 'host_copy_s': [], 'host_save_float_s_scaled': []}
with tempfile.TemporaryDirectory() as d:
    paths = [os.path.join(d, 'g%d.flac' % g) for g in range(3)]
    audio.save_flac(stems[:, :hop * 64], paths, sr)
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        audio.save_flac(stems, paths, sr)
        song['device_save_flac_s'].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h = stems.cpu().numpy()
        song['host_copy_s'].append(time.perf_counter() - t0)
        song['host_save_float_s_scaled'].append(sum(host_time(h[g]) for g in range(3)) * n / sr)
    song['device_file_bytes'] = [os.path.getsize(q) for q in paths]
song['host_file_bytes'] = 42 + (n // 4096) * (8 + 12289 + 2) + (8 + (8 + (n % 4096) * 24 + 7) // 8 + 2 if n % 4096 else 0)
song['samples_per_stem'] = n
song['speedup'] = (min(song['host_save_float_s_scaled']) + min(song['host_copy_s'])) / min(song['device_save_flac_s'])
out['song'] = song
print(json.dumps(out))
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], 'w') as f:
        json.dump(out, f, indent=1)
