"""The device FLAC decoder, measured against the host reader, all from one process.

    python scripts/flac_decode_bench.py [result.json] [kernels_only]

Legs:
  song     a 5-minute mono 24-bit song written by audio.flac_encode: audio.flac_decode wall time (host candidate search,
           upload, kernels, status copy) at verify=True / 'crc' / False; the same song twice in one call; and a
           5-minute two-channel 16-bit stream (mid/side, FIXED 2, Rice2) from the test writer -- the encoder is mono --
           whose frames are twenty written once and repeated (frame numbers are ignored; total and MD5 are the tiled
           signal's).  The host leg is flac.decode on a 10-s excerpt, scaled by length: the reader is a per-sample loop.
  lpc      one 30-s stream of LPC-order-8 Rice2 audio from the test writer (the shape of the reference's files; 10 s of
           frames repeated three times), against the same audio with FIXED order 2: the recurrence is what differs.
  batch    64 songs of 20 .. 40 s in one call, at the three verify levels.
  cli      python -m amt_saga.transcribe --songs over eight 30-s files, --decode host against device, wall time.
With `kernels_only` the host legs and the command line are left out: that form is what a kernel trace is taken of."""
import json
import os
import sys
import tempfile
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
import flac_stream_writer as W
from amt_saga import audio, flac

kernels_only = len(sys.argv) > 2 and sys.argv[2] == 'kernels_only'
sr = 44100
out = {}
gen = torch.Generator(device='cuda').manual_seed(0)


def tone_noise(n, f0, noise=1e-3):
    t = torch.arange(n, device='cuda', dtype=torch.float32)
    y = 0.5 * torch.exp(-(t % 44100.0) / 20000.0) * torch.sin(2 * np.pi * f0 / sr * t)
    return (y + noise * torch.randn(n, device='cuda', generator=gen)).contiguous()


def wall(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        del r
    return ts


def host_tables(datas, verify, reps=3):
    """Seconds of the host's share of a call: STREAMINFO, the candidate search and the tables."""
    t0 = time.perf_counter()
    for _ in range(reps):
        audio._flac_tables(datas, verify)
    return (time.perf_counter() - t0) / reps


def levels(datas, samples):
    res = {}
    for name, v in (('true', True), ('crc', 'crc'), ('false', False)):
        ts = wall(lambda: audio.flac_decode(datas, verify=v))
        res[name] = dict(wall_s=ts, samples_per_s=samples / min(ts))
    res['host_tables_s'] = host_tables(datas, True)
    return res


def tiled(unit, bps, frames, reps):
    """A stream whose frames are those of `unit` (int [n, ch]) written once and repeated `reps` times."""
    data = W.write_stream(unit, bps, frames)
    f0 = W.frames_start(data)
    pcm = np.tile(np.asarray(unit, np.int64).reshape(len(unit), -1), (reps, 1))
    v = int.from_bytes(data[18:26], 'big')
    v = (v >> 36 << 36) | len(pcm)
    return data[:18] + v.to_bytes(8, 'big') + W.pcm_md5(pcm, bps) + data[42:f0] + data[f0:] * reps, len(pcm)


audio.flac_decode(audio.flac_encode([tone_noise(8192, 220.0)], sr))                 # warm-up

# ---- one 5-minute song ---------------------------------------------------------------------------------------------------
n = 300 * sr
song = audio.flac_encode([tone_noise(n, 220.0)], sr)[0]
out['song'] = dict(samples=n, file_bytes=len(song), mono=levels([song], n), two_files=levels([song, song], 2 * n))
unit = W._tone(20 * 4096, 16, 4, ch=2)
stereo, ns = tiled(unit, 16, [(4096, dict(subframes=[W._fx(2, 3, 1), W._fx(2, 3, 1)], assignment=10))] * 20,
                   -(-n // len(unit)))
out['song']['stereo_16bit'] = dict(samples_per_channel=ns, file_bytes=len(stereo), **levels([stereo], 2 * ns))
if not kernels_only:
    m = 10 * sr
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'h.flac')
        audio.save_flac([tone_noise(m, 220.0)], [path], sr)
        t0 = time.perf_counter()
        flac.decode(path)
        host = time.perf_counter() - t0
    out['song']['host_reader'] = dict(excerpt_samples=m, excerpt_s=host, scaled_s_for_the_song=host * n / m,
                                      speedup_verify_true=host * n / m / min(out['song']['mono']['true']['wall_s']),
                                      speedup_verify_crc=host * n / m / min(out['song']['mono']['crc']['wall_s']))

# ---- LPC against FIXED, from the test writer ----------------------------------------------------------------------------------
m = 10 * sr // 4096 * 4096
x = W._tone(m, 16, 3)
c8 = [9000, -4000, 2500, -1500, 900, -500, 300, -100]
frames = lambda sub: [(4096, dict(subframes=[dict(sub)])) for _ in range(m // 4096)]    # noqa: E731
lpc, nl = tiled(x, 16, frames(W._lpc(c8, 15, 13, porder=3, method=1)), 3)
fixed, _ = tiled(x, 16, frames(W._fx(2, 3, 1)), 3)
out['lpc'] = dict(samples=nl, lpc8=levels([lpc], nl), fixed2=levels([fixed], nl),
                  file_bytes=dict(lpc8=len(lpc), fixed2=len(fixed)))

# ---- 64 ragged songs in one call ------------------------------------------------------------------------------------------------
rng = np.random.default_rng(0)
lens = rng.integers(20 * sr, 40 * sr, 64)
files = audio.flac_encode([tone_noise(int(k), 110.0 * 2 ** (i % 36 / 12)) for i, k in enumerate(lens)], sr)
out['batch'] = dict(songs=64, samples=int(lens.sum()), file_bytes=sum(len(f) for f in files),
                    **levels(files, int(lens.sum())))

# ---- the command line -----------------------------------------------------------------------------------------------------------
if not kernels_only:
    import subprocess
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, 'c%d.flac' % i) for i in range(8)]
        audio.save_flac([tone_noise(30 * sr, 110.0 * (i + 1)) for i in range(8)], paths, sr)
        cli = {}
        for mode in ('host', 'device'):
            t0 = time.perf_counter()
            subprocess.run([sys.executable, '-m', 'amt_saga.transcribe', '--songs'] + paths +
                           ['--out-dir', os.path.join(d, mode), '--iters', '1', '--decode', mode], check=True,
                           stdout=subprocess.DEVNULL, env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'amt-saga_amd')))
            cli[mode + '_s'] = time.perf_counter() - t0
        cli['same_midi'] = all(open(os.path.join(d, 'host', 'c%d.mid' % i), 'rb').read() ==
                               open(os.path.join(d, 'device', 'c%d.mid' % i), 'rb').read() for i in range(8))
    out['cli_eight_30s_files'] = cli
print(json.dumps(out))
if len(sys.argv) > 1 and sys.argv[1] != '-':
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(out, f, indent=1)
