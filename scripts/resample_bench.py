"""Resampler kernel rate (amt_resample_ragged through audio.Resampler): one 5-minute stereo song at 48 kHz and at 96 kHz
to 44.1 kHz, and a batch of 64 ragged mono songs (2 to 6 minutes, 48 kHz) in one launch.  GB/s on the ideal bytes
4 * (n_in * channels + n_out): every input float read once, every output float written once."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd')]
import numpy as np
import torch
from amt_saga.audio import Resampler


def run(name, rs, signals, channels, reps=5):
    n_in = sum(s.shape[0] for s in signals)
    n_out = sum(rs.out_len(s.shape[0]) for s in signals)
    out = torch.empty(n_out, device='cuda')
    arg = signals if len(signals) > 1 else signals[0]
    for _ in range(2): rs(arg, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): rs(arg, out=out)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    byt = 4 * (n_in * channels + n_out)
    print('%-28s L/M %d/%d taps %3d  %d signal(s) %9d in x %d ch -> %9d out  %.3f ms  %.1f GB/s ideal  %.1f Gtap/s'
          % (name, rs.L, rs.M, rs.taps, len(signals), n_in, channels, n_out, ms, byt / ms / 1e6,
             n_out * (2 * (rs.Z * max(rs.L, rs.M) // rs.L) + 2) / ms / 1e6))


for sr in (48000, 96000):
    rs = Resampler(sr, 44100)
    run('5 min stereo %d' % sr, rs, [torch.randn(300 * sr, 2, device='cuda') * 0.1], 2)
    run('5 min mono %d' % sr, rs, [torch.randn(300 * sr, device='cuda') * 0.1], 1)
lens = np.random.default_rng(0).integers(120 * 48000, 360 * 48000, 64)
# (a list is packed with one torch.cat per call: the time of the batch includes that copy)
run('64 ragged songs 48000', Resampler(48000, 44100), [torch.randn(int(n), device='cuda') * 0.1 for n in lens], 1)
