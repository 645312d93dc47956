#!/usr/bin/env python3
"""The two measurements of DESIGN 24 (instrument models in the loop), HIP events around device work:

  launch   amt_note_features with all three outputs against the three amt_short_window launches it replaces, at
           B = 1024 windows of 516 frames, N = 2048, a 348 x 8 tile: ROUNDS rounds, the two forms alternating inside a
           round, REPS launches per form and round after a warm-up; median and spread over the rounds.
  step     the step time of a C4-style loop (instrument + pitch heads, three iterations) per instrument model at
           B = 256 windows of 516 frames, against the default model in the same process.

    python scripts/instrument_models_bench.py [launch] [step] [--out FILE.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd')]

ROUNDS, REPS, WARMUP = 7, 100, 20


def _timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3                          # microseconds per call


def launch():
    import torch
    from amt_saga import _lib, audio
    from amt_saga.device import ptr
    lib = _lib.load()
    B, T, N, bands, frames = 1024, 516, 2048, 348, 8
    F, ldf = N // 2 + 1, audio.ldf_of(N)
    g = torch.Generator(device='cuda').manual_seed(1)
    mag = torch.rand((B, T, ldf), device='cuda', generator=g)
    ang = (torch.rand((B, T, ldf), device='cuda', generator=g) - 0.5) * 6.2
    ph = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).contiguous()
    del ang
    rng = np.random.default_rng(2)
    onset = rng.integers(0, T - 40, B)
    src = torch.from_numpy((onset[:, None] + np.arange(frames)[None, :]).astype(np.int32)).cuda()
    pitch_h = rng.integers(21, 109, B).astype(np.int32)
    tone_bin_h = audio.tone_bin_table(44100, N, 21, 108)
    pitch, tone_bin = torch.from_numpy(pitch_h).cuda(), torch.from_numpy(tone_bin_h).cuda()
    lo = torch.from_numpy(tone_bin_h[pitch_h - 21]).cuda()
    ref = torch.rand((B,), device='cuda', generator=g) + 0.5
    outs = [torch.empty((B, bands, frames), device='cuda') for _ in range(6)]

    def fused():
        _lib.check(lib.amt_note_features(ptr(mag), ptr(ph), B, T, F, ldf, T * ldf, ptr(src), frames, ptr(pitch), 60,
                                         ptr(tone_bin), 21, 88, bands, ptr(ref), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                         None))

    def three():
        for mode in range(3):
            _lib.check(lib.amt_short_window(ptr(mag) if mode != 2 else None, ptr(ph) if mode == 2 else None, B, T, F, ldf,
                                            T * ldf, ptr(src), frames, ptr(lo), bands, ptr(ref) if mode == 0 else None,
                                            mode, ptr(outs[3 + mode]), None))
    fused(), three()
    torch.cuda.synchronize()
    same = all(torch.equal(outs[i].view(torch.int32), outs[3 + i].view(torch.int32)) for i in range(3))
    for fn in (fused, three):
        _timed(torch, fn, WARMUP)
    t_f, t_3 = [], []
    for _ in range(ROUNDS):
        t_f.append(_timed(torch, fused, REPS))
        t_3.append(_timed(torch, three, REPS))
    res = dict(shape=dict(B=B, T=T, n_fft=N, bands=bands, frames=frames), rounds=ROUNDS, reps=REPS, bit_identical=same,
               note_features_us=dict(median=float(np.median(t_f)), min=float(min(t_f)), max=float(max(t_f))),
               three_short_window_us=dict(median=float(np.median(t_3)), min=float(min(t_3)), max=float(max(t_3))))
    print(json.dumps(res))
    return res


def step():
    import torch
    from amt_saga import synth
    from amt_saga.device import empty
    from amt_saga.hyperparams import Hyperparams
    from amt_saga.loop import EVENT_FIELDS, INSTRUMENT_MODELS, TranscriptionLoop
    p = Hyperparams(N=2048)
    B, iters, runs = 256, 3, 3
    L = p.H * (p.timing_frames - 1)
    wave, _ = synth.make_windows(B, L, seed=4, notes_per_window=(2, 4), groups=(0, 1, 2), max_onset=0.5 * p.window_size_note_time,
                                 device='cuda')
    out = {}
    for model in INSTRUMENT_MODELS:
        lp = TranscriptionLoop(p, heads=('instrument', 'pitch'), iters=iters, groups=(0, 1, 2),
                               instrument_model=model).setup_device()
        lp.run(wave)                                               # warm-up: every shape of the timed steps
        times = []
        for _ in range(runs):
            b = lp.prepare(wave, refs=lp.refs)
            events = empty((iters, B, len(EVENT_FIELDS)), torch.int32)
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for it in range(iters):
                lp.iterate(b, it, events)
            e.record()
            e.synchronize()
            times.append(a.elapsed_time(e) / iters)
        out[model] = dict(step_ms=float(np.median(times)), min=float(min(times)), max=float(max(times)))
        print(model, json.dumps(out[model]), flush=True)
        del lp
        torch.cuda.empty_cache()
    return dict(shape=dict(B=B, frames=p.timing_frames, n_fft=p.N, heads='instrument+pitch', iters=iters, runs=runs), models=out)


if __name__ == '__main__':
    args = sys.argv[1:]
    path = args[args.index('--out') + 1] if '--out' in args else None
    res = {}
    if 'launch' in args or not (set(args) & {'launch', 'step'}):
        res['launch'] = launch()
    if 'step' in args or not (set(args) & {'launch', 'step'}):
        res['step'] = step()
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(res, f, indent=1)
