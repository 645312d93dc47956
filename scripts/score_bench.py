#!/usr/bin/env python3
"""score_pairs on a collection against the Python restatement of the rule on the host.

    python scripts/score_bench.py [--pairs 256] [--notes 4000] [--repeats 20] [--host-pairs 256] [--out FILE.json]

A pair: `notes` gold notes over five minutes on pitches 36 .. 96, and a transcription of them -- onsets and offsets
jittered (some beyond the tolerances), a tenth of the notes missed, a tenth invented, a fifth with another program.  Times
one whole score_pairs call (pack on the host, upload, the kernel, the counts back), the kernel alone on packed device
arrays (events), and tests/score_reference.py on the first --host-pairs pairs; the counts of the two must be equal."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'amt-saga_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def make_pair(rng, notes):
    on = np.sort(rng.integers(0, 300_000_000, notes))
    ref = [(int(rng.integers(36, 97)), int(rng.choice((0, 24, 40, 48))), int(t), int(t + rng.integers(100_000, 1_000_000)))
           for t in on]
    est = []
    for p, g, a, b in ref:
        if rng.random() < 0.1:
            continue
        est.append((p, g if rng.random() < 0.8 else 24, a + int(rng.integers(-60_000, 60_001)),
                    b + int(rng.integers(-150_000, 150_001))))
    for _ in range(notes // 10):
        t = int(rng.integers(0, 300_000_000))
        est.append((int(rng.integers(36, 97)), 0, t, t + int(rng.integers(100_000, 1_000_000))))
    return est, ref


def as_dicts(notes):
    return [dict(pitch=p, program=g, start=a / 1e6, end=b / 1e6) for p, g, a, b in notes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=256)
    ap.add_argument('--notes', type=int, default=4000)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--host-pairs', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import score_reference as R
    from amt_saga import score
    rng = np.random.default_rng(27)
    pairs = [make_pair(rng, a.notes) for _ in range(a.pairs)]
    est = [score.pack(as_dicts(e)) for e, _ in pairs]
    ref = [score.pack(as_dicts(r)) for _, r in pairs]
    group = np.asarray(R.MERGED, np.int32)
    total = sum(len(e[0]) for e in est) + sum(len(r[0]) for r in ref)

    def once():
        torch.cuda.synchronize()
        t = time.perf_counter()
        got = score.score_pairs(est, ref, group=group)
        return time.perf_counter() - t, got
    for _ in range(3):                                                  # warm-up: the library, the allocator, the clocks
        _, counts = once()
    calls = sorted(once()[0] for _ in range(a.repeats))

    # the kernel alone: the call's own steps, taken apart
    from amt_saga import _lib
    from amt_saga.device import stream_ptr
    import ctypes
    lib = _lib.load()
    e_side, r_side = score._side(est), score._side(ref)
    dev = [[torch.from_numpy(x).cuda() for x in s] for s in (e_side, r_side)]
    need = int(lib.amt_score_scratch_bytes(int(e_side[4][-1]), int(r_side[4][-1])))
    scratch = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.empty((a.pairs, 10), dtype=torch.int64, device='cuda')
    g = torch.from_numpy(group).cuda()
    args = score.score_args(est_pitch=dev[0][0], est_program=dev[0][1], est_on=dev[0][2], est_off=dev[0][3],
                            ref_pitch=dev[1][0], ref_program=dev[1][1], ref_on=dev[1][2], ref_off=dev[1][3],
                            est_offsets_host=e_side[4].ctypes.data, ref_offsets_host=r_side[4].ctypes.data,
                            est_offsets=dev[0][4], ref_offsets=dev[1][4], group=g, scratch=scratch, scratch_bytes=need,
                            out=out, n_pairs=a.pairs)
    kernel = []
    for k in range(3 + a.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _lib.check(lib.amt_score_pairs(ctypes.byref(args), stream_ptr()))
        t1.record()
        torch.cuda.synchronize()
        if k >= 3:
            kernel.append(t0.elapsed_time(t1) * 1e-3)
    kernel.sort()
    assert np.array_equal(out.cpu().numpy(), counts)

    n_host = min(a.host_pairs, a.pairs)
    t = time.perf_counter()
    want = [R.score(e, r, group=R.MERGED) for e, r in pairs[:n_host]]
    host = time.perf_counter() - t
    assert counts[:n_host].tolist() == want, 'the kernel and the reference disagree'
    micro = score.summary(counts)['micro']
    res = dict(pairs=a.pairs, notes_per_side=a.notes, notes_total=total, scratch_bytes=need, repeats=a.repeats,
               call_s=dict(median=calls[len(calls) // 2], min=calls[0], max=calls[-1]),
               kernel_s=dict(median=kernel[len(kernel) // 2], min=kernel[0], max=kernel[-1]),
               host_reference_s=host, host_pairs=n_host, host_reference_s_scaled=host * a.pairs / max(1, n_host),
               f_onset=micro['onset']['f'], f_onset_offset=micro['onset_offset']['f'], f_frame=micro['frame']['f'])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
