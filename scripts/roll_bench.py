"""The piano-roll stages, measured, all from one process.

    python scripts/roll_bench.py [B] [result.json]

Two workloads at 1200 x 440 (pitches 21..108, five rows a pitch, a tick every second):
  songs        B (default 256) lists of 3000 notes over 180 s -- onsets uniform, durations 50 ms .. 2 s, pitches and
               programs uniform -- each drawn alone (single mode); and the same lists against a jittered copy (pair mode).
  adversarial  ONE list: a note that lasts the whole 200 s span under 200 000 one-millisecond notes of the same pitch.
Legs, five repeats each after a warm-up, alternated, the median reported (and every repeat of the two host-clock legs):
  draw         the ONE amt_roll_draw launch alone, by device events (lists packed and uploaded before): ms, GB/s on the
               pixels written.
  call         roll.piano_rolls from packed lists to finished device images (checks, uploads, launch), by the host clock.
  png          roll.piano_roll_png from packed lists to the finished files on the host, by the host clock; the bytes.
  host         for context, NOT the code under test: a numpy painter on the host that fills one slice per note (on
               `host_lists` of the lists, scaled), without onsets, ticks or the drawn-note rule."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from amt_saga import roll, score

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
W, PX, PITCH, NOTES, SECONDS = 1200, 5, (21, 108), 3000, 180.0
H = (PITCH[1] - PITCH[0] + 1) * PX
host_lists = min(B, 16)
rng = np.random.default_rng(0)


def song():
    """(pitch, program, on, off) arrays as score.pack returns them, made directly in microseconds."""
    pitch = rng.integers(PITCH[0], PITCH[1] + 1, NOTES)
    program = rng.integers(0, 128, NOTES)
    on = rng.integers(0, int(SECONDS * 1e6), NOTES)
    off = on + rng.integers(50000, 2000000, NOTES)
    order = np.lexsort((program, off, on, pitch))
    return (pitch[order].astype(np.int32), program[order].astype(np.int32), on[order].astype(np.int64), off[order].astype(np.int64))


def jitter(p):
    on = p[2] + rng.integers(-30000, 30000, len(p[2]))
    off = p[3] + rng.integers(-30000, 30000, len(p[2]))
    order = np.lexsort((p[1], off, on, p[0]))
    return (p[0][order], p[1][order], on[order], off[order])


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


def paint(p, span_us):
    """The host painter: one slice per note, the group colour, nothing else."""
    img = np.zeros((H, W), np.uint8)
    x0 = np.clip(p[2] * W // span_us, 0, W)
    x1 = np.clip(-(-np.maximum(p[3], p[2] + 1) * W // span_us), 0, W)
    for pitch, program, a, b in zip(p[0].tolist(), p[1].tolist(), x0.tolist(), x1.tolist()):
        r = (PITCH[1] - pitch) * PX
        img[r:r + PX, a:b] = 16 + 2 * (program % 16)
    return img


def med(v):
    return float(sorted(v)[len(v) // 2])


def measure(est, gold, span, n_host):
    kw = dict(width=W, row_px=PX, pitch=PITCH, span=span, tick=1.0)
    n, pixels = len(est), len(est) * W * H
    call = roll.prepare(est, gold, **kw)
    call()
    roll.piano_roll_png(est, gold, **kw)                               # (warm-up of every shape)
    t_draw, t_call, t_png = [], [], []
    for _ in range(5):
        t_draw.append(timed(call)[0])
        ms, files = wall(lambda: roll.piano_roll_png(est, gold, **kw))
        t_png.append(ms)
        t_call.append(wall(lambda: roll.piano_rolls(est, gold, **kw))[0])
    t0 = time.perf_counter()
    for p in est[:n_host]:
        paint(p, int(span[1] * 1e6))
    host_ms = 1e3 * (time.perf_counter() - t0) * n / n_host
    return dict(images=n, notes=int(sum(len(p[0]) for p in est)), pair=gold is not None,
                draw_ms=med(t_draw), draw_GBps_pixels=pixels / med(t_draw) / 1e6, call_ms=med(t_call), png_ms=med(t_png),
                call_ms_all=t_call, png_ms_all=t_png,
                png_bytes=int(sum(len(f) for f in files)), pixel_bytes=pixels, host_numpy_painter_ms=host_ms,
                host_lists_measured=n_host)


songs = [song() for _ in range(B)]
out = {'size': [W, H], 'device': torch.cuda.get_device_name(0)}
out['songs_single'] = measure(songs, None, (0.0, SECONDS), host_lists)
out['songs_pair'] = measure(songs, [jitter(p) for p in songs], (0.0, SECONDS), host_lists)
short_on = 1000 * np.arange(200000, dtype=np.int64)
adv = (np.full(200001, 60, np.int32), np.concatenate([[1], np.full(200000, 2)]).astype(np.int32),
       np.concatenate([[-10], short_on]), np.concatenate([[200000000], short_on + 1000]))
order = np.lexsort((adv[1], adv[3], adv[2], adv[0]))
adv = tuple(a[order] for a in adv)
out['adversarial'] = measure([adv], None, (0.0, 200.0), 1)
# the kernel's image of the adversarial list is the rule's
import roll_reference as R
notes = list(zip(adv[0].tolist(), adv[1].tolist(), adv[2].tolist(), adv[3].tolist()))
want = R.draw(R.case('adversarial', notes, None, W=W, row_px=PX, lo=PITCH[0], hi=PITCH[1], t0=0, t1=200000000, tick=1000000))
got = roll.piano_rolls([adv], None, width=W, row_px=PX, pitch=PITCH, span=(0.0, 200.0), tick=1.0)[0].cpu().numpy()
assert np.array_equal(got, want), 'the device image is not the rule\'s'
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        json.dump(out, f, indent=1)
