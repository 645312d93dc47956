"""The device WAV unpack and pack, measured next to the host numpy reader, all from one process.

    python scripts/wav_bench.py [result.json]          (default: profiles/wav_bench.json)

Legs:
  song16 / song24   a 5-minute stereo 16-bit / 24-bit file from the test writer: audio.wav_decode wall time (header walk,
                    upload, kernel), the unpack kernel alone between events, and wav.decode + to_wave on the host.
  batch             64 mono 24-bit files of 20 .. 40 s in one call, the same three figures.
  pack              the 64 signals (and one 5-minute signal) through audio.wav_encode for the three formats, with and
                    without norm: wall time (kernels, copy back, file assembly) and the pack kernel alone.
GB/s are on ideal bytes: file data + 4 per value for unpack, 4 + container bytes per sample for pack.  Information, not a
bar: the kernels are plain streaming."""
import ctypes as C
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'amt-saga_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
import wav_stream_writer as W
from amt_saga import _lib, audio, wav
from amt_saga.device import ptr, stream_ptr

sr = 44100
out = {}
lib = _lib.load()
rng = np.random.default_rng(0)


def wall(fn, reps=5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        del r
    return ts


def events(fn, reps=20, warm=3):
    """Seconds of each of `reps` enqueued calls, between events on the current stream."""
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e-3 for a, b in ev]


def unpack_leg(datas):
    infos, sm, out_values = audio._wav_tables(datas)
    values = sum(f * ch for _, ch, _, _, f in infos)
    data_bytes = sum(int(r[1] * r[2] * r[4]) for r in sm)
    ideal = data_bytes + 4 * values
    blob = torch.frombuffer(bytearray(b''.join(datas)), dtype=torch.uint8).cuda()
    sm_d = torch.from_numpy(sm).cuda()
    o = torch.empty((out_values,), dtype=torch.float32, device='cuda')
    mf = max(f for _, _, _, _, f in infos)
    ker = events(lambda: _lib.check(lib.amt_pcm_unpack_ragged(ptr(blob), blob.numel(), ptr(sm_d), len(infos), mf, ptr(o),
                                                              None, out_values, stream_ptr())))
    w = wall(lambda: audio.wav_decode(datas))
    t0 = time.perf_counter()
    for d in datas:
        x, _, bits = wav.decode(d)
        wav.to_wave(x, 'int', bits)
    host = time.perf_counter() - t0
    med = float(np.median(ker))
    return dict(files=len(datas), values=values, ideal_bytes=ideal, kernel_s=ker, kernel_median_s=med,
                kernel_GBps=ideal / med / 1e9, wav_decode_wall_s=w, wav_decode_GBps=ideal / min(w) / 1e9,
                host_numpy_s=host, host_numpy_GBps=ideal / host / 1e9)


def pack_leg(sigs):
    anchor, base, lens = audio._ragged_layout(sigs)
    res = {}
    for fmt in wav.FORMATS:
        c = wav.FORMAT_BYTES[fmt]
        ideal = (4 + c) * sum(lens)
        ob = np.concatenate([[0], np.cumsum([-(-l * c // 4) * 4 for l in lens])])
        meta = torch.tensor([base, lens, ob[:-1].tolist()], dtype=torch.int64).cuda()
        o = torch.empty((int(ob[-1]),), dtype=torch.uint8, device='cuda')
        peaks = torch.empty((len(sigs),), dtype=torch.float32, device='cuda')
        ker = events(lambda: _lib.check(lib.amt_pcm_pack_ragged(C.c_void_p(anchor), ptr(meta[0]), ptr(meta[1]), len(sigs),
                                                                max(lens), audio.PCM_FORMATS[fmt], None, ptr(o),
                                                                ptr(meta[2]), o.numel(), stream_ptr())))
        pk = events(lambda: _lib.check(lib.amt_pcm_peak_ragged(C.c_void_p(anchor), ptr(meta[0]), ptr(meta[1]), len(sigs),
                                                               max(lens), ptr(peaks), stream_ptr())))
        med = float(np.median(ker))
        res[fmt] = dict(ideal_bytes=ideal, kernel_median_s=med, kernel_GBps=ideal / med / 1e9,
                        peak_kernel_median_s=float(np.median(pk)), peak_GBps=4 * sum(lens) / float(np.median(pk)) / 1e9,
                        wav_encode_wall_s=wall(lambda: audio.wav_encode(sigs, sr, fmt=fmt), reps=3),
                        wav_encode_norm_wall_s=wall(lambda: audio.wav_encode(sigs, sr, fmt=fmt, norm=True), reps=3))
    return dict(signals=len(sigs), samples=sum(lens), **res)


audio.wav_decode([W.write(np.arange(64), c=2)])                                   # warm-up
n = 300 * sr
for name, c in (('song16', 2), ('song24', 3)):
    b = 8 * c
    x = rng.integers(-(1 << (b - 1)), 1 << (b - 1), (n, 2), dtype=np.int64)
    out[name] = unpack_leg([W.write(x, c=c, sr=sr, before=[(b'LIST', b'abc')])])
    del x
lens = rng.integers(20 * sr, 40 * sr, 64)
files = [W.write(rng.integers(-(1 << 23), 1 << 23, int(k), dtype=np.int64), c=3, sr=sr) for k in lens]
out['batch'] = unpack_leg(files)
sigs = [w for w, _, _ in audio.wav_decode(files)]
out['pack_batch'] = pack_leg(sigs)
out['pack_song'] = pack_leg([torch.rand(n, device='cuda') * 2 - 1])
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'wav_bench.json')
if path != '-':
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
