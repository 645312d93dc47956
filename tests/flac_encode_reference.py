"""numpy restatement of the device FLAC encoder's format rule, independent of the product's encoder:
nothing of amt_saga is imported.  Every step is integer, so the bytes are defined and the device's are compared for
equality.

    quantise(y, bps)                          float32 -> int64, round half to even, clip, NaN -> 0
    encode_frame(q, bps, number)              -> (bytes, (kind, o, p, [k_j]))
    encode_frames(y or q, ...)                -> ([frame bytes], [choices])
    encode_file(y, sr, bps, blocksize)        -> a complete file: fLaC, STREAMINFO, frames
"""
import hashlib

import numpy as np

K_MAX = 30                          # Rice2 parameters 0 .. 30; 31 is the escape code, never used
P_MAX = 8


def quantise(y, bps):
    y = np.asarray(y, dtype=np.float32)
    lim = 1 << (bps - 1)
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.rint(y * np.float32(lim))                      # float32 product: exact (a power of two), then half-even
    r = np.where(np.isnan(r), np.float32(0), r)
    return np.clip(r.astype(np.float64), -lim, lim - 1).astype(np.int64)


def utf8_num(v):
    """The frame number in the UTF-8 style coding, 1 .. 6 bytes, v < 2^31."""
    if v < 0x80:
        return bytes([v])
    for nb, top in ((2, 0x800), (3, 0x10000), (4, 0x200000), (5, 0x4000000), (6, 0x80000000)):
        if v < top:
            break
    else:
        raise ValueError('frame number >= 2^31')
    out = [((0xFF << (8 - nb)) & 0xFF) | (v >> (6 * (nb - 1)))]
    for i in range(nb - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


def crc8(data):
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


def _crc16_table():
    tab = []
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
        tab.append(c)
    return tab


_CRC16 = _crc16_table()


def crc16(data):
    crc = 0
    for b in data:
        crc = ((crc << 8) & 0xFFFF) ^ _CRC16[((crc >> 8) ^ b) & 0xFF]
    return crc


def _field_bits(values, width):
    """values (int64, two's complement taken modulo 2^width) as rows of `width` bits, MSB first -> flat uint8 0/1."""
    v = np.asarray(values, dtype=np.int64) & ((1 << width) - 1)
    sh = np.arange(width - 1, -1, -1, dtype=np.int64)
    return ((v[:, None] >> sh[None, :]) & 1).astype(np.uint8).reshape(-1)


def residual(q, o):
    r = np.asarray(q, dtype=np.int64)
    for _ in range(o):
        r = np.diff(r)
    return r                                                   # the o-th difference: bs - o values


def zigzag(r):
    return np.where(r >= 0, 2 * r, -2 * r - 1).astype(np.int64)


def partition_costs(u_part):
    """(best cost, best k) of one partition: min over k of 5 + n (k + 1) + sum(u >> k), the smallest k of a tie."""
    n = len(u_part)
    ks = np.arange(K_MAX + 1, dtype=np.int64)
    sums = (u_part[None, :] >> ks[:, None]).sum(axis=1)
    cost = 5 + n * (ks + 1) + sums
    k = int(np.argmin(cost))                                   # first minimum = smallest k
    return int(cost[k]), k, cost


def choose(q, bps):
    """(kind, o, p, ks, bits) by the rule; also the set of partitions where a tie was decided by the smallest k."""
    bs = len(q)
    if np.all(q == q[0]):
        return 'CONSTANT', 0, 0, [], 8 + bps, 0
    best = None
    for o in range(5):
        if bs <= o:
            break
        u = zigzag(residual(q, o))
        best_o = None
        p = 0
        while p <= P_MAX and bs % (1 << p) == 0 and (bs >> p) > o:
            plen = bs >> p
            total, ks, ties = 8 + o * bps + 2 + 4, [], 0
            for j in range(1 << p):
                a = 0 if j == 0 else j * plen - o
                part = u[a:(j + 1) * plen - o]
                c, k, cost = partition_costs(part)
                ties += int(np.count_nonzero(cost == c) > 1)
                total += c
                ks.append(k)
            if best_o is None or total < best_o[0]:            # smallest p on ties
                best_o = (total, p, ks, ties)
            p += 1
        if best is None or best_o[0] < best[0]:                # smallest o on ties
            best = (best_o[0], o, best_o[1], best_o[2], best_o[3])
    if best[0] < 8 + bs * bps:
        return 'FIXED', best[1], best[2], best[3], best[0], best[4]
    return 'VERBATIM', 0, 0, [], 8 + bs * bps, 0


def subframe_bits(q, bps, kind, o, p, ks):
    bs = len(q)
    if kind == 'CONSTANT':
        return np.concatenate([_field_bits([0], 8), _field_bits(q[:1], bps)])
    if kind == 'VERBATIM':
        return np.concatenate([_field_bits([0x02], 8), _field_bits(q, bps)])
    u = zigzag(residual(q, o))
    plen = bs >> p
    part = (np.arange(o, bs) // plen)                          # partition of every residual
    k = np.asarray(ks, dtype=np.int64)[part]
    first = np.ones(len(u), dtype=bool)
    first[1:] = part[1:] != part[:-1]
    length = (u >> k) + 1 + k + np.where(first, 5, 0)
    start = np.concatenate([[0], np.cumsum(length)[:-1]])
    bits = np.zeros(int(length.sum()), dtype=np.uint8)
    # the 5-bit parameter in front of each partition's first code
    for b in range(5):
        bits[start[first] + b] = (k[first] >> (4 - b)) & 1
    stop = start + np.where(first, 5, 0) + (u >> k)
    bits[stop] = 1
    for b in range(int(k.max()) if len(k) else 0):             # low bit k - 1 - b of u right after the stop bit
        sel = k > b
        bits[stop[sel] + 1 + b] = (u[sel] >> (k[sel] - 1 - b)) & 1
    head = np.concatenate([_field_bits([(8 + o) << 1], 8), _field_bits(q[:o], bps), _field_bits([0x10 | p], 6)])
    return np.concatenate([head, bits])


def encode_frame(q, bps, number):
    """One frame of the block q (int64, 1 .. 65536 samples) -> (bytes, (kind, o, p, ks))."""
    q = np.asarray(q, dtype=np.int64)
    bs = len(q)
    kind, o, p, ks, nbits, ties = choose(q, bps)
    hdr = bytes([0xFF, 0xF8, 0x70, {16: 4, 24: 6}[bps] << 1]) + utf8_num(number) + (bs - 1).to_bytes(2, 'big')
    hdr += bytes([crc8(hdr)])
    body = subframe_bits(q, bps, kind, o, p, ks)
    assert len(body) == nbits, (len(body), nbits)
    fr = hdr + np.packbits(body).tobytes()                     # packbits pads the last byte with zero bits
    fr += crc16(fr).to_bytes(2, 'big')
    return fr, (kind, o, p, list(ks), ties)


def encode_frames(q, bps=24, blocksize=4096, first_frame=0):
    q = np.asarray(q, dtype=np.int64)
    frames, choices = [], []
    for i, s0 in enumerate(range(0, len(q), blocksize)):
        fr, ch = encode_frame(q[s0:s0 + blocksize], bps, first_frame + i)
        frames.append(fr)
        choices.append(ch)
    return frames, choices


def pcm_md5(q, bps):
    nbytes = bps // 8
    raw = np.asarray(q, dtype='<i8').reshape(-1).view(np.uint8).reshape(-1, 8)[:, :nbytes]
    return hashlib.md5(np.ascontiguousarray(raw).tobytes()).digest()


def stream_header(n, sr, bps, blocksize, min_frame, max_frame, md5):
    si = blocksize.to_bytes(2, 'big') * 2 + min_frame.to_bytes(3, 'big') + max_frame.to_bytes(3, 'big')
    si += ((sr << 44) | ((bps - 1) << 36) | n).to_bytes(8, 'big') + md5
    return b'fLaC' + bytes([0x80]) + len(si).to_bytes(3, 'big') + si


def encode_file(y, sr=44100, bps=24, blocksize=4096, first_frame=0):
    """float32 waveform -> (file bytes, choices)."""
    q = quantise(y, bps)
    frames, choices = encode_frames(q, bps, blocksize, first_frame)
    sizes = [len(f) for f in frames]
    head = stream_header(len(q), sr, bps, blocksize, min(sizes) if sizes else 0, max(sizes) if sizes else 0,
                         pcm_md5(q, bps))
    return head + b''.join(frames), choices


# ---- the committed input set: every branch of the rule (test_flac_encode_cpu asserts the coverage) ----
def signals(n=8229, seed=5):
    """name -> float32 waveform of n samples."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    tone = 0.5 * np.exp(-t / 30000.0) * np.sin(2 * np.pi * 440.0 * t / 44100.0)
    out = {
        'zeros': np.zeros(n),
        'dc': np.full(n, 0.25),
        'impulse': np.where(t == 1000, 0.5, 0.0),
        'noise_full': rng.uniform(-1.0, 1.0, n),
        'square': np.where((t // 50) % 2 == 0, 1.0, -1.0),
        'tone': tone,
        'tone_noise': tone + 1e-3 * rng.standard_normal(n),
        'loud_quiet': np.where(t % 4096 < 2048, 0.3, 1e-4) * rng.standard_normal(n),
        'walk': np.cumsum(rng.standard_normal(n)) * 1e-3,
        'walk2': np.cumsum(np.cumsum(rng.standard_normal(n))) * 2e-6,
        'walk3': np.cumsum(np.cumsum(np.cumsum(rng.integers(-1, 2, n)))) * 2.0 ** -23,
        'tiny': rng.integers(0, 2, n) * 2.0 ** -23,
        'sparse': np.where(rng.uniform(size=n) < 0.02, 2.0 ** -23, 0.0),
        'ramp': (t % 7) * 2.0 ** -23 * 3,
    }
    return {k: np.clip(v, -4.0, 4.0).astype(np.float32) for k, v in out.items()}
