"""numpy restatement of the device FLAC encoder's rule with linear prediction, independent of the
product's encoder: nothing of amt_saga is imported.  The frame header, the quantiser, the CRCs, the Rice2 partition cost,
the MD5 and STREAMINFO are flac_encode_reference's; this file adds the LPC candidates.

    The candidates of a block that is not CONSTANT, in this order: FIXED o = 0..4 (flac_encode_reference.choose), then
    LPC m = 1..L with bs > m.  A candidate replaces the best so far only if its bit count is strictly smaller; VERBATIM
    unless the best is strictly below 8 + bs bps.

    analyse(q, bps, L)                        -> per order (shift, [c_j]) or None
    choose(q, bps, L)                         -> (kind, order, p, ks, bits, extra)
    encode_frame / encode_frames / encode_file   as flac_encode_reference's, with lpc_order

Integers wherever a sum could be reordered (window, autocorrelation, residual); the recurrence and the quantiser are
float64 in ONE operation order, written with Python floats: every + - * / is one IEEE operation, never fused.
"""
import math

import numpy as np

import flac_encode_reference as R

MAX_ORDER = 12
RESID_LIMIT = 1 << 27


def precision(bps):
    return 12 if bps == 16 else 14


def window(bs):
    i = np.arange(bs, dtype=np.int64)
    return ((4 * (i + 1) * (bs - i)) << 14) // ((bs + 1) * (bs + 1))


def autocorrelation(q, lags=MAX_ORDER):
    """R_l, l = 0 .. lags, of the windowed block as Python ints (|R| < 2^59: int64 holds every partial sum)."""
    q = np.asarray(q, dtype=np.int64)
    bs = len(q)
    x = (q * window(bs)) >> 14
    return [int(np.dot(x[l:], x[:bs - l])) if l < bs else 0 for l in range(lags + 1)]


def quantise_coefficients(a, P):
    """a (floats) -> (shift, [c_j]) or None."""
    if not all(math.isfinite(v) for v in a):
        return None
    cmax = max(abs(v) for v in a)
    if not cmax > 0.0:
        return None
    e = max(math.frexp(cmax)[1], -1022)
    shift = min(max(P - 1 - e, 0), 15)
    scale = float(1 << shift)
    hi, lo = float((1 << (P - 1)) - 1), -float(1 << (P - 1))
    fe, c = 0.0, []
    for v in a:
        fe = fe + v * scale
        r = float(np.rint(fe))                                  # half to even
        r = hi if r > hi else (lo if r < lo else r)
        c.append(int(r))
        fe = fe - r
    return shift, c


def analyse(q, bps, max_order):
    """[(shift, coefficients) or None for m = 1 .. max_order]: the recurrence in the core header's operation order."""
    out = [None] * max_order
    Rl = autocorrelation(q, max_order)
    if Rl[0] <= 0:
        return out
    r = [float(v) for v in Rl]                                  # int -> float: nearest, ties to even
    P = precision(bps)
    a = []
    err = r[0]
    for m in range(1, max_order + 1):
        acc = r[m]
        for j in range(m - 1):
            acc = acc - a[j] * r[m - 1 - j]
        k = acc / err
        a = [a[j] - k * a[m - 2 - j] for j in range(m - 1)] + [k]
        out[m - 1] = quantise_coefficients(a, P)
        kk = k * k
        err = err * (1.0 - kk)
        if not err > 0.0:
            break
    return out


def lpc_residual(q, c, shift):
    """r_i, i = m .. bs - 1 (int64 sums, arithmetic shift)."""
    q = np.asarray(q, dtype=np.int64)
    m, bs = len(c), len(q)
    s = np.zeros(bs - m, dtype=np.int64)
    for j, cj in enumerate(c):
        s += np.int64(cj) * q[m - 1 - j:bs - 1 - j]
    return q[m:] - (s >> shift)


def partition_search(u, o, bs):
    """(sum of the partition costs, p, ks, ties) over p = 0 .. 8 while 2^p | bs and (bs >> p) > o: the smallest total,
    the smallest p of a tie; per partition flac_encode_reference.partition_costs' rule, all partitions of a level at
    once (test_flac_lpc_cpu pins the two against each other)."""
    up = np.concatenate([np.zeros(o, dtype=np.int64), np.asarray(u, dtype=np.int64)])      # warm-up: no residual
    ks = np.arange(R.K_MAX + 1, dtype=np.int64)
    sh = up[None, :] >> ks[:, None]
    best, p = None, 0
    while p <= R.P_MAX and bs % (1 << p) == 0 and (bs >> p) > o:
        plen = bs >> p
        sums = sh.reshape(len(ks), 1 << p, plen).sum(axis=2)
        n = np.full(1 << p, plen, dtype=np.int64)
        n[0] -= o
        cost = 5 + n[None, :] * (ks[:, None] + 1) + sums
        k = np.argmin(cost, axis=0)                              # first minimum = smallest k
        c = cost[k, np.arange(1 << p)]
        ties = int(np.count_nonzero((cost == c[None, :]).sum(axis=0) > 1))
        total = int(c.sum())
        if best is None or total < best[0]:
            best = (total, p, [int(v) for v in k], ties)
        p += 1
    return best


def lpc_bits(m, bps):
    """Bits of an LPC subframe of order m before the partition costs."""
    return 8 + m * bps + 4 + 5 + m * precision(bps) + 6


def choose(q, bps, lpc_order=MAX_ORDER):
    """(kind, order, p, ks, bits, extra): extra = dict(shift, coef, tie_with_fixed, fixed_bits, disqualified) for every
    kind but CONSTANT."""
    q = np.asarray(q, dtype=np.int64)
    bs = len(q)
    kind, o, p, ks, bits, _ = R.choose(q, bps)
    if kind == 'CONSTANT':
        return kind, o, p, ks, bits, None
    # (a VERBATIM answer hides a FIXED count that is not below 8 + bs bps: an LPC candidate has to beat both anyway)
    best = (kind, o, p, ks, bits)
    extra = dict(shift=None, coef=None, tie_with_fixed=False, fixed_bits=bits, disqualified=[])
    max_order = min(lpc_order, bs - 1)
    totals = []
    for m, qc in enumerate(analyse(q, bps, max_order), 1):
        if qc is None:
            continue
        shift, c = qc
        r = lpc_residual(q, c, shift)
        if np.any(np.abs(r) >= RESID_LIMIT):
            extra['disqualified'].append(m)
            continue
        total, pp, kk, _ = partition_search(R.zigzag(r), m, bs)
        total += lpc_bits(m, bps)
        totals.append(total)
        if total < best[4]:
            best = ('LPC', m, pp, kk, total)
            extra.update(shift=shift, coef=c)
    extra['tie_with_fixed'] = best[0] == 'FIXED' and best[4] in totals      # equal counts: FIXED is kept
    return best + (extra,)


def rice_bits(u, o, bs, p, ks):
    """The residual coding of DESIGN 15: per partition a 5-bit parameter, per residual u >> k zeros, a one, k low bits."""
    u = np.asarray(u, dtype=np.int64)
    plen = bs >> p
    part = np.arange(o, bs) // plen
    k = np.asarray(ks, dtype=np.int64)[part]
    first = np.ones(len(u), dtype=bool)
    first[1:] = part[1:] != part[:-1]
    length = (u >> k) + 1 + k + np.where(first, 5, 0)
    start = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int64)
    bits = np.zeros(int(length.sum()), dtype=np.uint8)
    for b in range(5):
        bits[start[first] + b] = (k[first] >> (4 - b)) & 1
    stop = start + np.where(first, 5, 0) + (u >> k)
    bits[stop] = 1
    for b in range(int(k.max()) if len(k) else 0):
        sel = k > b
        bits[stop[sel] + 1 + b] = (u[sel] >> (k[sel] - 1 - b)) & 1
    return bits


def lpc_subframe_bits(q, bps, m, p, ks, shift, c):
    P = precision(bps)
    head = np.concatenate([R._field_bits([(32 + m - 1) << 1], 8), R._field_bits(q[:m], bps), R._field_bits([P - 1], 4),
                           R._field_bits([shift], 5), R._field_bits(c, P), R._field_bits([0x10 | p], 6)])
    return np.concatenate([head, rice_bits(R.zigzag(lpc_residual(q, c, shift)), m, len(q), p, ks)])


def encode_frame(q, bps, number, lpc_order=MAX_ORDER):
    """One frame of the block q -> (bytes, (kind, order, p, ks, extra))."""
    q = np.asarray(q, dtype=np.int64)
    bs = len(q)
    kind, o, p, ks, nbits, extra = choose(q, bps, lpc_order)
    hdr = bytes([0xFF, 0xF8, 0x70, {16: 4, 24: 6}[bps] << 1]) + R.utf8_num(number) + (bs - 1).to_bytes(2, 'big')
    hdr += bytes([R.crc8(hdr)])
    if kind == 'LPC':
        body = lpc_subframe_bits(q, bps, o, p, ks, extra['shift'], extra['coef'])
    else:
        body = R.subframe_bits(q, bps, kind, o, p, ks)
    assert len(body) == nbits, (len(body), nbits)
    fr = hdr + np.packbits(body).tobytes()
    fr += R.crc16(fr).to_bytes(2, 'big')
    return fr, (kind, o, p, list(ks), extra)


def encode_frames(q, bps=24, blocksize=4096, first_frame=0, lpc_order=MAX_ORDER):
    q = np.asarray(q, dtype=np.int64)
    frames, choices = [], []
    for i, s0 in enumerate(range(0, len(q), blocksize)):
        fr, ch = encode_frame(q[s0:s0 + blocksize], bps, first_frame + i, lpc_order)
        frames.append(fr)
        choices.append(ch)
    return frames, choices


def encode_file(y, sr=44100, bps=24, blocksize=4096, first_frame=0, lpc_order=MAX_ORDER):
    """float32 waveform -> (file bytes, choices)."""
    q = R.quantise(y, bps)
    frames, choices = encode_frames(q, bps, blocksize, first_frame, lpc_order)
    sizes = [len(f) for f in frames]
    head = R.stream_header(len(q), sr, bps, blocksize, min(sizes) if sizes else 0, max(sizes) if sizes else 0,
                           R.pcm_md5(q, bps))
    return head + b''.join(frames), choices


# ---- inputs beside flac_encode_reference.signals() ----
def more_signals(n=8229, seed=11):
    """name -> float32 waveform: decaying harmonics over low-passed noise (what a stem looks like), a loud copy whose
    coefficients are large, and a two-sample oscillation."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    harm = sum(0.25 / h * np.exp(-t / (20000.0 / h)) * np.sin(2 * np.pi * 196.0 * h * t / 44100.0 + h) for h in range(1, 7))
    lp = np.convolve(rng.standard_normal(n + 15), np.hanning(16) / 8.0, 'valid') * 2e-3
    out = {
        'harmonics': harm + lp,
        'harmonics_quiet': (harm + lp) * 2.0 ** -9,
        'lowpass': lp * 40.0,
        'alternating': np.where(t % 2 == 0, 0.7, -0.7) * np.exp(-t / 9000.0),
        'slow_sine': 0.9 * np.sin(2 * np.pi * 31.0 * t / 44100.0),
    }
    return {k: np.clip(v, -4.0, 4.0).astype(np.float32) for k, v in out.items()}
