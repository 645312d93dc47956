"""Test-side WAV writer in numpy / struct, independent of amt_saga/wav.py: any tag / container / valid-bits
combination, extra chunks with odd sizes, 16- / 18- / 40-byte fmt chunks, wrong data sizes -- and the value rule
restated, so that the host reader, the sanitised core and the kernels are all held to the same numbers.

    integer, container c bytes (little-endian, signed; c = 1 unsigned, u - 128), valid bits b, MSB-justified:
        q = container >> (8 c - b) (arithmetic); wave = float32(q) 2^-(b-1); pcm = q
    float32: the bits as they are; float64: rounded to float32 (numpy astype)
"""
import struct

import numpy as np

PCM_GUID_TAIL = bytes.fromhex('000000001000800000aa00389b71')        # KSDATAFORMAT_SUBTYPE_*: tag + these 14 bytes
TILE = 1024                                                           # values one workgroup takes (audio.PCM_TILE)


def chunk(cid, body, pad=True):
    """One RIFF chunk; an odd-sized body is followed by one pad byte."""
    return cid + struct.pack('<I', len(body)) + body + (b'\0' if pad and len(body) & 1 else b'')


def fmt_chunk(tag, channels, sr, container, valid, size=16, block_align=None, valid_field=None):
    ba = container * channels if block_align is None else block_align
    if size == 40:
        body = struct.pack('<HHIIHH', 0xFFFE, channels, sr, sr * ba & 0xFFFFFFFF, ba, 8 * container)
        body += struct.pack('<HHI', 22, valid if valid_field is None else valid_field, 0)
        body += struct.pack('<H', tag) + PCM_GUID_TAIL
    else:
        body = struct.pack('<HHIIHH', tag, channels, sr, sr * ba & 0xFFFFFFFF, ba, valid)
        if size == 18:
            body += struct.pack('<H', 0)
    assert len(body) == size
    return chunk(b'fmt ', body)


def containers(x, kind, c, b, low=0):
    """The data bytes of x [n, channels]: for integers x holds q (b valid bits), placed MSB-justified with `low` in the
    ignored low bits; floats as they are (c = 4) or widened (c = 8)."""
    x = np.asarray(x)
    if kind == 'float':
        return np.ascontiguousarray(x, dtype='<f4' if c == 4 else '<f8').tobytes()
    sh = max(8 * c - b, 0)                                              # (b above the container: a header to be refused)
    v = (x.astype(np.int64) << sh) | (int(low) & ((1 << sh) - 1))
    if c == 1:
        return (v + 128).astype(np.uint8).tobytes()
    raw = (v & ((1 << (8 * c)) - 1)).astype('<u8').reshape(-1)
    return np.ascontiguousarray(raw.view(np.uint8).reshape(-1, 8)[:, :c]).tobytes()


def write(x, kind='int', c=2, b=None, sr=44100, fmt_size=16, before=(), between=(), after=(), data_size=None,
          pad_data=True, low=0, magic=b'RIFF', form=b'WAVE', tag=None, block_align=None, fmt=True, valid_field=None):
    """A WAV file of x [n, channels] (or [n]).  before / between / after: (id, body) chunks in front of fmt, between fmt
    and data, and after data; data_size: the declared size of the data chunk when it is to be wrong."""
    x = np.asarray(x)
    x = x[:, None] if x.ndim == 1 else x
    b = 8 * c if b is None else b
    tag = (1 if kind == 'int' else 3) if tag is None else tag
    body = containers(x, kind, c, b, low)
    out = b''.join(chunk(i, d) for i, d in before)
    if fmt:
        out += fmt_chunk(tag, x.shape[1], sr, c, b, fmt_size, block_align, valid_field)
    out += b''.join(chunk(i, d) for i, d in between)
    out += b'data' + struct.pack('<I', len(body) if data_size is None else data_size) + body
    if pad_data and len(body) & 1:
        out += b'\0'
    out += b''.join(chunk(i, d) for i, d in after)
    return magic + struct.pack('<I', (4 + len(out)) & 0xFFFFFFFF) + form + out


def data_offset(data):
    """Byte of the first sample, by a chunk walk of the test's own."""
    pos = 12
    while data[pos:pos + 4] != b'data':
        size = struct.unpack_from('<I', data, pos + 4)[0]
        pos += 8 + size + (size & 1)
    return pos + 8


def rule(q_or_float, kind, b):
    """(wave float32, pcm int32 or None) the reader must return for written values."""
    x = np.asarray(q_or_float)
    if kind == 'float':
        with np.errstate(over='ignore'):
            return (x if x.dtype == np.float32 else x.astype(np.float32)), None
    q = x.astype(np.int32)
    return q.astype(np.float32) * np.float32(2.0 ** -(b - 1)), q


# (kind, container bytes, valid bits, fmt chunk size)
FORMS = (('int', 1, 8, 16), ('int', 2, 16, 16), ('int', 3, 24, 18), ('int', 4, 32, 16), ('int', 2, 12, 40),
         ('int', 3, 20, 40), ('int', 4, 24, 40), ('int', 1, 5, 40), ('float', 4, 32, 18), ('float', 8, 64, 40))
FRAMES = (1, 2, 3, 5, TILE // 8 + 1, TILE // 2 - 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
CHANNELS = (1, 2, 3, 8)


def values(kind, c, b, n, ch, seed):
    """Written values [n, ch] with the extremes in front: full scale both ways, 0, -1; for 32-bit, values that round in
    float32; for floats NaN with a payload, -0.0, infinities, a denormal and a double that rounds."""
    rng = np.random.default_rng(seed)
    if kind == 'float':
        x = rng.standard_normal(n * ch).astype(np.float32 if c == 4 else np.float64)
        if c == 4:
            sp = np.array([0x7fc12345, 0xffc00001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x3f800000],
                          np.uint32).view(np.float32)
        else:
            sp = np.array([np.nan, -0.0, np.inf, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e-45, 1e300, -1e-320])
        k = min(len(sp), x.size)
        x[:k] = sp[:k]
        return x.reshape(n, ch)
    lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
    x = rng.integers(lo, hi + 1, n * ch, dtype=np.int64)
    sp = [lo, hi, 0, -1, 1, hi - 1, lo + 1, (1 << 24) + 1, -(1 << 24) - 1, (1 << 25) + 3, hi - 64, (1 << 30) + 64]
    sp = [v for v in sp if lo <= v <= hi]
    k = min(len(sp), x.size)
    x[:k] = sp[:k]
    return x.reshape(n, ch)


_JUNK = (b'LIST', b'\x01\x02\x03'), (b'bext', bytes(range(7))), (b'cue ', b''), (b'fact', struct.pack('<I', 1))


def corpus():
    """[(name, data, wave float32 [n, ch], pcm int32 [n, ch] or None, (kind, c, b))]: every form with every channel
    count, the frame counts taken in rotation, and every form in mono at every frame count; junk chunks (odd-sized
    among them) in front of, between and after the standard ones in rotation."""
    out, k = [], 0
    cases = [(f, ch, None) for f in FORMS for ch in CHANNELS] + [(f, 1, n) for f in FORMS for n in FRAMES]
    for (kind, c, b, fsize), ch, n in cases:
        n = FRAMES[k % len(FRAMES)] if n is None else n
        x = values(kind, c, b, n, ch, seed=k)
        junk = [_JUNK[(k + i) % len(_JUNK)] for i in range(k % 3)]
        data = write(x, kind, c, b, sr=(8000, 44100, 48000, 96000)[k % 4], fmt_size=fsize, before=junk[:1],
                     between=junk[1:], after=junk[:k % 2], pad_data=bool(k % 5), low=0x5a5a5a5a if k % 2 else 0)
        wave, pcm = rule(x, kind, b)
        out.append(('%s%d_%d_ch%d_n%d_%d' % (kind, 8 * c, b, ch, n, k), data, wave, pcm, (kind, c, b)))
        k += 1
    return out


# ---------------------------------------------------------------------------------------------------------------
# the writer's rule restated (wav.encode, audio.wav_encode)
# ---------------------------------------------------------------------------------------------------------------
def quantise(y, bps):
    y = np.asarray(y, np.float32)
    lim = 1 << (bps - 1)
    with np.errstate(all='ignore'):
        r = np.rint(y * np.float32(lim)).astype(np.float64)
    r[np.isnan(r)] = 0
    return np.clip(r, -lim, lim - 1).astype(np.int32)


def expect_file(y, sr, fmt, norm=False):
    """The bytes wav.encode / audio.wav_encode must give for the mono float32 signal y, by the layout of the issue."""
    y = np.asarray(y, np.float32)
    if norm:
        a = np.abs(y)
        a = a[~np.isnan(a)]
        p = np.float32(a.max()) if a.size else np.float32(0)
        if p != 0 and np.isfinite(p):
            with np.errstate(all='ignore'):
                y = (y / p).astype(np.float32)
    if fmt == 'float32':
        body = y.astype('<f4').tobytes()
        return (b'RIFF' + struct.pack('<I', 50 + len(body)) + b'WAVE' + b'fmt ' + struct.pack('<IHHIIHHH', 18, 3, 1, sr,
                sr * 4, 4, 32, 0) + b'fact' + struct.pack('<II', 4, len(y)) + b'data' + struct.pack('<I', len(body))
                + body)
    bps = {'pcm16': 16, 'pcm24': 24}[fmt]
    body = containers(quantise(y, bps)[:, None], 'int', bps // 8, bps)
    D = len(body)
    return (b'RIFF' + struct.pack('<I', 36 + D + (D & 1)) + b'WAVE' + b'fmt ' + struct.pack('<IHHIIHH', 16, 1, 1, sr,
            sr * (bps // 8), bps // 8, bps) + b'data' + struct.pack('<I', D) + body + (b'\0' if D & 1 else b''))


def pack_signals():
    """Mono float32 signals for the writer: NaN, infinities, values at and beyond +-1, half-way rounding cases for both
    widths, lengths 1, odd, even and one past a tile."""
    rng = np.random.default_rng(5)
    h = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5]
    sp = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0 - 2.0 ** -24, 1.5, -3.0, 0.0, -0.0, 1e-30]
                  + [v * 2.0 ** -15 for v in h] + [v * 2.0 ** -23 for v in h] + [32766.5 / 32768, 8388606.5 / 8388608],
                  np.float32)
    sigs = [np.array([0.75], np.float32), sp, sp[::-1].copy()[:-1]]
    for n in (2, 7, TILE - 1, TILE + 5):
        y = (rng.standard_normal(n) * 0.4).astype(np.float32)
        y[:min(n, len(sp))] = sp[:min(n, len(sp))] if n > 2 else y[:n]
        sigs.append(y)
    sigs.append(np.array([np.nan, np.nan, 0.0], np.float32))           # peak 0: left as it is
    sigs.append((rng.standard_normal(33) * 0.1).astype(np.float32))    # all finite: normalisation moves every sample
    return sigs
