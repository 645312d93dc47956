"""The spectrogram-image rule restated in Python, independent of csrc/amt_png_core.h and of amt_saga.png:
a writer of the PNG rule (row filters by smallest absolute residue, pieces of whole rows, run-length tokens, the smallest
of stored / fixed / dynamic blocks, length-limited Huffman by the stated integer rule), a reader that trusts nothing of it
(chunk walk, zlib.crc32, zlib.decompress, un-filtering in numpy), the level rule, and the case corpus of the tests."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
PIECE_BYTES = 32768
MAX_DIM = 16384
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
KINDS = ('stored', 'fixed', 'dynamic')


# ---------------------------------------------------------------------------------------------------------------
# the level rule
# ---------------------------------------------------------------------------------------------------------------
def thresholds(top_db=80.0):
    return np.array([10.0 ** (-(top_db / 20.0) * (1.0 - (k - 0.5) / 255.0)) for k in range(1, 256)], np.float64).astype(np.float32)


def cols(T, W):
    return [(i * T // W, max(i * T // W + 1, (i + 1) * T // W)) for i in range(W)]


def levels(mag, ref, rows, columns, thr):
    """mag [T, >= F] float32 (host), rows [(lo, hi)] over bins with row 0 the top, columns [(lo, hi)] over frames."""
    ref = np.float32(ref)
    H, W = len(rows), len(columns)
    out = np.zeros((H, W), np.uint8)
    if not np.isfinite(ref) or ref < np.float32(2.0 ** -100):
        return out
    prod = (np.asarray(thr, np.float32) * ref).astype(np.float32)          # one float32 multiply each
    for j, (b0, b1) in enumerate(rows):
        for i, (t0, t1) in enumerate(columns):
            cell = mag[t0:t1, b0:b1].astype(np.float32).reshape(-1)
            v = np.float32(0)
            for x in cell[~np.isnan(cell)]:
                if x > v:
                    v = x
            out[j, i] = int(np.sum(v >= prod))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------
def filter_rows(img):
    """[H, 1 + W] uint8: every row behind the number of the filter with the smallest sum of |signed residue|."""
    x = np.asarray(img, np.uint8).astype(np.int32)
    H, W = x.shape
    a = np.concatenate([np.zeros((H, 1), np.int32), x[:, :-1]], axis=1)
    b = np.concatenate([np.zeros((1, W), np.int32), x[:-1]], axis=0)
    c = np.concatenate([np.zeros((H, 1), np.int32), b[:, :-1]], axis=1)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)                  # [5, H]
    pick = np.argmin(cost, axis=0)                                          # the first smallest: the lower number
    out = np.empty((H, 1 + W), np.uint8)
    out[:, 0] = pick
    out[:, 1:] = res[pick, np.arange(H)]
    return out


def piece_rows(W):
    return max(1, PIECE_BYTES // (W + 1))


def length_symbol(n):
    """(symbol, extra bits, extra value) of a match length 3 .. 258, from the table of RFC 1951 3.2.5."""
    if n == 258:
        return 285, 0, 0
    base, sym = 3, 257
    for eb in (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5):
        if n < base + (1 << eb):
            return sym, eb, n - base
        base += 1 << eb
        sym += 1
    raise AssertionError(n)


def run_tokens(data):
    """[(symbol, extra bits, extra value)]: literals and distance-1 matches of the piece `data`, run by run."""
    d = np.frombuffer(bytes(data), np.uint8)
    starts = np.concatenate([[0], np.flatnonzero(d[1:] != d[:-1]) + 1, [len(d)]])
    toks = []
    for s, e in zip(starts[:-1].tolist(), starts[1:].tolist()):
        v, m = int(d[s]), e - s - 1
        toks.append((v, 0, 0))
        toks += [(285, 0, 0)] * (m // 258)
        rem = m % 258
        toks += [length_symbol(rem)] if rem >= 3 else [(v, 0, 0)] * rem
    return toks


def code_lengths(freq, limit):
    """The integer rule: pad to two used symbols; Huffman with two queues over the symbols sorted by (count, symbol),
    the leaf first on equal weights; depths cut at `limit`; Kraft repair; lengths handed out from the most frequent."""
    freq = list(freq)
    for s in range(len(freq)):
        if sum(1 for f in freq if f) >= 2:
            break
        if freq[s] == 0:
            freq[s] = 1
    order = sorted((s for s in range(len(freq)) if freq[s]), key=lambda s: (freq[s], s))
    m = len(order)
    w = [freq[s] for s in order]
    parent = [0] * (2 * m)
    leaf, inner = 0, m
    while len(w) < 2 * m - 1:
        pick = []
        for _ in range(2):
            if leaf < m and (inner >= len(w) or w[leaf] <= w[inner]):
                pick.append(leaf)
                leaf += 1
            else:
                pick.append(inner)
                inner += 1
        for k in pick:
            parent[k] = len(w)
        w.append(w[pick[0]] + w[pick[1]])
    depth = [0] * (2 * m - 1)
    for i in range(2 * m - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    count = [0] * (limit + 2)
    for i in range(m):
        count[min(depth[i], limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total > 1 << limit:
        count[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    lens = [0] * len(freq)
    j = m
    for l in range(1, limit + 1):
        for _ in range(count[l]):
            j -= 1
            lens[order[j]] = l
    return lens


def canonical(lens):
    """{symbol: (code with its first bit lowest, bits)} of the canonical code (RFC 1951 3.2.2)."""
    code, out = 0, {}
    for l in range(1, 16):
        for s, n in enumerate(lens):
            if n == l:
                out[s] = (int(format(code, '0%db' % l)[::-1], 2), l)
                code += 1
        code <<= 1
    return out


FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def cl_tokens(seq):
    out, i = [], 0
    while i < len(seq):
        e = i
        while e < len(seq) and seq[e] == seq[i]:
            e += 1
        r, v = e - i, seq[i]
        if v == 0:
            while r >= 11:
                t = min(r, 138)
                out.append((18, 7, t - 11))
                r -= t
            if r >= 3:
                out.append((17, 3, r - 3))
                r = 0
            out += [(0, 0, 0)] * r
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                t = min(r, 6)
                out.append((16, 2, t - 3))
                r -= t
            out += [(v, 0, 0)] * r
        i = e
    return out


def pack_bits(fields):
    """[(value, bits)] least significant bit first -> (bytes zero-padded to a whole byte, bit count)."""
    if not fields:
        return b'', 0
    vals = np.array([f[0] for f in fields], np.int64)
    bits = np.array([f[1] for f in fields], np.int64)
    keep = bits > 0
    vals, bits = vals[keep], bits[keep]
    total = int(bits.sum())
    idx = np.repeat(np.arange(len(bits)), bits)
    within = np.arange(total) - np.repeat(np.cumsum(bits) - bits, bits)
    return np.packbits(((vals[idx] >> within) & 1).astype(np.uint8), bitorder='little').tobytes(), total


def block_fields(toks, codes, dist):
    out = []
    for s, eb, ev in toks:
        out.append(codes[s])
        if s > 256:
            out += [(ev, eb), dist]
    out.append(codes[256])
    return out


def encode_piece(data, last):
    """(deflate bytes of the piece, kind): one block, byte-aligned at its end."""
    n = len(data)
    toks = run_tokens(data)
    freq = [0] * 286
    for s, _, _ in toks:
        freq[s] += 1
    freq[256] = 1
    final = 1 if last else 0
    fixed = [(final | 2, 3)] + block_fields(toks, canonical(FIXED_LENS), (0, 5))
    lens = code_lengths(freq, 15)
    hlit = max(257, max(s for s in range(286) if lens[s]) + 1)
    cl = cl_tokens(lens[:hlit] + [1])
    cl_freq = [0] * 19
    for s, _, _ in cl:
        cl_freq[s] += 1
    cl_lens = code_lengths(cl_freq, 7)
    cl_codes = canonical(cl_lens)
    hclen = 19
    while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    dyn = [(final | 4, 3), (hlit - 257, 5), (0, 5), (hclen - 4, 4)] + [(cl_lens[CL_ORDER[k]], 3) for k in range(hclen)]
    for s, eb, ev in cl:
        dyn += [cl_codes[s], (ev, eb)]
    dyn += block_fields(toks, canonical(lens), (0, 1))
    cands = [bytes([final, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + bytes(data)]
    for fields in (fixed, dyn):
        body, bits = pack_bits(fields)
        if not last:                                                  # the empty stored block: 000, padding, 00 00 FF FF
            body = body + (b'\0' if (bits + 3 + 7) // 8 > len(body) else b'') + b'\x00\x00\xff\xff'
        cands.append(body)
    kind = min(range(3), key=lambda k: (len(cands[k]), k))
    return cands[kind], KINDS[kind]


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def encode(img, palette=None, info=None):
    """The bytes of the PNG file of `img` (uint8 [H, W]); palette: uint8 [256, 3] or None (greyscale).  info: a dict that
    receives the kinds, the filters and the IDAT payload bytes."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    assert 1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM
    fb = filter_rows(img)
    out = SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 0 if palette is None else 3, 0, 0, 0))
    if palette is not None:
        out += chunk(b'PLTE', np.asarray(palette, np.uint8).reshape(256, 3).tobytes())
    R = piece_rows(W)
    kinds, payload = [], 0
    for y in range(0, H, R):
        last = y + R >= H
        body, kind = encode_piece(fb[y:y + R].tobytes(), last)
        kinds.append(kind)
        data = (b'\x78\x01' if y == 0 else b'') + body + (struct.pack('>I', zlib.adler32(fb.tobytes())) if last else b'')
        payload += len(data)
        out += chunk(b'IDAT', data)
    if info is not None:
        info.update(kinds=kinds, filters=fb[:, 0].tolist(), payload=payload, filtered=fb.tobytes())
    return out + chunk(b'IEND', b'')


# ---------------------------------------------------------------------------------------------------------------
# the reader
# ---------------------------------------------------------------------------------------------------------------
def decode(data, pixels=True):
    """(image uint8 [H, W] or None, palette uint8 [256, 3] or None, chunk names) of a PNG file, every CRC checked."""
    assert data[:8] == SIGNATURE, 'signature'
    at, names, idat, hdr, pal = 8, [], [], None, None
    while at < len(data):
        n, kind = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert len(body) == n, 'chunk past the end'
        assert struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), 'CRC of ' + repr(kind)
        names.append(kind)
        if kind == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'PLTE':
            pal = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b'IDAT':
            idat.append(body)
        at += 12 + n
    assert at == len(data) and names[0] == b'IHDR' and names[-1] == b'IEND' and names.count(b'IEND') == 1
    W, H, depth, colour, comp, filt, lace = hdr
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 3) and (colour == 3) == (pal is not None)
    raw = zlib.decompress(b''.join(idat))
    assert len(raw) == H * (W + 1), 'filtered bytes'
    if not pixels:
        return np.zeros((H, W), np.uint8)[:0], pal, names
    rows = np.frombuffer(raw, np.uint8).reshape(H, W + 1)
    img = np.zeros((H, W), np.uint8)
    prev = np.zeros(W, np.int32)
    for y in range(H):
        f, r = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if f == 0:
            cur = r
        elif f == 1:
            cur = np.cumsum(r) & 255
        elif f == 2:
            cur = (r + prev) & 255
        else:
            assert f in (3, 4), 'filter'
            cur = np.zeros(W, np.int32)
            a = c = 0
            for x in range(W):
                b = int(prev[x])
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                a = (int(r[x]) + pred) & 255
                c = b
                cur[x] = a
        img[y] = cur
        prev = cur
    return img, pal, names


# ---------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------
def filter_images():
    """{filter number: an image built so that most of its rows choose that filter}."""
    rng = np.random.default_rng(5)
    H, W = 10, 30
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    none = ((ii + jj) & 1).astype(np.uint8)                               # a checkerboard
    slope = np.array([16, 8, 4, 2, 1] * 2)
    sub = (slope[:, None] * ii).astype(np.uint8)                          # ramps from 0, each half as steep as the one above
    top = (np.arange(W) * 7 % 50) * 4
    up = (top[None, :] + jj).astype(np.uint8)                             # every row the one above plus one
    avg = np.zeros((H, W), np.int32)
    avg[0] = rng.integers(0, 256, W)
    avg[:, 0] = rng.integers(0, 256, H)
    for y in range(1, H):
        for x in range(1, W):
            avg[y, x] = (avg[y, x - 1] + avg[y - 1, x]) >> 1
    cstep = np.where(rng.integers(0, 2, W) == 1, 12, 1)
    paeth = (np.cumsum(cstep)[None, :] + 5 * jj).astype(np.uint8)         # a plane with uneven steps
    return {0: none, 1: sub, 2: up, 3: avg.astype(np.uint8), 4: paeth}


def corpus():
    """[(name, image uint8 [H, W])]: the encoder shapes of the tests."""
    rng = np.random.default_rng(1)
    out = [('1x1', np.array([[7]], np.uint8)), ('1xN', np.arange(37, dtype=np.uint8)[:, None] * 5),
           ('Nx1', (np.arange(300) % 251).astype(np.uint8)[None, :])]
    for w in (258, 259, 260, 517):                                     # one repeated byte: the 258 cap and its remainders
        out.append(('run%d' % w, np.full((2, w), 9, np.uint8)))
    short = np.zeros((3, 40), np.uint8)
    short[0, :9] = [1, 1, 2, 2, 2, 3, 3, 3, 3]                             # runs of 2, 3 and 4
    short[1, 5:7], short[2, 9:12] = 200, 100
    out.append(('runs234', short))
    out.append(('zeros', np.zeros((50, 70), np.uint8)))
    out.append(('noise255', rng.integers(0, 256, (90, 130)).astype(np.uint8)))
    out.append(('noise15', rng.integers(0, 16, (90, 130)).astype(np.uint8)))
    out.append(('small', np.array([[1, 200, 3], [90, 5, 60]], np.uint8)))
    for f, img in filter_images().items():
        out.append(('filter%d' % f, img))
    W = 4095
    R = piece_rows(W)
    assert R == 8
    base = (rng.integers(0, 8, (2 * R + 1, W)) * rng.integers(0, 2, (2 * R + 1, 1)) + np.arange(W)[None, :] // 700).astype(np.uint8)
    for h in (R - 1, R, R + 1, 2 * R + 1):
        out.append(('rows%d' % h, base[:h]))
    wide = (np.arange(MAX_DIM)[None, :] // 64 + np.arange(3)[:, None]).astype(np.uint8)    # the widest row: one per piece
    out.append(('widest', wide))
    return out


def ragged_six():
    rng = np.random.default_rng(2)
    sizes = [(5, 3), (64, 64), (1, 9), (300, 2), (33, 120), (129, 17)]
    return [np.minimum(rng.integers(0, 40, (h, w)), rng.integers(0, 255, (h, 1))).astype(np.uint8) for w, h in sizes]
