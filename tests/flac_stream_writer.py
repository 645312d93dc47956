"""Test infrastructure: a FLAC stream writer in which the caller gives every choice and nothing is searched for --
per-frame block size and its header code, subframe type / order / coefficients / precision / shift, Rice method,
partition order, per-partition k or escape width, wasted bits, channel assignment, blocking strategy, metadata blocks.
Any coefficients give a valid stream, because the residual is defined as sample minus prediction; the writer needs no
encoder intelligence.  Written from the public FLAC format specification.

corpus() is the set of smallest streams at which a decoder can still go wrong (one to three frames each), shared by
the CPU and the GPU tests; damaged(corpus) the hostile variants of it."""
import hashlib

import numpy as np

FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
            16384: 14, 32768: 15}
SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0, (value, nbits)
        self.v = (self.v << nbits) | value
        self.n += nbits

    def signed(self, value, nbits):
        assert nbits == 0 and value == 0 or -(1 << (nbits - 1)) <= value < (1 << (nbits - 1)), (value, nbits)
        self.put(value & ((1 << nbits) - 1), nbits)

    def unary(self, q):
        self.put(1, q + 1)

    def align(self):
        self.put(0, -self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, 'big')


def crc8(data):
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


def crc16(data):
    crc = 0
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x8005) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def utf8_number(v):
    """The UTF-8 style number of a frame header, 1 .. 7 bytes (36 bits)."""
    if v < 0x80:
        return bytes([v])
    for nbytes in range(2, 8):
        if v < 1 << (5 * nbytes + 1) or nbytes == 7:
            tail = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(nbytes - 2, -1, -1)]
            lead = ((0xFF << (8 - nbytes)) & 0xFF) | (v >> (6 * (nbytes - 1)))
            return bytes([lead] + tail)


def pcm_md5(pcm, bps):
    nbytes = (bps + 7) // 8
    raw = np.ascontiguousarray(np.asarray(pcm, np.int64).reshape(-1)).astype('<i8').view(np.uint8).reshape(-1, 8)
    return hashlib.md5(np.ascontiguousarray(raw[:, :nbytes]).tobytes()).digest()


def auto_k(res, limit=30):
    """A Rice parameter near the mean of the folded residuals (the caller's convenience, not a search)."""
    u = [(r << 1) ^ (r >> 63) for r in res]
    m = sum(u) // max(len(u), 1)
    return min(max(m.bit_length() - 1, 0), limit)


def write_subframe(bw, x, bps, spec, forms):
    """x: the subframe's samples (ints), bps: its bits (side channel's extra bit included).
    spec: dict(type='constant'|'verbatim'|'fixed'|'lpc', order, coefs, precision, shift, wasted, method (0 Rice, 1
    Rice2), porder, params = per partition k, ('esc', bits) or None for auto_k)."""
    w = spec.get('wasted', 0)
    bw.put(0, 1)
    typ = spec['type']
    order = spec.get('order', 0)
    code = {'constant': 0, 'verbatim': 1}.get(typ, 8 + order if typ == 'fixed' else 32 + order - 1)
    bw.put(code, 6)
    if w:
        bw.put(1, 1)
        bw.unary(w - 1)
        assert all(v % (1 << w) == 0 for v in x)
        x = [v >> w for v in x]
        bps -= w
        forms.add('WASTED%d' % w)
    else:
        bw.put(0, 1)
    if typ == 'constant':
        assert len(set(x)) == 1
        bw.signed(x[0], bps)
        forms.add('CONSTANT')
        return
    if typ == 'verbatim':
        for v in x:
            bw.signed(v, bps)
        forms.add('VERBATIM')
        return
    for v in x[:order]:
        bw.signed(v, bps)
    if typ == 'fixed':
        co, shift = FIXED[order], 0
        forms.add('FIXED%d' % order)
    else:
        co, shift, prec = spec['coefs'], spec['shift'], spec['precision']
        assert len(co) == order
        bw.put(prec - 1, 4)
        bw.signed(shift, 5)
        for c in co:
            bw.signed(c, prec)
        forms.update(('LPC%d' % order, 'PREC%d' % prec, 'SHIFT%d' % shift))
    res = []
    for i in range(order, len(x)):
        s = sum(c * x[i - j - 1] for j, c in enumerate(co))
        res.append(x[i] - (s >> shift if shift >= 0 else s))
    spec['_max_residual_bits'] = max([abs(r).bit_length() for r in res] + [0])
    spec['_max_sum'] = max([abs(sum(c * x[i - j - 1] for j, c in enumerate(co))) for i in range(order, len(x))] + [0])
    method, porder = spec.get('method', 0), spec.get('porder', 0)
    pbits = 5 if method else 4
    bw.put(method, 2)
    bw.put(porder, 4)
    forms.update(('RICE2' if method else 'RICE', 'PORDER%d' % porder))
    params = spec.get('params') or [None] * (1 << porder)
    at = 0
    for p in range(1 << porder):
        n = spec.get('psize', len(x) >> porder) - (order if p == 0 else 0)
        part = res[at:at + n]
        at += n
        if n == 0:
            forms.add('EMPTY_FIRST_PARTITION')
        k = params[p]
        if k is None:
            k = auto_k(part, 14 if method == 0 else 30)
        if isinstance(k, tuple):
            bw.put((1 << pbits) - 1, pbits)
            bw.put(k[1], 5)
            for r in part:
                bw.signed(r, k[1])
            forms.add('ESCAPE%d' % k[1])
        else:
            bw.put(k, pbits)
            for r in part:
                u = (r << 1) ^ (r >> 63)
                bw.unary(u >> k)
                bw.put(u & ((1 << k) - 1), k)
                if (u >> k) >= 10000:
                    forms.add('UNARY10000')
            forms.add('K%d' % k)


def write_frame(block, bps, spec, number, forms, stream_bps=None):
    """block: int array [bs, channels].  spec: dict(subframes=[per channel spec], assignment=None|8|9|10, bs_code=None
    (chosen from the size) | 6 | 7, ss_code=None | 0, variable=False)."""
    block = np.asarray(block, np.int64)
    bs, ch = block.shape
    ca = spec.get('assignment')
    if ca is None:
        ca = ch - 1
        subs = [(block[:, c].tolist(), bps) for c in range(ch)]
    else:
        left, right = block[:, 0], block[:, 1]
        side = left - right
        if ca == 8:
            subs = [(left.tolist(), bps), (side.tolist(), bps + 1)]
        elif ca == 9:
            subs = [(side.tolist(), bps + 1), (right.tolist(), bps)]
        else:
            subs = [(((left + right) >> 1).tolist(), bps), (side.tolist(), bps + 1)]
            if np.any(side & 1):
                forms.add('ODD_SIDE')
        forms.add('ASSIGNMENT%d' % ca)
    bs_code = spec.get('bs_code')
    if bs_code is None:
        bs_code = BS_CODES.get(bs, 6 if bs <= 256 else 7)
    ss_code = spec.get('ss_code', SS_CODES.get(bps, 0))
    if ss_code == 0:
        assert stream_bps == bps
        forms.add('SS_CODE0')
    hdr = bytearray([0xFF, 0xF9 if spec.get('variable') else 0xF8, (bs_code << 4) | spec.get('sr_code', 0),
                     (ca << 4) | (ss_code << 1)])
    hdr += utf8_number(number)
    if bs_code == 6:
        hdr += bytes([bs - 1])
        forms.add('BS_TAIL8')
    elif bs_code == 7:
        hdr += (bs - 1).to_bytes(2, 'big')
        forms.add('BS_TAIL16')
    else:
        forms.add('BS_CODE%d' % bs_code)
    hdr += {12: bytes([44]), 13: (44100).to_bytes(2, 'big'), 14: (4410).to_bytes(2, 'big')}.get(spec.get('sr_code', 0), b'')
    hdr += bytes([crc8(hdr)])
    bw = Bits()
    for (x, b), sub in zip(subs, spec['subframes']):
        write_subframe(bw, x, b, sub, forms)
    bw.align()
    fr = bytes(hdr) + bw.bytes()
    return fr + crc16(fr).to_bytes(2, 'big')


def write_stream(pcm, bps, frames, sr=44100, metadata=(), forms=None):
    """pcm [n, channels] ints; frames: list of (block size, frame spec) covering n in order.  metadata: extra
    (type, body) blocks after STREAMINFO.  Returns the file's bytes."""
    forms = set() if forms is None else forms
    pcm = np.asarray(pcm, np.int64)
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    n, ch = pcm.shape
    out, at = [], 0
    for fi, (bs, spec) in enumerate(frames):
        number = spec.get('number', at if spec.get('variable') else fi)
        out.append(write_frame(pcm[at:at + bs], bps, spec, number, forms, stream_bps=bps))
        at += bs
    assert at == n, (at, n)
    sizes = [len(f) for f in out]
    bmax = max(bs for bs, _ in frames)
    bmin = min(bs for bs, _ in frames[:-1]) if len(frames) > 1 else bmax
    si = bmin.to_bytes(2, 'big') + bmax.to_bytes(2, 'big') + min(sizes).to_bytes(3, 'big') + max(sizes).to_bytes(3, 'big')
    si += ((sr << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | n).to_bytes(8, 'big') + pcm_md5(pcm, bps)
    blocks = [(0, si)] + list(metadata)
    head = b'fLaC'
    for i, (t, body) in enumerate(blocks):
        head += bytes([(0x80 if i == len(blocks) - 1 else 0) | t]) + len(body).to_bytes(3, 'big') + body
    if len(blocks) > 1:
        forms.add('METADATA%d' % len(blocks))
    return head + b''.join(out)


# ------------------------------------------------------------------------------------
# the corpus
# ------------------------------------------------------------------------------------
def _tone(n, bps, seed, ch=1):
    """A deterministic signal of `bps` bits: a few sines plus noise, so every predictor leaves a modest residual."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None]
    amp = (1 << (bps - 1)) * 0.6
    y = sum(np.sin(t * f + rng.uniform(0, 6.28, (1, ch))) for f in (0.031, 0.11, 0.27)) / 3 * amp
    y = y + rng.randint(-(1 << max(bps - 9, 1)), 1 << max(bps - 9, 1), (n, ch))
    return np.clip(np.rint(y), -(1 << (bps - 1)), (1 << (bps - 1)) - 1).astype(np.int64)


def _fx(order, porder=0, method=0, params=None, wasted=0):
    return dict(type='fixed', order=order, porder=porder, method=method, params=params, wasted=wasted)


def _lpc(coefs, precision, shift, porder=0, method=1, params=None, wasted=0):
    return dict(type='lpc', order=len(coefs), coefs=list(coefs), precision=precision, shift=shift, porder=porder,
                method=method, params=params, wasted=wasted)


_CORPUS = None
PLANTED = 'planted_header'
STRESS = 'lpc32_stress'
REQUIRED_FORMS = (
    ['CONSTANT', 'VERBATIM', 'RICE', 'RICE2', 'K0', 'K30', 'ESCAPE0', 'ESCAPE25', 'UNARY10000', 'EMPTY_FIRST_PARTITION',
     'WASTED1', 'WASTED7', 'ASSIGNMENT8', 'ASSIGNMENT9', 'ASSIGNMENT10', 'ODD_SIDE', 'SS_CODE0', 'BS_TAIL8', 'BS_TAIL16',
     'BS_CODE1', 'BS_CODE2', 'BS_CODE8', 'BS_CODE12', 'METADATA4', 'PREC2', 'PREC15', 'SHIFT0', 'SHIFT14']
    + ['FIXED%d' % o for o in range(5)] + ['LPC%d' % o for o in (1, 2, 8, 12, 32)] + ['PORDER%d' % p for p in range(9)])


def corpus():
    """[(name, file bytes, pcm int64 [n, channels], bps)], built once; corpus_forms() the forms the writer emitted."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS[0]
    forms, items = set(), []

    def add(name, pcm, bps, frames, **kw):
        pcm = np.asarray(pcm, np.int64)
        pcm = pcm[:, None] if pcm.ndim == 1 else pcm
        items.append((name, write_stream(pcm, bps, frames, forms=forms, **kw), pcm, bps))

    one = lambda *subs, **kw: dict(subframes=list(subs), **kw)                      # noqa: E731
    # block sizes, each with the header form it forces, and a shorter last frame
    add('bs16_17', _tone(33, 16, 1), 16, [(16, one(_fx(1))), (17, one(_fx(2)))])
    add('bs192_256', _tone(192 + 256 + 100, 16, 2), 16, [(192, one(_fx(2))), (256, one(_fx(3, 2))), (100, one(_fx(1)))])
    add('bs576_1000', _tone(576 + 1000, 16, 3), 16, [(576, one(_fx(4, 1))), (1000, one(_fx(2, 3)))])
    # bps: 8, 12, 20, 24 by code, 18 through sample-size code 0
    for bps in (8, 12, 20, 24):
        add('bps%d' % bps, _tone(64, bps, 10 + bps), bps, [(64, one(_fx(2, 1, 1)))])
    add('bps18_code0', _tone(48, 18, 5), 18, [(48, one(_fx(1), ss_code=0))])
    # channels: the four assignments (odd side values under mid/side), 3 and 8 independent
    st = _tone(96, 16, 6, ch=2)
    st[::3, 0] += 1 - ((st[::3, 0] - st[::3, 1]) & 1)                              # make some sides odd
    st = np.clip(st, -32768, 32767)
    add('stereo_all', np.concatenate([st, st[::-1], st, st[::-1]]), 16,
        [(96, one(_fx(2), _fx(1))), (96, one(_fx(2), _fx(2, 1), assignment=8)),
         (96, one(_fx(1, 0, 1), _fx(2), assignment=9)), (96, one(_fx(2), _fx(0, 2), assignment=10))])
    add('ch3', _tone(40, 16, 7, ch=3), 16, [(40, one(_fx(0), _fx(1), _fx(2)))])
    add('ch8', _tone(32, 24, 8, ch=8), 24, [(32, one(*[_fx(c % 5) for c in range(8)]))])
    # subframe types
    flat = np.full(64, -1234)
    add('constant_verbatim', np.concatenate([flat, _tone(64, 16, 9)[:, 0]]), 16,
        [(64, one(dict(type='constant'))), (64, one(dict(type='verbatim')))])
    add('fixed0_4', _tone(5 * 32, 16, 11), 16, [(32, one(_fx(o))) for o in range(5)])
    rng = np.random.RandomState(12)
    add('lpc1_2', _tone(128, 16, 13), 16, [(64, one(_lpc([1], 2, 0))), (64, one(_lpc([1, -2], 2, 0, porder=1)))])
    c8 = rng.randint(-4000, 4000, 8).tolist()
    c12 = rng.randint(-16384, 16384, 12).tolist()
    add('lpc8_12', _tone(256 + 192, 16, 14), 16,
        [(256, one(_lpc(c8, 15, 14, porder=2))), (192, one(_lpc(c12, 15, 14, porder=1, method=0, params=[('esc', 25)] * 2)))])
    # order 32, alternating full-scale 24-bit samples, coefficients +-16383: the sum passes 2^40
    alt = np.where(np.arange(96) % 2 == 0, (1 << 23) - 1, -(1 << 23))
    c32 = [16383 if j % 2 == 0 else -16383 for j in range(32)]
    add(STRESS, alt, 24, [(96, one(_lpc(c32, 15, 14, params=[27])))])
    # Rice: k = 0 and 30, escapes of 0 and 25 bits, a 10 000-bit unary run
    spike = np.zeros(64, np.int64)
    spike[40] = 5000
    add('rice_k0_unary', spike, 16, [(64, one(_fx(0, 0, 0, [0])))])
    add('rice2_k30', _tone(32, 24, 15), 24, [(32, one(_fx(1, 1, 1, [30, None])))])
    ramp = np.arange(64) * 3 - 90
    full = np.where(rng.randint(0, 2, 64) == 1, (1 << 23) - 1, -(1 << 23))
    add('escape0_25', np.concatenate([ramp, full]), 24,
        [(64, one(_fx(2, 1, 0, [('esc', 0), ('esc', 0)]))), (64, one(_fx(1, 0, 1, [('esc', 25)])))])
    # partitions: orders 0..8 at 4096, order 4 at 16, a first partition of exactly 0 residuals
    big = _tone(9 * 4096, 16, 16)
    for g in range(3):
        add('porder%d_%d' % (3 * g, 3 * g + 2), big[3 * g * 4096:(3 * g + 3) * 4096], 16,
            [(4096, one(_fx(2, 3 * g + j, j & 1))) for j in range(3)])
    add('porder4_bs16', _tone(16, 16, 17), 16, [(16, one(_fx(0, 4, 1)))])
    add('empty_first_partition', _tone(16, 16, 18), 16, [(16, one(_fx(4, 2)))])
    # wasted bits: 1 and 7, the 7 on a side channel
    add('wasted1', _tone(48, 16, 19) // 2 * 2, 16, [(48, one(_fx(2, wasted=1)))])
    ws = _tone(48, 16, 20, ch=2) // 4
    ws[:, 1] = ws[:, 0] - (((ws[:, 0] - ws[:, 1]) >> 7) << 7)                      # side = left - right: 7 zero bits
    add('wasted7_side', ws, 16, [(48, one(_fx(1), _fx(1, wasted=7), assignment=8))])
    # variable block size with a sample number past 2^31 (a 7-byte number)
    add('variable_2p31', _tone(24 + 40, 16, 21), 16,
        [(24, one(_fx(1), variable=True, number=(1 << 31) + 5)), (40, one(_fx(2), variable=True, number=(1 << 31) + 29))])
    # three more metadata blocks before the frames: PADDING (holding a sync pattern), VORBIS_COMMENT, SEEKTABLE
    add('metadata4', _tone(32, 16, 22), 16, [(32, one(_fx(1)))],
        metadata=[(1, b'\xff\xf8' + bytes(30)), (4, (4).to_bytes(4, 'little') + b'test' + bytes(4)), (3, bytes(18))])
    # a VERBATIM subframe whose samples spell a complete frame header with a correct CRC-8
    fake = bytes([0xFF, 0xF8, 0xC9, 0x02, 0x00])
    fake += bytes([crc8(fake)])
    body = np.frombuffer(bytes(range(3, 8)) + fake + bytes(range(20, 25)), np.int8).astype(np.int64)
    add(PLANTED, body, 8, [(16, one(dict(type='verbatim')))])
    _CORPUS = (items, forms)
    return items


def corpus_forms():
    corpus()
    return _CORPUS[1]


def planted_offset(data):
    """Byte of the header planted inside PLANTED's payload."""
    fake = bytes([0xFF, 0xF8, 0xC9, 0x02, 0x00])
    return data.index(fake + bytes([crc8(fake)]))


def frames_start(data):
    pos = 4
    while True:
        last = data[pos] >> 7
        pos += 4 + int.from_bytes(data[pos + 1:pos + 4], 'big')
        if last:
            return pos


def damaged():
    """[(name, file bytes, kind)] -- kind: 'crc16' | 'sync' | 'metadata' | 'md5' | 'any' (any refusal)."""
    out = []
    for name, data, pcm, bps in corpus():
        f0 = frames_start(data)
        bit = ((f0 + len(data)) // 2) * 8 + 3                                      # one payload bit, mid-frames
        flipped = bytearray(data)
        flipped[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((name + ':bitflip', bytes(flipped), 'any'))
    name, data, pcm, bps = corpus()[0]                                             # bs16_17: two short frames
    f0 = frames_start(data)
    out.append((name + ':cut_header', data[:f0 + 3], 'sync'))
    out.append((name + ':cut_crc16', data[:-2], 'sync'))
    out.append((name + ':cut_metadata', data[:20], 'metadata'))
    spike = next(d for n, d, _, _ in corpus() if n == 'rice_k0_unary')
    out.append(('rice_k0_unary:cut_unary', spike[:frames_start(spike) + 6 + 200], 'sync'))
    verb = next(d for n, d, _, _ in corpus() if n == 'constant_verbatim')
    out.append(('constant_verbatim:cut_raw', verb[:-40], 'sync'))
    md5 = bytearray(data)
    md5[4 + 4 + 18] ^= 0x55                                                        # only STREAMINFO's digest
    out.append((name + ':md5', bytes(md5), 'md5'))
    x = _tone(32, 16, 30)
    bad = write_stream(x, 16, [(32, dict(subframes=[_lpc([1, 1], 3, -3)]))])
    out.append(('negative_shift', bad, 'sync'))
    x = _tone(24, 16, 31)
    spec = _fx(0, 4)
    spec['psize'] = 1                                                              # 2^4 does not divide 24
    out.append(('porder_not_dividing', write_stream(x, 16, [(24, dict(subframes=[spec]))]), 'sync'))
    # an escape of 31 raw bits declared for a 25-sample block whose bits are not there: the frame is cut after 8 samples
    x = _tone(25, 16, 32)
    esc = write_stream(x, 16, [(25, dict(subframes=[_fx(0, 0, 0, [('esc', 31)])]))])
    out.append(('escape31_overrun', esc[:frames_start(esc) + 6 + 2 + 31], 'sync'))
    return out


def reader_frame_starts(flac, path):
    """The frame starts the sequential reader amt_saga.flac.decode visits in the file at `path` (frames lie back to back
    from the first frame byte; each frame's length is what the reader hands its CRC-16 plus the two CRC bytes), and
    what it decodes: (starts, pcm, sr, bps)."""
    lens, real = [], flac._crc16

    def spy(data):
        lens.append(len(data))
        return real(data)
    flac._crc16 = spy
    try:
        pcm, sr, bps = flac.decode(path, verify=True)
    finally:
        flac._crc16 = real
    with open(path, 'rb') as f:
        at = frames_start(f.read())
    starts = []
    for n in lens:
        starts.append(at)
        at += n + 2
    return starts, pcm, sr, bps
