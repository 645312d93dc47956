"""WAV files on the host: the RIFF chunk walk, a numpy reader and a writer (no GPU, no library).

Stands where the reference calls librosa.load for a WAV file (audio_from_file, util_audio.py:962-964) and
librosa.output.write_wav (audio_complete.save(flac=False), util_audio.py:526-527).  read_header is also the host's
whole share of the device reader (audio.wav_decode): O(chunks) work, nothing per sample.

The value rule, shared with csrc/amt_pcm_core.h:
    integer, container c bytes (little-endian, signed; c = 1: unsigned, u - 128), valid bits b, MSB-justified:
        q = container >> (8 c - b) (arithmetic), wave = float32(q) 2^-(b-1) (nearest even), pcm = q
    float32: the 32 bits as they are (NaN payloads, -0.0);  float64: rounded to float32, nearest even
    no clipping and no normalisation on read
    writing: q = clip(rint(y 2^(b-1)), -2^(b-1), 2^(b-1) - 1) on the float32 product, NaN -> 0 (the FLAC encoder's rule)
"""
import numpy as np

MAX_CHANNELS = 8                                   # audio.Resampler.MAX_CHANNELS: what the resampler downmixes
FORMATS = ('pcm16', 'pcm24', 'float32')
FORMAT_BYTES = {'pcm16': 2, 'pcm24': 3, 'float32': 4}
MAX_DATA = (1 << 32) - 64                          # the data chunk of a file this writer makes stays below this
_TAG_NAMES = {0: 'unknown', 2: 'MS ADPCM', 6: 'A-law', 7: 'mu-law', 0x11: 'IMA ADPCM', 0x31: 'GSM 6.10', 0x55: 'MP3'}


def _u(data, pos, n):
    return int.from_bytes(data[pos:pos + n], 'little')


def read_header(data):
    """(sample rate, channels, kind 'int' | 'float', valid bits, container bytes, data offset, frames) of a WAV file's
    bytes.  Every chunk but `fmt ` and `data` is skipped by its size (odd sizes are followed by a pad byte); the data
    size is clamped to the bytes present (a declared 0 -- a streaming writer's placeholder -- stands for all that
    follow) and floored to whole frames.  Every refusal is a ValueError."""
    data = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    magic = bytes(data[:4])
    if magic == b'RIFX':
        raise ValueError('RIFX (big-endian RIFF) files are not supported')
    if magic == b'RF64':
        raise ValueError('RF64 files are not supported')
    if magic != b'RIFF':
        raise ValueError('not a WAV file')
    if len(data) < 12:
        raise ValueError('WAV file ends at byte %d, inside the RIFF header' % len(data))
    if bytes(data[8:12]) != b'WAVE':
        raise ValueError('RIFF file of form %r, not WAVE' % bytes(data[8:12]))
    pos, fmt = 12, None
    while True:
        if pos + 8 > len(data):
            raise ValueError('WAV file ends at byte %d before a data chunk' % len(data))
        cid, size = bytes(data[pos:pos + 4]), _u(data, pos + 4, 4)
        body = pos + 8
        if cid == b'data':
            break
        if cid == b'fmt ':
            if size < 16:
                raise ValueError('WAV fmt chunk of %d bytes' % size)
            if body + size > len(data):
                raise ValueError('WAV file ends at byte %d, inside the fmt chunk' % len(data))
            tag, channels, sr = _u(data, body, 2), _u(data, body + 2, 2), _u(data, body + 4, 4)
            block_align, bits = _u(data, body + 12, 2), _u(data, body + 14, 2)
            valid = bits
            if tag == 0xFFFE:                                        # WAVE_FORMAT_EXTENSIBLE
                if size < 40:
                    raise ValueError('WAV EXTENSIBLE fmt chunk of %d bytes (40 are needed)' % size)
                valid = _u(data, body + 18, 2) or bits               # wValidBitsPerSample (0: the container's)
                tag = _u(data, body + 24, 2)                         # the sub-format GUID begins with the tag
            fmt = (tag, channels, sr, block_align, valid)
        pos = body + size + (size & 1)
    if fmt is None:
        raise ValueError('WAV file without a fmt chunk before its data')
    tag, channels, sr, block_align, valid = fmt
    if tag not in (1, 3):
        raise ValueError('WAV format tag 0x%04X (%s) is not supported: integer PCM (1) and IEEE float (3) are'
                         % (tag, _TAG_NAMES.get(tag, 'a compressed codec')))
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError('WAV file of %d channels: 1 to %d are supported' % (channels, MAX_CHANNELS))
    if sr < 1:
        raise ValueError('WAV file with sample rate 0')
    if block_align == 0 or block_align % channels:
        raise ValueError('WAV block align %d does not divide into %d channels' % (block_align, channels))
    c = block_align // channels
    if tag == 1:
        kind = 'int'
        if not 1 <= c <= 4:
            raise ValueError('WAV integer samples of %d bytes: 1 to 4 are supported' % c)
        if not 1 <= valid <= 8 * c:
            raise ValueError('WAV file with %d valid bits in containers of %d' % (valid, 8 * c))
    else:
        kind = 'float'
        if c not in (4, 8):
            raise ValueError('WAV float samples of %d bytes: 4 and 8 are supported' % c)
        valid = 8 * c
    avail = len(data) - body
    if size == 0 or size > avail:
        size = avail
    frames = size // block_align
    if frames == 0:
        raise ValueError('WAV file without a whole sample frame in its data chunk')
    return sr, channels, kind, valid, c, body, frames


def containers(data, offset, values, kind, c):
    """The `values` containers at data[offset ..): int32 (sign-extended; c = 1: u - 128) or, for floats, float32 /
    float64 as stored."""
    raw = np.frombuffer(data, np.uint8, values * c, offset)
    if kind == 'float':
        return raw.view('<f4' if c == 4 else '<f8')
    if c == 1:
        return raw.astype(np.int32) - 128
    if c == 2:
        return raw.view('<i2').astype(np.int32)
    if c == 4:
        return raw.view('<i4').astype(np.int32)
    b = raw.reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return (v ^ 0x800000) - 0x800000


def to_wave(x, kind, bits):
    """The value rule: decode()'s array -> the float32 waveform."""
    if kind == 'float':
        with np.errstate(over='ignore'):                              # (a double beyond float32's range: infinity)
            return x if x.dtype == np.float32 else x.astype(np.float32)
    return x.astype(np.float32) * np.float32(2.0 ** -(bits - 1))


def decode(data):
    """(array [n, channels], sample rate, valid bits) of a WAV file's bytes: int32 q for integer files, float32 for
    float files (float64 rounded)."""
    sr, ch, kind, bits, c, off, n = read_header(data)
    x = containers(data, off, n * ch, kind, c)
    if kind == 'int':
        x = x >> (8 * c - bits)
    else:
        x = to_wave(x, kind, bits)
    return x.reshape(n, ch), sr, bits


def load_float(path):
    """flac.load_float for a WAV file: (float64 [n] for mono or [n, channels], sample rate); the values are the
    float32 waveform of the value rule, widened."""
    with open(path, 'rb') as f:
        data = f.read()
    x, sr, bits = decode(data)
    y = to_wave(x, 'int' if x.dtype == np.int32 else 'float', bits).astype(np.float64)
    return (y[:, 0] if y.shape[1] == 1 else y), sr


def is_wav(path):
    """True if the file at `path` begins with RIFF (a missing file raises FileNotFoundError)."""
    with open(path, 'rb') as f:
        return f.read(4) == b'RIFF'


# ------------------------------------------------------------------------------------
# writing
# ------------------------------------------------------------------------------------
def quantise(y, bps):
    """q = clip(rint(y 2^(bps-1)), -2^(bps-1), 2^(bps-1) - 1) on the float32 product, NaN -> 0: int32."""
    lim = 1 << (bps - 1)
    with np.errstate(over='ignore', invalid='ignore'):
        r = np.rint(np.asarray(y, np.float32) * np.float32(lim))
    r = np.where(np.isnan(r), np.float32(0), r)
    return np.clip(r, -lim, lim - 1).astype(np.int32)


def peak(y):
    """max |y| with NaNs skipped, float32; 0 for an empty or all-NaN signal."""
    a = np.abs(np.asarray(y, np.float32))
    a = a[~np.isnan(a)]
    return np.float32(a.max()) if a.size else np.float32(0)


def normalise(y):
    """y / peak(y) in float32 (librosa.output.write_wav's norm=True); a peak of 0 or a non-finite one leaves y as it
    is."""
    y = np.asarray(y, np.float32)
    p = peak(y)
    if p == 0 or not np.isfinite(p):
        return y
    with np.errstate(invalid='ignore'):
        return y / p


def header(n, sr, fmt):
    """The bytes before the samples of a mono file of n samples: 44 for the integer forms; 58 for float32 (an 18-byte
    fmt chunk and a fact chunk with the frame count)."""
    if fmt not in FORMATS:
        raise ValueError("Requested attribute does not exist: fmt must be one of %s" % (FORMATS,))
    if int(sr) != sr or not 1 <= int(sr) < 1 << 32:
        raise ValueError('WAV sample rate must be a positive integer. Got: %r' % (sr,))
    ba = FORMAT_BYTES[fmt]
    n, sr = int(n), int(sr)
    D = n * ba
    if n < 0 or D >= MAX_DATA:
        raise ValueError('WAV data of %d bytes: a file holds less than 2^32 - 64' % D)
    le = lambda v, k: int(v).to_bytes(k, 'little')                                # noqa: E731
    rate = le((sr * ba) & 0xFFFFFFFF, 4)
    if fmt == 'float32':
        return (b'RIFF' + le(50 + D, 4) + b'WAVE' + b'fmt ' + le(18, 4) + le(3, 2) + le(1, 2) + le(sr, 4) + rate
                + le(ba, 2) + le(32, 2) + le(0, 2) + b'fact' + le(4, 4) + le(n, 4) + b'data' + le(D, 4))
    return (b'RIFF' + le(36 + D + (D & 1), 4) + b'WAVE' + b'fmt ' + le(16, 4) + le(1, 2) + le(1, 2) + le(sr, 4) + rate
            + le(ba, 2) + le(8 * ba, 2) + b'data' + le(D, 4))


def sample_bytes(y, fmt):
    """The data bytes of a mono signal: integer input is taken as already quantised, float input goes through
    quantise (or, for float32, is written as it is)."""
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError('Invalid Input shape. Expected: a mono signal [n] . Got: %s' % (y.shape,))
    if fmt == 'float32':
        return np.ascontiguousarray(y, dtype='<f4').tobytes()
    bps = 8 * FORMAT_BYTES[fmt]
    q = y.astype(np.int32) if np.issubdtype(y.dtype, np.integer) else quantise(y, bps)
    if bps == 16:
        return q.astype('<i2').tobytes()
    return np.ascontiguousarray(q.astype('<i4').view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def encode(y, sr, fmt='pcm24'):
    """The bytes of a complete mono WAV file (header, samples, a zero pad byte after an odd data size)."""
    h = header(len(np.asarray(y)), sr, fmt)
    body = sample_bytes(y, fmt)
    return h + body + (b'\0' if len(body) & 1 else b'')


def save_float(wf, path, sr=44100, fmt='pcm24'):
    """flac.save_float's counterpart: the mono waveform as a WAV file of `fmt`."""
    data = encode(np.asarray(wf, dtype=np.float32), sr, fmt)
    with open(path, 'wb') as f:
        f.write(data)
