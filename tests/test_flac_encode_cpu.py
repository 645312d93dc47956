"""CPU: the numpy restatement of the device FLAC encoder's format rule (tests/flac_encode_reference.py) through the
product's reader, the coverage of the committed input set, the frame-number coding of the restatement and of the host
writer, the host-side checks of the two ABI entries and the --flac switch."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_encode_reference as R                               # noqa: E402


def _host_frame_bytes(bs, bps, number):
    """Size of the host writer's (VERBATIM) frame for a block."""
    return 4 + len(R.utf8_num(number)) + 2 + 1 + (8 + bs * bps + 7) // 8 + 2


@pytest.fixture(scope='module')
def committed():
    """bps -> name -> (file bytes, choices) of the committed input set at block size 4096, computed once."""
    sig = R.signals()
    return {bps: {name: R.encode_file(y, 44100, bps, 4096) for name, y in sig.items()} for bps in (24, 16)}


@pytest.mark.parametrize('bps', [16, 24])
@pytest.mark.parametrize('blocksize', [16, 192, 4096])
def test_restatement_decodes_through_the_reader(tmp_path, bps, blocksize):
    """Every length of (0, 1, 3, 5, bs - 1, bs, bs + 1, 2 bs + 37) of a tone with noise: CRC-8, CRC-16 and
    MD5 verify and the samples are the quantised ones; no frame is longer than the host writer's."""
    from amt_saga import flac
    y = R.signals(2 * 4096 + 37)['tone_noise']
    for n in (0, 1, 3, 5, blocksize - 1, blocksize, blocksize + 1, 2 * blocksize + 37):
        data, choices = R.encode_file(y[:n], 44100, bps, blocksize)
        path = str(tmp_path / 'r.flac')
        open(path, 'wb').write(data)
        pcm, sr, b = flac.decode(path, verify=True)
        assert (sr, b) == (44100, bps) and np.array_equal(pcm.reshape(-1), R.quantise(y[:n], bps)), n
        assert len(choices) == -(-n // blocksize)
        if n == 0:
            assert len(data) == 42
        if n == 1:
            assert choices[0][0] == 'CONSTANT'
        frames, _ = R.encode_frames(R.quantise(y[:n], bps), bps, blocksize)
        for i, fr in enumerate(frames):
            assert len(fr) <= _host_frame_bytes(min(blocksize, n - i * blocksize), bps, i), (n, i)


@pytest.mark.parametrize('bps', [16, 24])
def test_committed_set_decodes(committed, tmp_path, bps):
    from amt_saga import flac
    sig = R.signals()
    for name, (data, choices) in committed[bps].items():
        path = str(tmp_path / (name + '.flac'))
        open(path, 'wb').write(data)
        pcm = flac.decode(path, verify=True)[0]
        assert np.array_equal(pcm[:, 0], R.quantise(sig[name], bps)), name
        host = 42 + sum(_host_frame_bytes(min(4096, len(sig[name]) - s), bps, i)
                        for i, s in enumerate(range(0, len(sig[name]), 4096)))
        assert len(data) <= host, name


def test_committed_set_covers_the_rule(committed):
    """The choices over the committed inputs include every branch a kernel could get wrong."""
    choices = [c for bps in committed for data, ch in committed[bps].values() for c in ch]
    kinds = {c[0] for c in choices}
    assert {'CONSTANT', 'VERBATIM', 'FIXED'} <= kinds
    fixed = [c for c in choices if c[0] == 'FIXED']
    assert {c[1] for c in fixed} == {0, 1, 2, 3, 4}
    ps = {c[2] for c in fixed}
    assert 0 in ps and any(p >= 3 for p in ps) and 7 in ps
    ks = {k for c in fixed for k in c[3]}
    assert len(ks) >= 6 and 0 in ks and any(k >= 16 for k in ks)
    assert any(c[4] > 0 for c in fixed)                            # a tie the smallest-k rule decided
    c24 = {name: ch for name, (data, ch) in committed[24].items()}
    assert c24['impulse'][0][:3] == ('FIXED', 0, 7)
    assert all(c[0] == 'CONSTANT' for c in c24['zeros'] + c24['dc'])
    assert all(c[0] == 'VERBATIM' for c in c24['noise_full'])
    assert c24['walk'][0][1] == 1 and c24['walk3'][0][1] == 3 and c24['tone'][0][1] == 4
    assert c24['loud_quiet'][0][2] > 0
    assert R.encode_frames(R.quantise(np.float32([0.1, -0.2, 0.3]), 24))[1][0][0] == 'VERBATIM'     # three samples


def test_smallest_k_decides_a_tie():
    """One residual u = 2 at order 0: k = 0 costs 5 + 1 + 2, k = 1 costs 5 + 2 + 1 -- equal, and k = 0 is taken."""
    cost, k, table = R.partition_costs(np.array([2], dtype=np.int64))
    assert (cost, k) == (8, 0) and table[1] == 8


def test_frame_number_coding():
    from amt_saga import flac
    for v in (0, 127, 128, 2047, 2048, 65535, 65536, 0x10FFFF):
        assert R.utf8_num(v) == chr(v).encode('utf-8', 'surrogatepass'), v
        assert flac._utf8_num(v) == R.utf8_num(v), v               # 128 and 2047 fail before the lead-byte fix
    for v, nb in ((1 << 21, 5), (1 << 26, 6), ((1 << 31) - 1, 6)):
        b = R.utf8_num(v)
        assert len(b) == nb
        lead_ones = 0
        while b[0] & (0x80 >> lead_ones):
            lead_ones += 1
        assert lead_ones == nb and all(c >> 6 == 2 for c in b[1:])
        val = b[0] & (0x7F >> nb)
        for c in b[1:]:
            val = (val << 6) | (c & 0x3F)
        assert val == v
        assert flac._utf8_num(v) == b


def test_host_writer_past_128_frames(tmp_path):
    """130 blocks at block size 16: frame 128 is the first with a two-byte number.  Fails before the lead-byte fix
    (FLAC frame header CRC-8 mismatch)."""
    from amt_saga import flac
    pcm = (np.arange(130 * 16) % 97 - 40).astype(np.int64)
    path = str(tmp_path / 'long.flac')
    flac.encode(pcm, path, blocksize=16)
    got, sr, bps = flac.decode(path, verify=True)
    assert np.array_equal(got[:, 0], pcm)


def test_abi_host_checks():
    from amt_saga import _lib
    lib = _lib.load()
    assert lib.amt_flac_frame_bound(4096, 24) == 13 + 12289 + 2
    assert lib.amt_flac_frame_bound(16, 16) == 13 + 33 + 2
    for bs, bps in ((15, 24), (4097, 24), (4096, 8), (4096, 20), (0, 16)):
        assert lib.amt_flac_frame_bound(bs, bps) < 0, (bs, bps)
    assert lib.amt_flac_scratch_bytes(3, 8229, 4096, 24) == 3 * 3 * 12304 + 8 * 9
    assert lib.amt_flac_scratch_bytes(1, 10, 16, 16) == 48 + 8
    assert lib.amt_flac_scratch_bytes(0, 10, 16, 16) < 0 and lib.amt_flac_scratch_bytes(1, 10, 16, 12) < 0
    p = ctypes.c_void_p(8)                                         # never dereferenced: the checks come first
    big = 1 << 40

    def call(wave=p, base=p, length=p, n=1, max_len=100, bs=16, bps=24, ff=0, scratch=p, sb=big, out=p, ob=big, fb=p,
             so=p, mm=p, md5=p):
        return lib.amt_flac_encode_ragged(wave, base, length, n, max_len, bs, bps, ff, scratch, sb, out, ob, fb, so, mm,
                                          md5, None)
    for name in ('wave', 'base', 'length', 'scratch', 'out', 'fb', 'so', 'mm', 'md5'):
        assert call(**{name: None}) == _lib.AMT_E_INVALID, name
    assert call(n=0) == _lib.AMT_E_INVALID
    assert call(bps=20) == _lib.AMT_E_INVALID and call(bs=15) == _lib.AMT_E_INVALID and call(bs=4097) == _lib.AMT_E_INVALID
    assert call(ff=-1) == _lib.AMT_E_INVALID
    assert call(ff=(1 << 31) - 7) == _lib.AMT_E_INVALID            # 100 samples = 7 frames: the last would be 2^31 - 1 + ...
    need = lib.amt_flac_scratch_bytes(1, 100, 16, 24)
    assert call(sb=need - 1) == _lib.AMT_E_SHAPE
    assert call(ob=7 * lib.amt_flac_frame_bound(16, 24) - 1) == _lib.AMT_E_SHAPE


def test_flac_switch_parsing(tmp_path):
    """--flac takes host or device in both modes and refuses anything else before any work starts."""
    from amt_saga import transcribe as tr
    assert tr.FLAC_WRITERS == ('host', 'device')
    for argv in (['in.flac', 'out.mid', '--flac', 'gpu'],
                 ['--songs', 'a.flac', '--out-dir', str(tmp_path), '--flac', 'gpu']):
        with pytest.raises(SystemExit):
            tr.main(argv)
    with pytest.raises(ValueError):
        tr.write_song_audio(44100, residual=np.zeros(4), residual_path=str(tmp_path / 'x.flac'), flac='gpu')
    assert not os.path.exists(str(tmp_path / 'x.flac'))
