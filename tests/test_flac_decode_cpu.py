"""CPU: the host side of the device FLAC decoder.  The test writer is pinned to the sequential reader; frame_candidates
holds every frame the reader visits; the decoder core the kernels compile (csrc/amt_flacdec_core.h) reproduces every PCM
bit and refuses every damaged stream in a stand-alone program built with the address and undefined-behaviour
sanitizers; the ABI, the Python entry points and --decode refuse bad arguments before a GPU is touched."""
import ctypes
import glob
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import flac_stream_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'flac', '*.flac')))


@pytest.fixture(scope='module')
def streams(tmp_path_factory):
    """[(name, path, data, pcm, bps, reader's frame starts)] for the corpus and the recorded files, decoded once."""
    from amt_saga import flac
    d = tmp_path_factory.mktemp('flac_corpus')
    out = []
    for name, data, pcm, bps in W.corpus():
        path = str(d / (name + '.flac'))
        with open(path, 'wb') as f:
            f.write(data)
        starts, got, sr, gbps = W.reader_frame_starts(flac, path)
        assert gbps == bps and sr == 44100, name
        assert got.shape == pcm.shape and np.array_equal(got, pcm), name          # the writer pinned to the reader
        out.append((name, path, data, pcm, bps, starts))
    for path in GOLDEN:
        data = open(path, 'rb').read()
        starts, got, sr, gbps = W.reader_frame_starts(flac, path)
        out.append((os.path.basename(path), path, data, got, gbps, starts))
    return out


def test_writer_streams_decode_through_the_reader_and_reach_every_form(streams):
    assert len(GOLDEN) == 4
    forms = W.corpus_forms()
    assert not set(W.REQUIRED_FORMS) - forms, sorted(set(W.REQUIRED_FORMS) - forms)
    assert 32 * 16383 * ((1 << 23) - 1) > 1 << 40                                  # the stress stream's prediction sum
    names = [s[0] for s in streams]
    assert W.STRESS in names and W.PLANTED in names
    assert all(1 <= len(s[5]) <= 5 for s in streams[:len(W.corpus())])             # the writer's streams stay small


def test_candidates_hold_every_frame_the_reader_visits(streams):
    from amt_saga import flac
    for name, path, data, pcm, bps, starts in streams:
        sr, ch, sbps, total, md5, first = flac.read_streaminfo(data)
        assert (ch, sbps, total) == (pcm.shape[1], bps, pcm.shape[0]), name
        assert first == W.frames_start(data) == starts[0], name
        pos, hdr, bs, ca, fb = flac.frame_candidates(data, first)
        assert pos.dtype == np.int64 and np.all(np.diff(pos) > 0)
        assert set(starts) <= set(pos.tolist()), name
        on = np.isin(pos, starts)
        assert int(bs[on].sum()) >= total > int(bs[on].sum()) - int(bs[on][-1]), name
        assert set(fb[on].tolist()) <= {0, bps}, name
        if name == W.PLANTED:
            fake = W.planted_offset(data)
            assert fake in pos.tolist() and fake not in starts
            assert int(bs[pos.tolist().index(fake)]) == 4096
    with pytest.raises(ValueError, match='not a FLAC file'):
        flac.read_streaminfo(b'RIFF' + bytes(40))
    with pytest.raises(ValueError, match='metadata ends'):
        flac.read_streaminfo(W.corpus()[0][1][:20])


def _corpus_file(path, entries):
    """entries: [(expect, data, pcm or None)]; see tests/flacdec_host_main.cpp for the layout."""
    from amt_saga import flac
    with open(path, 'wb') as f:
        f.write(b'FDC1' + struct.pack('<i', len(entries)))
        for expect, data, pcm in entries:
            sr, ch, bps, total, md5, first = flac.read_streaminfo(data)
            pos, hdr, bs, ca, fb = flac.frame_candidates(data, first)
            f.write(struct.pack('<iiiqqq', min(expect, 1), ch, bps, total, first, len(data)) + data)
            f.write(struct.pack('<i', len(pos)))
            for i in range(len(pos)):
                f.write(struct.pack('<qiiii', int(pos[i]), 0 if expect == 2 else int(hdr[i]), int(bs[i]), int(ca[i]),
                                    int(fb[i]) or bps))
            if expect == 0:
                assert pcm.shape == (total, ch)
                f.write(np.ascontiguousarray(pcm, dtype='<i4').tobytes())


def test_core_in_a_sanitised_stand_alone_program(streams, tmp_path):
    """amt_flacdec_core.h, host only, under the address and undefined-behaviour sanitizers: every stream bit for bit, every damaged stream
    refused, no sanitizer report (a report aborts the program: a nonzero exit)."""
    from amt_saga import flac
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'flacdec_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'flacdec_host_main.cpp'), '-o', exe], check=True)
    good = str(tmp_path / 'good.bin')
    _corpus_file(good, [(0, data, pcm) for _, _, data, pcm, _, _ in streams])
    r = subprocess.run([exe, good], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('-> ok') == len(streams)
    entries, n_meta = [], 0
    for name, data, kind in W.damaged():
        if kind == 'md5':
            continue                                                               # (the digest is the kernels' to check)
        if kind == 'metadata':
            with pytest.raises(ValueError, match='metadata ends'):
                flac.read_streaminfo(data)
            n_meta += 1
            continue
        entries.append((1, data, None))
    assert n_meta == 1 and len(entries) >= len(W.corpus()) + 7
    # a frame of 28 bits per sample (Python refuses such a file first: here the core's own refusal is reached), and a
    # candidate row that is out of range (header length 0), which the walk reports as a table error
    deep = W.write_stream(np.arange(-8, 8, dtype=np.int64) << 20, 28, [(16, dict(subframes=[dict(type='verbatim')]))])
    entries.append((1, deep, None))
    entries.append((2, W.corpus()[0][1], None))
    bad = str(tmp_path / 'bad.bin')
    _corpus_file(bad, entries)
    r = subprocess.run([exe, bad], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('-> ok') == len(entries) and 'runtime error' not in r.stderr
    lines = r.stdout.strip().splitlines()
    assert 'status %d ' % 2 in lines[-2] and 'frame_err 4 ' in lines[-2], lines[-2]  # FD_S_FRAME, FD_E_UNSUPPORTED
    assert 'status 5 ' in lines[-1] and 'frame_err 5 ' in lines[-1], lines[-1]      # FD_S_TABLE, FD_E_TABLE


def test_abi_refuses_bad_arguments_before_any_hip_call():
    from amt_saga import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                                        # never dereferenced: checks come first
    assert lib.amt_flac_decode_scratch_bytes(3, 100) == 400 + 48
    assert lib.amt_flac_decode_scratch_bytes(3, 101) == 408 + 48
    assert lib.amt_flac_decode_scratch_bytes(-1, 0) == _lib.AMT_E_INVALID
    assert lib.amt_flac_decode_scratch_bytes(0, -1) == _lib.AMT_E_INVALID

    def call(**kw):
        a = dict(data=p, data_bytes=10, sm=p, n=1, cm=p, n_cand=1, md5=p, verify=2, scratch=p, scratch_bytes=1 << 20,
                 slot_ints=16, out=p, pcm=None, out_values=16, status=p, cand_out=p, md5_out=p)
        a.update(kw)
        return lib.amt_flac_decode_ragged(a['data'], a['data_bytes'], a['sm'], a['n'], a['cm'], a['n_cand'], a['md5'],
                                          a['verify'], a['scratch'], a['scratch_bytes'], a['slot_ints'], a['out'],
                                          a['pcm'], a['out_values'], a['status'], a['cand_out'], a['md5_out'], None)
    for k in ('data', 'sm', 'cm', 'md5', 'scratch', 'out', 'status', 'cand_out', 'md5_out'):
        assert call(**{k: None}) == _lib.AMT_E_INVALID, k
    for kw in (dict(n=0), dict(n_cand=-1), dict(data_bytes=-1), dict(slot_ints=-1), dict(out_values=-1), dict(verify=3),
               dict(verify=-1)):
        assert call(**kw) == _lib.AMT_E_INVALID, kw
    assert call(scratch_bytes=16 * 4 + 16 - 1) == _lib.AMT_E_SHAPE


def test_python_refuses_bad_arguments_before_the_gpu(tmp_path):
    from amt_saga import audio
    good = W.corpus()[0][1]
    with pytest.raises(ValueError, match='a list of bytes'):
        audio.flac_decode(good)
    with pytest.raises(ValueError, match='a list of bytes'):
        audio.flac_decode(['name.flac'])
    with pytest.raises(ValueError, match='at least one file'):
        audio.flac_decode([])
    for v in (2, 1, 0, 'md5', None, ['crc']):
        with pytest.raises(ValueError, match='verify'):
            audio.flac_decode([good], verify=v)
    with pytest.raises(ValueError, match='not a FLAC file'):
        audio.flac_decode([good, b'OggS' + bytes(100)])
    with pytest.raises(ValueError, match='metadata ends'):
        audio.flac_decode([good[:20]])
    x = np.arange(-8, 8, dtype=np.int64) << 20
    deep = W.write_stream(x, 28, [(16, dict(subframes=[dict(type='verbatim')]))])
    with pytest.raises(ValueError, match='above 24 is not supported'):
        audio.flac_decode([good, deep])
    with pytest.raises(FileNotFoundError):
        audio.load_flac([str(tmp_path / 'missing.flac')])
    # a small file of nothing but valid headers that declare 65536-sample blocks: refused, not given scratch
    h = bytes([0xFF, 0xF8, 0x70, 0x08, 0x00, 0xFF, 0xFF])
    h += bytes([W.crc8(h)])
    greedy = good[:W.frames_start(good)] + h * 2000
    with pytest.raises(ValueError, match='candidate frame headers declare'):
        audio.flac_decode([good, greedy])


def test_decode_option_parses_in_both_modes(tmp_path, capsys):
    from amt_saga import transcribe as tr
    assert tr.DECODERS == ('host', 'device')
    missing = str(tmp_path / 'missing.flac')
    for mode in tr.DECODERS:                                                       # accepted: the file is what fails
        with pytest.raises(FileNotFoundError):
            tr.main([missing, str(tmp_path / 'o.mid'), '--decode', mode])
        with pytest.raises(FileNotFoundError):
            tr.main(['--songs', missing, '--out-dir', str(tmp_path / 'o'), '--decode', mode])
    for argv in ([missing, str(tmp_path / 'o.mid'), '--decode', 'gpu'],
                 ['--songs', missing, '--out-dir', str(tmp_path / 'o'), '--decode', 'gpu']):
        with pytest.raises(SystemExit):
            tr.main(argv)
    assert 'invalid choice' in capsys.readouterr().err
