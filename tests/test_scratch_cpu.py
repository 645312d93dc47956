"""CPU: the scratch of the ragged calls without a GPU.  Every module has ONE layout function on the carver of
csrc/amt_scratch.h, run with a null base to count and with the buffer to carve.  tests/scratch_host_main.cpp carves
exactly the counted bytes under the address and undefined-behaviour sanitizers; here the counts are held against the
closed formulas the modules had before they shared a carver, restated below, and against the built library."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def up(v, a):
    return -(-v // a) * a


def flac_bytes(n, max_len, blocksize, bps):
    slots, bound = n * -(-max_len // blocksize), 13 + (8 + blocksize * bps + 7) // 8 + 2
    return up(slots * bound, 8) + 8 * slots


def flacdec_bytes(n_cand, slot_ints):
    return up(4 * slot_ints, 8) + 16 * n_cand


def score_bytes(n_est, n_ref):
    return 16 + 2 * 4 * up(4 * n_est, 16) + (2 + 2 * 4) * up(4 * n_ref, 16)


def png_bytes(*wh):
    """The layout as it stood: meta 32 n at 0, pieces 32 P behind it, then res (32 P), sizes (8 n), piece_off (8 P) and
    the slots, each on the next multiple of 16; a piece is max(1, 32768 // (W + 1)) rows, its slot the chunk bound
    23 + bytes, + 4, rounded up to 16."""
    n, P, slot = len(wh) // 2, 0, 0
    for w, h in zip(wh[::2], wh[1::2]):
        r = max(1, 32768 // (w + 1))
        for y in range(0, h, r):
            slot += up(23 + min(r, h - y) * (w + 1) + 4, 16)
            P += 1
    res = up(32 * n + 32 * P, 16)
    sizes = up(res + 32 * P, 16)
    piece_off = up(sizes + 8 * n, 16)
    return up(piece_off + 8 * P, 16) + slot


FORMULAS = dict(flac=flac_bytes, flacdec=flacdec_bytes, score=score_bytes, png=png_bytes)


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    """The stand-alone program's output: a sanitizer report aborts it, a broken layout ends it with a message."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path_factory.mktemp('scratch') / 'scratch_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'scratch_host_main.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr
    return r.stdout.strip().split('\n')


def cases(lines, module):
    out = []
    for line in lines:
        words = line.split()
        if words[0] == module:
            assert words[-2] == '->'
            out.append(([int(v) for v in words[1:-2]], int(words[-1])))
    return out


def test_carver_refuses_negative_and_overflowing_counts(lines):
    assert lines[0] == 'carver ok'


@pytest.mark.parametrize('module,least', [('flac', 19), ('flacdec', 12), ('score', 100), ('png', 10)])
def test_counted_bytes_equal_the_closed_formulas(lines, module, least):
    got = cases(lines, module)
    assert len(got) >= least
    for args, total in got:
        assert total == FORMULAS[module](*args), (module, args)
    if module == 'flac':                                               # both ends of both settings; every residue of 8
        assert {(16, 16), (16, 24), (4096, 16), (4096, 24)} <= {(a[2], a[3]) for a, _ in got}
        assert {(a[0] * -(-a[1] // a[2]) * (13 + (8 + a[2] * a[3] + 7) // 8 + 2)) % 8 for a, _ in got} == set(range(8))
    if module == 'png':
        assert {(1, 1), (3, 2), (16384, 1)} <= {tuple(a) for a, _ in got}


def test_counted_bytes_equal_the_library(lines):
    from amt_saga import _lib
    lib = _lib.load()
    for (n, max_len, blocksize, bps), total in cases(lines, 'flac'):
        want = total if n >= 1 and blocksize <= 4096 else _lib.AMT_E_INVALID           # the ABI wants a signal
        assert lib.amt_flac_scratch_bytes(n, max_len, blocksize, bps) == want, (n, max_len, blocksize, bps)
    for (n_cand, slot_ints), total in cases(lines, 'flacdec'):
        assert lib.amt_flac_decode_scratch_bytes(n_cand, slot_ints) == total
    for (n_est, n_ref), total in cases(lines, 'score'):
        assert lib.amt_score_scratch_bytes(n_est, n_ref) == total
    for wh, total in cases(lines, 'png'):
        meta, at = [], 3
        for w, h in zip(wh[::2], wh[1::2]):
            meta += [at, w, h]
            at += w * h
        assert lib.amt_png_scratch_bytes((ctypes.c_longlong * len(meta))(*meta), len(wh) // 2) == total, wh
