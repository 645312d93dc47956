"""CPU: the numpy restatement of the FLAC encoder's rule with linear prediction (tests/flac_lpc_reference.py) through
the product's reader, frame by frame against the fixed rule, the coverage of the input set, the analysis of
csrc/amt_flac_lpc_core.h in a stand-alone program built with the address and undefined-behaviour sanitizers, the host-side
checks of amt_flac_encode_lpc_ragged and the --flac-predictor switch."""
import ctypes
import glob
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_encode_reference as R                               # noqa: E402
import flac_lpc_reference as L                                  # noqa: E402

RECORDINGS = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'flac', '*.flac')))
SMALLER = ['sw_10_29', 'sw_6_26', 'sw_8_39', 'sw_8_85', 'tone', 'tone_noise', 'ramp']      # at 24 bit


def _frame_bytes(bits, bs, number):
    """Size of a frame whose subframe has `bits` bits."""
    return 4 + len(R.utf8_num(number)) + 2 + 1 + (bits + 7) // 8 + 2


@pytest.fixture(scope='module')
def inputs():
    """(name, bps) -> quantised samples: the 14 committed signals and the additions at 24 and 16 bit, the four
    recordings (24 bit) as they decode."""
    from amt_saga import flac
    sig = dict(R.signals())
    sig.update(L.more_signals())
    out = {(name, bps): R.quantise(y, bps) for name, y in sig.items() for bps in (24, 16)}
    assert len(RECORDINGS) == 4
    for path in RECORDINGS:
        pcm, sr, bps = flac.decode(path, verify=True)
        assert bps == 24 and pcm.shape[1] == 1
        out[(os.path.basename(path)[:-5], 24)] = pcm[:, 0].astype(np.int64)
    return out


@pytest.fixture(scope='module')
def encoded(inputs):
    """(name, bps) -> (frames, choices) of the LPC rule at block size 4096 and order 12, computed once."""
    return {key: L.encode_frames(q, key[1], 4096) for key, q in inputs.items()}


def test_partition_search_is_the_fixed_rules(inputs):
    """The all-partitions-at-once search equals flac_encode_reference's partition by partition: the FIXED choice found
    through it is choose()'s, bits, p and k_j; the residual coding written here gives subframe_bits' bits."""
    for key in (('tone_noise', 24), ('loud_quiet', 16), ('walk3', 24), ('impulse', 24)):
        q = inputs[key][:4096]
        kind, o, p, ks, bits, _ = R.choose(q, key[1])
        assert kind == 'FIXED'
        best = None
        for oo in range(5):
            total, pp, kk, _ = L.partition_search(R.zigzag(R.residual(q, oo)), oo, len(q))
            total += 8 + oo * key[1] + 6
            if best is None or total < best[0]:
                best = (total, oo, pp, kk)
        assert best == (bits, o, p, ks), key
        tail = L.rice_bits(R.zigzag(R.residual(q, o)), o, len(q), p, ks)
        assert np.array_equal(R.subframe_bits(q, key[1], kind, o, p, ks)[8 + o * key[1] + 6:], tail), key


@pytest.mark.parametrize('bps', [16, 24])
@pytest.mark.parametrize('blocksize', [16, 192, 4096])
def test_restatement_decodes_through_the_reader(tmp_path, bps, blocksize):
    """Lengths 0, 1, 3, 5, 13, bs - 1, bs, bs + 1, 2 bs + 37 of a tone with noise at lpc_order 4 and 12 and of a
    two-sample oscillation at lpc_order 1: CRC-8, CRC-16 and MD5 verify, the samples are the quantised ones, and LPC
    subframes are among the frames."""
    from amt_saga import flac
    kinds = set()
    # (16-sample blocks are too short for the tone to pay for coefficients; the two-sample oscillation does at order 1)
    for order, y in ((1, L.more_signals(2 * 4096 + 37)['alternating']), (4, R.signals(2 * 4096 + 37)['tone_noise']),
                     (12, R.signals(2 * 4096 + 37)['tone_noise'])):
        for n in (0, 1, 3, 5, 13, blocksize - 1, blocksize, blocksize + 1, 2 * blocksize + 37):
            data, choices = L.encode_file(y[:n], 44100, bps, blocksize, lpc_order=order)
            path = str(tmp_path / 'r.flac')
            open(path, 'wb').write(data)
            pcm, sr, b = flac.decode(path, verify=True)
            assert (sr, b) == (44100, bps) and np.array_equal(pcm.reshape(-1), R.quantise(y[:n], bps)), (order, n)
            assert len(choices) == -(-n // blocksize)
            assert all(c[1] <= order for c in choices if c[0] == 'LPC')
            kinds |= {c[0] for c in choices}
            if n == 0:
                assert len(data) == 42
    assert 'LPC' in kinds, kinds


def test_no_frame_longer_than_the_fixed_rules(inputs, encoded):
    """Frame by frame: an LPC-rule frame is never longer than the fixed rule's for the same block (its size from the
    fixed rule's bit count), and where every LPC candidate loses the bytes are the fixed rule's."""
    same = 0
    for key, (frames, choices) in encoded.items():
        q, bps = inputs[key], key[1]
        for i, (fr, ch) in enumerate(zip(frames, choices)):
            blk = q[i * 4096:(i + 1) * 4096]
            if ch[0] == 'CONSTANT':
                continue
            assert len(fr) <= _frame_bytes(ch[4]['fixed_bits'], len(blk), i), (key, i)
            if ch[0] != 'LPC' and key[0] in ('noise_full', 'square', 'walk', 'impulse', 'tone', 'sw_8_39', 'slow_sine'):
                assert fr == R.encode_frame(blk, bps, i)[0], (key, i)
                same += 1
    assert same >= 10
    # lpc_order given, no candidate better: full-scale noise stays VERBATIM, a square wave FIXED, byte for byte
    for name in ('noise_full', 'square'):
        q = inputs[(name, 24)][:4096]
        for order in (1, 5):
            assert L.encode_frame(q, 24, 3, order)[0] == R.encode_frame(q, 24, 3)[0]


def test_input_set_covers_the_rule(inputs, encoded):
    """The choices over the inputs include every branch a kernel could get wrong."""
    choices = [c for frames, ch in encoded.values() for c in ch]
    assert {'CONSTANT', 'VERBATIM', 'FIXED', 'LPC'} <= {c[0] for c in choices}
    lpc = [c for c in choices if c[0] == 'LPC']
    orders = {c[1] for c in lpc}
    assert 1 in orders and 12 in orders and len(orders & set(range(2, 12))) >= 3, orders
    shifts = {c[4]['shift'] for c in lpc}
    assert len(shifts) >= 3, shifts
    coefs = [v for c in lpc for v in c[4]['coef']]
    assert min(coefs) < 0 < max(coefs)
    assert any(c[2] > 0 for c in lpc) and any(c[2] == 0 for c in lpc)          # partition orders
    print('orders', sorted(orders), 'shifts', sorted(shifts))
    # A coefficient at a clamp: the analysis reaches both clamps in orders that lose (walks and the slow sine at order 1:
    # 2^(P-1) - 1; the two-sample oscillation: -2^(P-1)), which test_core_in_a_sanitised_stand_alone_program compares; at
    # lpc_order 1 the oscillation's subframe carries one.
    kind, m, p, ks, bits, extra = L.choose(inputs[('alternating', 24)][:4096], 24, 1)
    assert (kind, m, extra['shift'], extra['coef']) == ('LPC', 1, 13, [-8192])
    # A tie between a FIXED and an LPC bit count, decided for FIXED: the set has none, and no order is disqualified in
    # it; test_tie_is_decided_for_fixed makes a tie, the host program's hand-made residuals the disqualification.
    assert not any(c[4]['tie_with_fixed'] or c[4]['disqualified'] for c in choices if c[4])


def test_tie_is_decided_for_fixed(monkeypatch):
    """Equal bit counts: FIXED is kept.  The LPC candidates' head is made cheaper until order 1 of a walk costs exactly
    the FIXED winner's bits; one bit less and LPC wins."""
    q = R.quantise(R.signals()['walk'], 24)[:192]
    kind, o, p, ks, bits, extra = L.choose(q, 24, 1)
    assert kind == 'FIXED'
    shift, c = L.analyse(q, 24, 1)[0]
    total = L.partition_search(R.zigzag(L.lpc_residual(q, c, shift)), 1, len(q))[0]
    head = L.lpc_bits
    monkeypatch.setattr(L, 'lpc_bits', lambda m, bps: bits - total)
    assert L.choose(q, 24, 1)[0] == 'FIXED' and L.choose(q, 24, 1)[5]['tie_with_fixed']
    monkeypatch.setattr(L, 'lpc_bits', lambda m, bps: bits - total - 1)
    assert L.choose(q, 24, 1)[0] == 'LPC'
    monkeypatch.setattr(L, 'lpc_bits', head)


def test_lpc_streams_are_smaller(inputs, encoded):
    """On the four recordings and on tone, tone_noise and ramp the LPC stream is strictly smaller than the fixed one."""
    for name in SMALLER:
        q = inputs[(name, 24)]
        frames, choices = encoded[(name, 24)]
        fixed = sum(_frame_bytes(c[4]['fixed_bits'], 0, i) for i, c in enumerate(choices))
        assert all(c[0] != 'CONSTANT' for c in choices)
        lpc = sum(len(f) for f in frames)
        print('%s: lpc %d bytes, fixed %d (%.3f)' % (name, lpc, fixed, lpc / fixed))
        assert lpc < fixed, name
    q = inputs[('sw_6_26', 24)]
    assert sum(len(f) for f in R.encode_frames(q, 24, 4096)[0]) == \
        sum(_frame_bytes(c[4]['fixed_bits'], 0, i) for i, c in enumerate(encoded[('sw_6_26', 24)][1]))


def _records(inputs):
    """(record bytes, expected output lines) of every block of every input at block size 4096 and order 12, and of
    smaller blocks and orders."""
    recs, want = [], []

    def analysis(q, bps, order):
        q = np.asarray(q, dtype=np.int64)
        recs.append(struct.pack('<4i', 0, bps, order, len(q)) + q.astype('<i4').tobytes())
        want.append('R ' + ' '.join(str(v) for v in L.autocorrelation(q)))
        for m, qc in enumerate(L.analyse(q, bps, min(order, len(q) - 1)), 1):
            want.append('%d -' % m if qc is None else '%d %d %s' % (m, qc[0], ' '.join(str(v) for v in qc[1])))

    for (name, bps), q in inputs.items():
        for s0 in range(0, len(q), 4096):
            analysis(q[s0:s0 + 4096], bps, 12)
    for key in (('tone_noise', 24), ('harmonics', 16), ('alternating', 24), ('zeros', 24), ('ramp', 24)):
        q = inputs[key]
        for bs, order in ((16, 12), (192, 5), (13, 12), (5, 12), (3, 1), (1, 12), (2, 12)):
            analysis(q[1000:1000 + bs], key[1], order)

    def resid(q, c, shift):
        q = np.asarray(q, dtype=np.int64)
        recs.append(struct.pack('<2i', 1, len(q)) + q.astype('<i4').tobytes()
                    + struct.pack('<%di' % (2 + len(c)), len(c), shift, *c))
        r = L.lpc_residual(q, c, shift)
        want.append('resid %d %d %d' % (r.min(), r.max(), int(not np.any(np.abs(r) >= L.RESID_LIMIT))))

    top = (1 << 23) - 1
    resid([top, 15, top, 15], [-16], 0)                         # r = q_i + 16 q_(i-1): at most 2^27 - 1, a candidate
    resid([top, 16, top, 15], [-16], 0)                         # 2^27: disqualified
    resid([-top - 1, 0, 3, 4], [16], 0)                         # 2^27 again, from the most negative sample
    resid([-top - 1, 1, 3, 4], [16], 0)                         # 2^27 + 1
    resid([top] * 40, [-8192] * 12, 0)                          # 12 coefficients at the 14-bit clamp: sums of 2^39.6
    resid([-top - 1] * 40, [8191] * 12, 2)                      # the same through a shift: 2^37.6
    resid(inputs[('tone', 24)][:300], [5000, -3000, 700], 12)   # an ordinary predictor
    return recs, want


def test_core_in_a_sanitised_stand_alone_program(inputs, tmp_path):
    """amt_flac_lpc_core.h on the host, -O2 -ffp-contract=off with the address and undefined-behaviour sanitizers: the
    autocorrelation, every order's shift and coefficients and the hand-made residual checks equal the restatement's,
    value for value; a sanitizer report aborts the program (a nonzero exit)."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'flac_lpc_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O2', '-g', '-ffp-contract=off', '-Xarch_host',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'flac_lpc_host_main.cpp'), '-o', exe], check=True)
    recs, want = _records(inputs)
    path = str(tmp_path / 'blocks.bin')
    with open(path, 'wb') as f:
        f.write(b'FLP1' + struct.pack('<i', len(recs)) + b''.join(recs))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'Sanitizer' not in r.stderr, r.stderr[-3000:]
    got = r.stdout.strip().splitlines()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert [w.rsplit(' ', 1)[1] for w in want if w.startswith('resid')] == ['1', '0', '0', '0', '0', '0', '1']
    values = {int(v) for w in want if w[0].isdigit() and not w.endswith('-') for v in w.split()[2:]}
    assert {-8192, 8191, -2048, 2047} <= values                    # both clamps of both precisions were compared
    assert any(w.endswith(' -') for w in want)                     # and orders without a candidate


def test_abi_host_checks():
    from amt_saga import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(8)                                         # never dereferenced: the checks come first
    big = 1 << 40

    def call(wave=p, base=p, length=p, n=1, max_len=100, bs=16, bps=24, ff=0, order=12, scratch=p, sb=big, out=p,
             ob=big, fb=p, so=p, mm=p, md5=p):
        return lib.amt_flac_encode_lpc_ragged(wave, base, length, n, max_len, bs, bps, ff, order, scratch, sb, out, ob,
                                              fb, so, mm, md5, None)
    for name in ('wave', 'base', 'length', 'scratch', 'out', 'fb', 'so', 'mm', 'md5'):
        assert call(**{name: None}) == _lib.AMT_E_INVALID, name
    for order in (0, 13, -1, 1 << 20):
        assert call(order=order) == _lib.AMT_E_INVALID, order
    assert call(n=0) == _lib.AMT_E_INVALID and call(n=65536) == _lib.AMT_E_UNSUPPORTED
    assert call(bps=20) == _lib.AMT_E_INVALID and call(bs=15) == _lib.AMT_E_INVALID and call(bs=4097) == _lib.AMT_E_INVALID
    assert call(ff=-1) == _lib.AMT_E_INVALID and call(ff=(1 << 31) - 7) == _lib.AMT_E_INVALID
    assert call(max_len=-1) == _lib.AMT_E_INVALID
    need = lib.amt_flac_scratch_bytes(1, 100, 16, 24)
    assert call(sb=need - 1) == _lib.AMT_E_SHAPE
    assert call(ob=7 * lib.amt_flac_frame_bound(16, 24) - 1) == _lib.AMT_E_SHAPE
    assert lib.amt_flac_scratch_bytes(3, 8229, 4096, 24) == 3 * 3 * 12304 + 8 * 9      # the layout is the fixed entry's
    header = open(os.path.join(ROOT, 'include', 'amt_saga.h')).read()
    assert 'int amt_flac_encode_lpc_ragged(' in header and 'amt_flac_encode_lpc_ragged' in _lib.PROTOTYPES


def test_python_arguments_are_checked_before_any_device_work():
    """predictor / lpc_order outside their sets: ValueError, raised before the signals are looked at (a host array would
    otherwise be refused as 'not a device tensor')."""
    from amt_saga import audio
    host = np.zeros(8, np.float32)
    for kw in (dict(predictor='welch'), dict(predictor=None), dict(predictor='lpc', lpc_order=0),
               dict(predictor='lpc', lpc_order=13), dict(predictor='fixed', lpc_order=13),
               dict(predictor='lpc', lpc_order=4.0), dict(predictor='lpc', lpc_order=True)):
        for fn in (lambda **k: audio.flac_encode_streams([host], **k), lambda **k: audio.flac_encode([host], 44100, **k),
                   lambda **k: audio.save_flac([host], ['never.flac'], 44100, **k)):
            with pytest.raises(ValueError, match='predictor|lpc_order'):
                fn(**kw)
    assert not os.path.exists('never.flac')
    assert audio.FLAC_PREDICTORS == ('fixed', 'lpc')


def test_flac_predictor_switch_parsing(tmp_path):
    """--flac-predictor takes fixed or lpc in both modes, refuses anything else, and refuses lpc with the host writer
    before any work starts: no input file exists here, and no output directory is made."""
    from amt_saga import transcribe as tr
    out = str(tmp_path / 'never')
    for argv in (['in.flac', 'out.mid', '--flac-predictor', 'welch'],
                 ['--songs', 'a.flac', '--out-dir', out, '--flac-predictor', 'welch'],
                 ['in.flac', 'out.mid', '--flac-predictor', 'lpc'],
                 ['in.flac', 'out.mid', '--flac-predictor', 'lpc', '--flac', 'host'],
                 ['--songs', 'a.flac', '--out-dir', out, '--flac-predictor', 'lpc'],
                 ['--songs', 'a.flac', '--out-dir', out, '--flac', 'host', '--flac-predictor', 'lpc']):
        with pytest.raises(SystemExit) as e:
            tr.main(argv)
        if 'welch' not in argv:
            assert '--flac device' in str(e.value)
        assert not os.path.exists(out)
    # accepted: the run then fails on the missing input, past the argument checks
    for argv in (['missing.flac', 'out.mid', '--flac', 'device', '--flac-predictor', 'lpc'],
                 ['missing.flac', 'out.mid', '--format', 'wav', '--flac-predictor', 'lpc'],
                 ['missing.flac', 'out.mid', '--flac-predictor', 'fixed']):
        with pytest.raises(OSError):
            tr.main(argv)
    with pytest.raises(ValueError):
        tr.write_song_audio(44100, residual=np.zeros(4), residual_path=str(tmp_path / 'x.flac'), predictor='welch')
    with pytest.raises(ValueError, match='device'):
        tr.write_song_audio(44100, residual=np.zeros(4), residual_path=str(tmp_path / 'x.flac'), predictor='lpc')
    assert not os.path.exists(str(tmp_path / 'x.flac'))
