"""GPU: the device FLAC decoder (amt_flacdec.hip) against the writer's source PCM and flac.decode of the recorded files.
Integers and bytes only: nothing here has a tolerance."""
import glob
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_encode_reference as R                                  # noqa: E402
import flac_stream_writer as W                                     # noqa: E402
from oracle import synth as osynth                                 # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'flac', '*.flac')))
SENTINEL = 0x5A


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import audio, flac, _lib
    return dict(torch=torch, audio=audio, flac=flac, _lib=_lib, lib=_lib.load())


@pytest.fixture(scope='module')
def streams(env, tmp_path_factory):
    """[(name, data, pcm int64 [n, ch], bps, reader's frame starts)]: the corpus and the four recorded files, the
    expected values computed once by the sequential reader."""
    d = tmp_path_factory.mktemp('flac_gpu')
    out = []
    for name, data, pcm, bps in W.corpus():
        path = str(d / (name + '.flac'))
        open(path, 'wb').write(data)
        starts, got, _, _ = W.reader_frame_starts(env['flac'], path)
        assert np.array_equal(got, pcm)
        out.append((name, data, pcm, bps, starts))
    assert len(GOLDEN) == 4
    for path in GOLDEN:
        starts, got, _, bps = W.reader_frame_starts(env['flac'], path)
        out.append((os.path.basename(path), open(path, 'rb').read(), got, bps, starts))
    return out


def _ragged(env, datas, verify=True, pad=(5, 3)):
    """amt_flac_decode_ragged called directly, every device buffer between sentinels, the file bytes at odd offsets
    (pad[0] bytes before the first file and pad[1] between files).  Returns host copies and asserts the sentinels."""
    torch, audio, lib, _lib = env['torch'], env['audio'], env['lib'], env['_lib']
    infos, sm, cm, md5, slot_ints, out_values = audio._flac_tables(datas, verify)
    blob, at = bytearray(b'\xee' * pad[0]), []
    for dta in datas:
        at.append(len(blob))
        blob += dta + b'\xee' * pad[1]
    sm = sm.copy()
    sm[:, 0] = at
    if len(blob) % 2 == 0:
        blob += b'\xee'
    assert any(a % 2 for a in at)
    dev = 'cuda'
    G = 64                                                                         # guard bytes on either side

    def guarded(nbytes):
        t = torch.full((nbytes + 2 * G,), SENTINEL, dtype=torch.uint8, device=dev)
        return t, t[G:G + nbytes]
    n, n_cand = len(datas), len(cm)
    need = int(lib.amt_flac_decode_scratch_bytes(n_cand, slot_ints))
    bufs = {k: guarded(b) for k, b in dict(scratch=need, out=4 * out_values, pcm=4 * out_values, status=32 * n,
                                           cand_out=24 * max(n_cand, 1), md5=16 * n).items()}
    data_d = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
    sm_d = torch.from_numpy(sm).to(dev)
    cm_d = torch.from_numpy(cm if n_cand else np.zeros((1, 7), np.int64)).to(dev)
    md5_d = torch.from_numpy(md5.copy()).to(dev)
    p = lambda k: bufs[k][1].data_ptr()                                            # noqa: E731
    _lib.check(lib.amt_flac_decode_ragged(
        data_d.data_ptr(), data_d.numel(), sm_d.data_ptr(), n, cm_d.data_ptr(), n_cand, md5_d.data_ptr(),
        audio.FLAC_VERIFY[verify], p('scratch'), need, slot_ints, p('out'), p('pcm'), out_values, p('status'),
        p('cand_out'), p('md5'), None))
    torch.cuda.synchronize()
    host = {}
    for k, (whole, inner) in bufs.items():
        w = whole.cpu().numpy()
        assert np.all(w[:G] == SENTINEL) and np.all(w[len(w) - G:] == SENTINEL), k
        host[k] = w[G:len(w) - G].copy()
    return dict(out=host['out'].view(np.float32), pcm=host['pcm'].view(np.int32),
                status=host['status'].view(np.int64).reshape(n, 4),
                cand_out=host['cand_out'].view(np.int64).reshape(-1, 3)[:n_cand], md5=host['md5'].reshape(n, 16),
                sm=sm, cm=cm, infos=infos)


def _check_stream(r, i, pcm, bps, starts=None):
    sm = r['sm'][i]
    ch, total, base = int(sm[3]), int(sm[5]), int(sm[6])
    assert (total, ch) == pcm.shape
    got = r['pcm'][base:base + total * ch].reshape(total, ch)
    assert np.array_equal(got, pcm)
    want_f = (pcm.astype(np.float64) * 2.0 ** -(bps - 1)).astype(np.float32)
    assert np.array_equal(r['out'][base:base + total * ch].reshape(total, ch), want_f)
    assert np.array_equal(want_f.astype(np.float64) * 2.0 ** (bps - 1), pcm)       # (float32 holds them exactly)
    assert r['status'][i].tolist() == [0, r['status'][i][1], (1 << 63) - 1, 0]
    if starts is not None:
        lo, hi = int(sm[7]), int(sm[8])
        on = r['cm'][lo:hi, 1][r['cand_out'][lo:hi, 2] == 1]
        assert on.tolist() == starts


def test_one_ragged_call_over_the_whole_corpus(env, streams):
    r = _ragged(env, [s[1] for s in streams])
    for i, (name, data, pcm, bps, starts) in enumerate(streams):
        _check_stream(r, i, pcm, bps, starts)
        assert r['md5'][i].tobytes() == W.pcm_md5(pcm, bps), name
        if name == W.PLANTED:
            lo, hi = int(r['sm'][i][7]), int(r['sm'][i][8])
            k = r['cm'][lo:hi, 1].tolist().index(W.planted_offset(data))
            assert r['cand_out'][lo + k, 2] == 0                                   # the planted header: off chain
    raw = np.ascontiguousarray(streams[0][2].astype('<i2')).tobytes()
    assert hashlib.md5(raw).digest() == r['md5'][0].tobytes()                      # hashlib's, said once without the helper


def test_alone_and_repeated(env, streams):
    datas = [s[1] for s in streams]
    a = _ragged(env, datas)
    b = _ragged(env, datas)
    for k in ('out', 'pcm', 'status', 'cand_out', 'md5'):
        assert a[k].tobytes() == b[k].tobytes(), k
    for i, (name, data, pcm, bps, starts) in enumerate(streams):                   # every stream alone
        one = _ragged(env, [data], pad=(1, 0))
        _check_stream(one, 0, pcm, bps, starts)
        base, nv = int(a['sm'][i][6]), pcm.size
        assert one['out'].tobytes() == a['out'][base:base + nv].tobytes(), name       # the same bytes as in the batch
        assert one['pcm'].tobytes() == a['pcm'][base:base + nv].tobytes(), name
        assert one['md5'][0].tobytes() == a['md5'][i].tobytes(), name
        lo, hi = int(a['sm'][i][7]), int(a['sm'][i][8])
        assert np.array_equal(one['cand_out'], a['cand_out'][lo:hi]), name


def test_round_trip_with_the_encoder(env):
    torch, audio = env['torch'], env['audio']
    sig = R.signals()
    assert len(sig) == 14
    for bps in (24, 16):
        for blocksize in (16, 192, 4096):
            ys = [v[:1000] if blocksize == 16 else v for v in sig.values()]
            files = audio.flac_encode([torch.from_numpy(y).cuda() for y in ys], 44100, bps=bps, blocksize=blocksize)
            got = audio.flac_decode(files, verify=True, pcm=True)
            r = audio.flac_decode_streams(files, verify=True)
            md5 = r['md5'].cpu().numpy()
            for i, (y, f, (wave, sr, gbps, pcm)) in enumerate(zip(ys, files, got)):
                q = R.quantise(y, bps)
                assert (sr, gbps) == (44100, bps) and wave.dim() == 1
                assert np.array_equal(pcm.cpu().numpy(), q)
                assert np.array_equal(wave.cpu().numpy(), (q * 2.0 ** -(bps - 1)).astype(np.float32))
                assert md5[i].tobytes() == f[26:42] == R.pcm_md5(q, bps)


def test_damaged_streams_are_refused_and_neighbours_untouched(env, streams):
    audio = env['audio']
    good = {s[0]: s for s in streams}
    a, b = good['bps20'], good['stereo_all']
    bad = [(n, d, k) for n, d, k in W.damaged() if k != 'metadata']
    datas = []
    for n, d, k in bad:
        datas += [a[1], d, b[1]]                                                   # every damaged stream between two good ones
    r = _ragged(env, datas)
    kinds = set()
    for j, (name, d, kind) in enumerate(bad):
        _check_stream(r, 3 * j, a[2], a[3], a[4])
        _check_stream(r, 3 * j + 2, b[2], b[3], b[4])
        msg = audio.flac_status_error(r['status'][3 * j + 1])
        assert msg is not None, name
        got = 'crc16' if 'CRC-16' in msg else 'sync' if msg.startswith('lost sync') else 'md5' if 'MD5' in msg else msg
        assert got in (('crc16', 'sync') if kind == 'any' else (kind,)), (name, msg)
        kinds.add(got)
        with pytest.raises(ValueError) as e:
            audio.flac_decode([a[1], d])
        assert msg in str(e.value) and 'file 1 of the call' in str(e.value)
    assert kinds == {'crc16', 'sync', 'md5'}
    md5_only = next(d for n, d, k in bad if k == 'md5')
    assert len(audio.flac_decode([md5_only], verify='crc')) == 1                   # 'crc' skips the digest
    flip = next(d for n, d, k in bad if n == 'bps24:bitflip')
    with pytest.raises(ValueError):
        audio.flac_decode([flip], verify='crc')
    audio.flac_decode([flip], verify=False)                                        # as the reader with verify=False


def test_load_flac_on_the_recorded_files(env, streams):
    audio = env['audio']
    want = streams[-4:]
    got = audio.load_flac(GOLDEN, pcm=True)
    for (name, data, pcm, bps, _), (wave, sr, gbps, ipcm) in zip(want, got):
        assert (sr, gbps) == (44100, bps)
        assert np.array_equal(ipcm.cpu().numpy().reshape(pcm.shape), pcm)
        y, _ = env['flac'].load_float(os.path.join(ROOT, 'tests', 'golden', 'flac', name))
        assert np.array_equal(wave.cpu().numpy().astype(np.float64), y)            # what the host path reads
    one = audio.load_flac(GOLDEN[0])
    assert np.array_equal(one[0].cpu().numpy(), got[0][0].cpu().numpy())
    st = next(s for s in streams if s[0] == 'stereo_all')
    w = audio.flac_decode([st[1]])[0][0]
    assert tuple(w.shape) == st[2].shape


@pytest.mark.parametrize('cli', ['one_file', 'songs'])
def test_command_line_decode_device_equals_host(env, tmp_path, cli):
    """Both modes of the command line on the smallest live walk: mono inputs written by flac.save_float give
    byte-identical .mid files under --decode host and --decode device."""
    from amt_saga import flac, transcribe as tr
    from amt_saga.hyperparams import Hyperparams
    p = Hyperparams(N=2048, window_size_note_time=1)
    L = p.H * (p.timing_frames - 1)
    paths = []
    for k, frac in enumerate((1.4, 2.1)):
        n = int(frac * L)
        notes_in = [(k % 3, 60 + 2 * j + k, 100, 0.2 + 0.7 * j, 0.4) for j in range(int(n / p.sr / 0.7))]
        paths.append(str(tmp_path / ('clip%d.flac' % k)))
        flac.save_float(osynth.render_window(notes_in, n, p.sr).numpy(), paths[-1], p.sr)
    mids = {}
    for mode in tr.DECODERS:
        if cli == 'one_file':
            one = str(tmp_path / ('one_%s.mid' % mode))
            tr.main([paths[1], one, '--iters', '1', '--decode', mode])
            mids[mode] = [open(one, 'rb').read()]
        else:
            out_dir = str(tmp_path / ('mid_' + mode))
            tr.main(['--songs'] + paths + ['--out-dir', out_dir, '--slots', '2', '--iters', '1', '--decode', mode])
            mids[mode] = [open(os.path.join(out_dir, 'clip%d.mid' % k), 'rb').read() for k in range(2)]
    assert mids['host'] == mids['device']
    assert all(len(m) > 20 for m in mids['host'])
