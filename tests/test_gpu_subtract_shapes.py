"""GPU: the three subtraction entries on rows whose live width F is not n_fft / 2 + 1.  Every other test has F mod 4 = 1,
so only one of the four branches of "pad columns stay out of the max" is ever the last live bin of a row; here F runs over
ldf - 3 .. ldf, on a row shorter than one wave's pass (ldf 72 = 18 float4) and on one where a lane takes a second pass
(ldf 260 = 65 float4).  amt_subtract, amt_subtract_span and amt_subtract_span_stems against numpy float32, bit for bit."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B, T, TG, OVERKILL = 3, 6, 4, 1.25
ONSET = [0, 3, -2]                                              # 3: the span is clipped at T; -2: clamped to 0
GFR = [4, 4, 0]                                                 # the last window has no guess frame at all
GIDX = [0, 1, 1]


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import _lib
    return torch, _lib, _lib.load()


def _np_step(resid, guess, rmax, gmax):
    """numpy float32 restatement of the step, in place on resid [B, T, ldf]; returns the spans as (b, first, end)."""
    spans = []
    for b in range(B):
        g = GIDX[b]
        scale = np.float32(rmax[b]) / np.float32(gmax[g])
        off = max(ONSET[b], 0)
        t_end = min(off + GFR[b], T)
        for t in range(off, t_end):
            sub = (guess[g, t - off] * scale) * np.float32(OVERKILL)
            resid[b, t] = np.maximum(resid[b, t] - sub, np.float32(0))
        spans.append((b, off, t_end))
    return spans


@pytest.mark.parametrize('pad', [3, 2, 1, 0])
@pytest.mark.parametrize('ldf', [72, 260])
def test_subtract_entries_live_width(env, ldf, pad):
    """Pad columns of the residual hold 5.0 (every live bin is below 1) and those of the guesses 0, so a pad column that
    leaked into a maximum shows at once.  Residual in every float, pad columns included; new_max = the maximum over bins
    below F; frame_max = the row's maximum inside each span and untouched outside it; the stem rows = before - after."""
    torch, _lib, lib = env
    F = ldf - pad
    rng = np.random.default_rng(1000 * ldf + pad)
    resid = rng.random((B, T, ldf)).astype(np.float32)
    guess = rng.random((2, TG, ldf)).astype(np.float32)
    resid[:, :, F:] = 5.0
    guess[:, :, F:] = 0.0
    fmax = resid[:, :, :F].max(axis=2)
    rmax, gmax = fmax.max(axis=1), guess[:, :, :F].max(axis=(1, 2))
    want = resid.copy()
    spans = _np_step(want, guess, rmax, gmax)
    want_fmax = fmax.copy()
    for b, t0, t1 in spans:
        want_fmax[b, t0:t1] = want[b, t0:t1, :F].max(axis=1)
    assert sum(t1 - t0 for _, t0, t1 in spans) == 7 and not np.array_equal(want, resid)
    assert np.array_equal(want_fmax.max(axis=1), want[:, :, :F].max(axis=(1, 2)))    # what frames_max reduces

    def dev(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()

    d_guess, d_rmax, d_gmax = dev(guess), dev(rmax), dev(gmax)
    d_gidx, d_gfr, d_on = dev(GIDX, np.int32), dev(GFR, np.int32), dev(ONSET, np.int32)
    d_stems = torch.zeros((1, B * T, ldf), device='cuda')
    d_fb, d_off, d_ts = dev([b * T for b in range(B)], np.int64), dev([0] * B, np.int32), dev([T] * B, np.int32)
    stem = _lib.stem_args(stems=d_stems, frame_base=d_fb, offset=d_off, t_song=d_ts, program=None, prog_group=None,
                          n_prog=0, G=1, pool_frames=B * T)
    got = {}
    for name in ('whole', 'span', 'stems'):
        d_r, d_fm, d_nm = dev(resid), dev(fmax), torch.full((B,), -1.0, device='cuda')
        a = _lib.SubtractArgs()
        a.resid, a.resid_max, a.guess, a.guess_max = d_r.data_ptr(), d_rmax.data_ptr(), d_guess.data_ptr(), d_gmax.data_ptr()
        a.guess_index, a.guess_frames, a.offset_frames = d_gidx.data_ptr(), d_gfr.data_ptr(), d_on.data_ptr()
        a.new_max, a.resid_stride, a.guess_stride = d_nm.data_ptr(), T * ldf, TG * ldf
        a.B, a.T, a.ldf, a.F = B, T, ldf, F
        a.guess_frames_all, a.normalize, a.relu, a.overkill_factor = 0, 1, 1, OVERKILL
        if name == 'whole':
            status = lib.amt_subtract(ctypes.byref(a), None)
        elif name == 'span':
            status = lib.amt_subtract_span(ctypes.byref(a), d_fm.data_ptr(), TG, None)
        else:
            status = lib.amt_subtract_span_stems(ctypes.byref(a), d_fm.data_ptr(), TG, ctypes.byref(stem), None)
        assert status == _lib.AMT_OK, name
        torch.cuda.synchronize()
        got[name] = (d_r.cpu().numpy(), d_fm.cpu().numpy(), d_nm.cpu().numpy())
    for name, (r, fm, nm) in got.items():
        assert np.array_equal(r, want), ('residual', name)
        assert np.array_equal(nm, want[:, :, :F].max(axis=(1, 2))), ('new_max', name)
        assert np.array_equal(fm, fmax if name == 'whole' else want_fmax), ('frame_max', name)
    assert np.array_equal(d_stems.cpu().numpy().reshape(B, T, ldf), resid - want)
