"""CPU: bench.py --dump-outputs writes what the timed step returned, as float32 / float64 arrays, within its size
bound, with the same seeded sample of windows every run."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _batch(B, T, F, ldf, seed):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(mag=torch.rand(B, T, ldf, generator=g), ref_max=torch.rand(B, generator=g), F=F)


def test_dump_outputs(tmp_path, monkeypatch):
    B, T, F, ldf = 40, 12, 9, 12
    monkeypatch.setattr(bench, 'DUMP_BYTES', 5 * T * F * 4)           # room for 5 of the 40 windows
    b = _batch(B, T, F, ldf, 0)
    ev = torch.randint(-1, 500, (B, 7), dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / 'a'), ev, b)
    bench.dump_outputs(str(tmp_path / 'b'), ev, _batch(B, T, F, ldf, 0))
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['events.npy', 'residual_mag_sample.npy', 'residual_mag_windows.npy', 'residual_ref_max.npy']
    got = {n[:-4]: np.load(tmp_path / 'a' / n) for n in names}
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(tmp_path / 'b' / n))
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got['events'], ev.numpy())
    assert np.array_equal(got['residual_ref_max'], b.ref_max.numpy())
    w = got['residual_mag_windows'].astype(np.int64)
    assert len(w) == 5 and len(set(w)) == 5 and w.min() >= 0 and w.max() < B
    assert np.array_equal(got['residual_mag_sample'], b.mag[w, :, :F].numpy())      # padded columns dropped
