"""CPU: the window ranges tests/test_gpu_workload_batches.py compares (tests/workload_positions.py), checked against the
product's own geometry -- ldf_of, Hyperparams(N=2048) and bench.WORKLOADS -- so that a later change of layout or of
workload size cannot turn the GPU tests' 32-bit and chunk-boundary positions into ordinary ones unnoticed."""
import pytest

import workload_positions as wp


def _geometry(name):
    import bench
    from amt_saga.audio import ldf_of
    from amt_saga.hyperparams import Hyperparams
    from amt_saga.loop import TranscriptionLoop
    wl = bench.WORKLOADS[name]
    p = Hyperparams(N=2048)
    # the phase plane is stored exactly when the loop says so (prepare(): 516 frames = hop x 515 samples, no odd length)
    lp = TranscriptionLoop(p, heads=wl['heads'], iters=wl['iters'], subtract=wl['subtract'], groups=wl['groups'])
    return wl['B'], p.timing_frames, ldf_of(p.N), bool(lp.needs_phase)


def _check_shape(groups, B):
    assert groups == sorted(groups)
    assert all(0 <= a < b <= B for a, b in groups), groups
    assert all(groups[i][1] <= groups[i + 1][0] for i in range(len(groups) - 1)), ('overlap', groups)


def _covered(groups, a, b):
    return any(lo <= a and b <= hi for lo, hi in groups)


def test_c5_batch_crosses_every_limit_and_the_chunk():
    B, T, ldf, with_phase = _geometry('c5')
    assert (B, T, ldf, with_phase) == (2048, 516, 1028, True)
    # not vacuous: the batch's phase plane does pass 2^31 floats and 2^33 bytes, its magnitudes 2^32 bytes
    assert B * T * ldf * 2 > 1 << 31 and B * T * ldf * 8 > 1 << 33 and B * T * ldf * 4 > 1 << 32
    lim = dict(wp.limit_windows(B, T, ldf, with_phase))
    assert lim == {'ph element index (floats) passes 2^31': 2024, 'ph byte offset passes 2^32': 1012,
                   'ph byte offset passes 2^33': 2024, 'mag byte offset passes 2^32': 2024}
    for w in lim.values():                                  # the limit lies inside window w
        assert w < B
    n = T * ldf
    assert 2024 * 2 * n <= 1 << 31 < 2025 * 2 * n and 1012 * 8 * n <= 1 << 32 < 1013 * 8 * n
    assert 2024 * 8 * n <= 1 << 33 < 2025 * 8 * n and 2024 * 4 * n <= 1 << 32 < 2025 * 4 * n
    g = wp.groups_for(B, T, ldf, with_phase)
    _check_shape(g, B)
    assert _covered(g, 0, 16) and _covered(g, B - 16, B)
    assert _covered(g, 1016, 1032), 'no range straddles window 1024'
    assert _covered(g, 1004, 1020) and _covered(g, 2016, 2032)
    sizes = [b - a for a, b in g]
    assert 5 in sizes and 1 in sizes and sizes.count(16) >= 4 + 2
    rows = wp.fixture_rows(B, T, ldf, with_phase, 7)         # the C5 fixture holds 7 windows
    assert len(set(rows)) == 7 and 1023 in rows and 1024 in rows and 2024 in rows and 1012 in rows
    assert all(_covered(g, r, r + 1) for r in rows)


@pytest.mark.parametrize('name,limits', [('c2', {}), ('c3', {}), ('c4', {'ph byte offset passes 2^32': 1012})])
def test_other_workloads(name, limits):
    B, T, ldf, with_phase = _geometry(name)
    assert with_phase == (name == 'c4') and T == 516
    assert dict(wp.limit_windows(B, T, ldf, with_phase)) == limits
    g = wp.groups_for(B, T, ldf, with_phase)
    _check_shape(g, B)
    assert _covered(g, 0, 16) and _covered(g, B - 16, B)
    assert not any(a < 1024 < b for a, b in g)              # B <= chunk: nothing straddles
    for w in limits.values():
        assert _covered(g, w - 8, min(B, w + 8))
    sizes = [b - a for a, b in g]
    assert 5 in sizes and 1 in sizes and sizes.count(16) >= 4
    n = {'c3': 16, 'c4': 8}.get(name)
    if n:
        rows = wp.fixture_rows(B, T, ldf, with_phase, n)
        assert len(set(rows)) == n and all(_covered(g, r, r + 1) for r in rows) and 0 in rows and B - 1 in rows


def test_small_and_edge_batches():
    T, ldf = 516, 1028
    for B in (1, 5, 15):
        assert wp.groups_for(B, T, ldf, True) == [(0, B)]
    assert wp.groups_for(16, T, ldf, False) == [(0, 16)]
    g = wp.groups_for(1024, T, ldf, False)                  # B == chunk: no boundary inside the batch
    _check_shape(g, 1024)
    assert g[0] == (0, 16) and g[-1] == (1008, 1024) and not any(a < 1024 < b for a, b in g)
    g = wp.groups_for(1030, T, ldf, False)                  # the smallest second chunk the GPU test runs: 6 windows
    _check_shape(g, 1030)
    assert g[-1] == (1014, 1030) and _covered(g, 1016, 1030)
    g = wp.groups_for(2049, T, ldf, False)
    assert _covered(g, 1016, 1032) and _covered(g, 2040, 2049)
    g = wp.groups_for(3000, T, ldf, False, chunk=1000, group=8)
    _check_shape(g, 3000)
    assert _covered(g, 996, 1004) and _covered(g, 1996, 2004) and g[-1][1] == 3000
    assert wp.groups_for(2048, T, ldf, True, seed=0) == wp.groups_for(2048, T, ldf, True, seed=0)
    assert wp.groups_for(2048, T, ldf, True, seed=0) != wp.groups_for(2048, T, ldf, True, seed=1)
    assert len(wp.groups_for(2048, T, ldf, True, n_random=1)) == len(wp.groups_for(2048, T, ldf, True)) - 3
