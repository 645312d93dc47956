"""GPU: the batches the benchmark measures (bench.WORKLOADS: C2 256, C3 and C4 1024, C5 2048 windows of 516 frames)
pinned to the path the oracle tests reach.

Parity with the oracle is asserted on small batches (tests/test_gpu_fullsize_fixtures.py: at most 16 windows of 516
frames; the live comparisons: at most 70).  A metric-size batch differs from those in two ways only a large batch shows:
the networks walk it in chunks of 1024 windows through one workspace (RD_CHUNK, amt_rdcnn.hip), and its spectrograms
pass the limits of 32-bit indexing (C5: ph [2048, 516, 1028, 2] is 2.17e9 floats and 8.7e9 bytes).  Two ties close
that gap:

  1. every window range tests/workload_positions.py marks in a metric-size batch -- both ends, every chunk boundary,
     every window in which an element index passes 2^31 or a byte offset 2^32 / 2^33, a ragged range, a single window,
     seeded random ranges -- returns, run as a small batch of its own, the SAME BITS it returns inside the full batch:
     events, every head's pre-rounding floats of every iteration, the residual magnitudes and their maxima, and the
     song-level normalisers of prepare();
  2. the oracle-fixture windows (fullsize_fixtures.npz) are written over marked rows of the full batch -- both sides of
     window 1024, the windows at 2^32 bytes (1012) and at 2^31 floats / 2^33 bytes (2024) -- and compared with the
     fixture there, through the comparison of test_gpu_fullsize_fixtures.py.

The bar of (1) is bit equality: a window's arithmetic does not depend on its batch (fixed-order reductions, per-window
operand scaling).  ONE stage was found to depend on the batch size, by rounding only -- the iSTFT that feeds the CQT heads
(pitch, instrument, velocity) from iteration 1 on: launch_istft cuts a signal into segments of GH hops and takes GH from
the batch size (istft_stream_gh, amt_stft.hip: 32 hops, halved down to 4 while fewer than ~2048 workgroups would be in
flight; at 516 frames GH = 32 from 121 windows on, 4 for 16 windows).  The last frame of a segment is transformed alone,
an inner one paired with its neighbour, and the two round differently, so a window's resynthesised samples differ in
the last bits between a 16-window and a 2048-window batch (measured on C4 / C5: pitch floats 9.2e-5 semitones, velocity
3.0e-4 steps, instrument probabilities 6.8e-6).  For exactly those floats -- CQT heads, iteration >= 1, a range run in
a batch of fewer than 121 windows -- the bar is the project's band for head floats, bands_for(p) of oracle/compare.py
(2e-3, 2e-3, 1e-4); events, the timing heads' floats, every float of iteration 0, the residual and its maxima stay
bit-equal for those ranges too, and two 128-window ranges of C5 (same segment length as the full batch), over windows
1012 / 1024 and 2024, pin every quantity bit for bit.  The windows, heads and loop are bench.py's own
(bench.build, synth.make_windows with seed = workload seed x 1000); nothing here reads anything outside the repository.
A workload is skipped only on a device whose TOTAL memory is below NEED_GB (measured peaks: profiles/workload_batches.txt).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import fixture_waves as fw                                   # noqa: E402
import workload_positions as wp                              # noqa: E402

# device memory a workload's full batch needs while this module runs (GB, total memory of the device; the measured peaks
# of torch.cuda.max_memory_allocated() are in profiles/workload_batches.txt, rounded up here with the earlier
# workloads' retained results included)
NEED_GB = {'c2': 8, 'c3': 32, 'c4': 40, 'c5': 72}
_LOOPS = {}
PEAKS = {}


def _need(name):
    import torch
    total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory
    if total < NEED_GB[name] << 30:
        pytest.skip('%s needs %d GB of device memory, this device has %.0f GB in all' % (name, NEED_GB[name], total / 2 ** 30))


def _loop(name):
    """bench.build's loop of a workload (one per module run), at the default conv mode, one timing stream."""
    import bench
    if name not in _LOOPS:
        wl = bench.WORKLOADS[name]
        p, lp = bench.build(wl, wl['B'])
        _LOOPS[name] = (wl, p, lp)
    return _LOOPS[name]


def _windows(name, B=None):
    """The workload's windows exactly as bench.main renders them on rank 0."""
    from amt_saga import synth
    wl, p, _ = _loop(name)
    L = p.H * (p.timing_frames - 1)
    wave, _notes = synth.make_windows(B or wl['B'], L, seed=wl['seed'] * 1000, notes_per_window=wl['notes'],
                                      groups=wl['groups'], sr=p.sr, device='cuda')
    return wave


def _groups(name, B=None, **kw):
    from amt_saga.audio import ldf_of
    wl, p, lp = _loop(name)
    return wp.groups_for(B or wl['B'], p.timing_frames, ldf_of(p.N), bool(lp.needs_phase), **kw)


def _run(lp, wave, window0=0, refs=None):
    """One run() with the heads' floats traced: dict(events, trace, mag [B, T, F] view, ref_max, refs)."""
    lp.trace = []
    try:
        events, b = lp.run(wave, window0=window0, refs=refs)
        trace = lp.trace
    finally:
        lp.trace = None
    return dict(events=events, trace=trace, mag=b.mag[..., :b.F], ref_max=b.ref_max, refs=lp.refs)


def _rows(res, a, b):
    return dict(events=res['events'][:, a:b], trace=[{k: v[a:b] for k, v in t.items()} for t in res['trace']],
                mag=res['mag'][a:b], ref_max=res['ref_max'][a:b])


CQT_HEADS = ('pitch', 'instrument', 'velocity')             # read the iSTFT of the residual from iteration 1 on
ISTFT_SAME_SEGMENTS = 121                                   # windows of 516 frames from which istft_stream_gh gives 32 hops


def _differences(want, got, bands=None):
    """[(quantity, rows that differ, largest |difference|)] of two results over the same windows; empty = same bits.
    bands: None, or bands_for(p) -- the CQT heads' floats of iterations >= 1 are then held to their band instead (the
    iSTFT's segment length follows the batch size, see the module's docstring)."""
    import torch
    out = []

    def cmp(what, x, y):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape)
        if not torch.equal(x, y):
            ne = (x != y) | (x.isnan() != y.isnan() if x.is_floating_point() else torch.zeros_like(x, dtype=torch.bool))
            dim0 = 1 if what == 'events' else 0
            rows = ne.movedim(dim0, 0).reshape(ne.shape[dim0], -1).any(dim=1).nonzero().flatten().tolist()
            out.append((what, rows, float((x.double() - y.double()).abs().nan_to_num(nan=float('inf')).max())))
    cmp('events', want['events'], got['events'])
    assert len(want['trace']) == len(got['trace'])
    for it, (tw, tg) in enumerate(zip(want['trace'], got['trace'])):
        assert sorted(tw) == sorted(tg)
        for k in tw:
            if bands is not None and it >= 1 and k in CQT_HEADS:
                d = float((tw[k].double() - tg[k].double()).abs().nan_to_num(nan=float('inf')).max())
                if not d <= bands[k]:
                    out.append(('%s floats, iteration %d: outside the band %g' % (k, it, bands[k]), [], d))
                continue
            cmp('%s floats, iteration %d' % (k, it), tw[k], tg[k])
    cmp('residual magnitudes', want['mag'], got['mag'])
    cmp('residual maxima', want['ref_max'], got['ref_max'])
    return out


def _check_ranges(name, lp, wave, full, ranges, prepare_alone=True):
    """Every range, run as a batch of its own at window0 = its start, gives the bits of its rows in the full batch
    (a range shorter than ISTFT_SAME_SEGMENTS windows: the CQT heads' floats of iterations >= 1 within their band)."""
    import torch
    from oracle.compare import bands_for
    bad = []
    assert wave.shape[0] >= ISTFT_SAME_SEGMENTS or lp.iters == 1
    for a, b in ranges:
        sub = wave[a:b].contiguous()
        if prepare_alone:
            lp.prepare(sub)
            for k, v in full['refs'].items():
                if not torch.equal(lp.refs[k], v[a:b]):
                    bad.append(((a, b), 'prepare() alone: ' + k, (lp.refs[k] != v[a:b]).nonzero().flatten().tolist(),
                                float((lp.refs[k].double() - v[a:b].double()).abs().max())))
        got = _run(lp, sub, window0=a, refs={k: v[a:b] for k, v in full['refs'].items()})
        for k, v in got['trace'][0].items():                 # not a constant: the heads' floats are finite numbers
            assert torch.isfinite(v).all(), (name, (a, b), k)
        bands = bands_for(lp.p) if b - a < ISTFT_SAME_SEGMENTS else None
        bad += [((a, b),) + d for d in _differences(_rows(full, a, b), got, bands)]
    assert not bad, '%s: windows give other bits in the full batch than in a batch of their own: %s' % (name, bad)


def _full(name):
    import torch
    _need(name)
    wl, p, lp = _loop(name)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    wave = _windows(name)
    lp.prepare(wave)
    res = _run(lp, wave, window0=0, refs=lp.refs)
    torch.cuda.synchronize()
    PEAKS[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    print('%s: full batch of %d windows: peak device memory %.1f GB above the %.1f GB held before it'
          % (name, wl['B'], PEAKS[name], base / 2 ** 30))
    # spread: the decisions move with the input
    assert torch.unique(res['events'][..., 2]).numel() >= 8, name
    return dict(res, wave=wave)


@pytest.fixture(scope='module')
def full_c2():
    return _full('c2')


@pytest.fixture(scope='module')
def full_c3():
    return _full('c3')


@pytest.fixture(scope='module')
def full_c4():
    return _full('c4')


@pytest.fixture(scope='module')
def full_c5():
    return _full('c5')


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(HERE, 'golden', 'fullsize_fixtures.npz'))


# ---- (1) marked ranges of the full batch against batches of their own -----------------------------------------------
def test_c2_ranges_same_bits(full_c2):
    _, _, lp = _loop('c2')
    _check_ranges('c2', lp, full_c2['wave'], full_c2, _groups('c2'))


def test_c3_ranges_same_bits(full_c3):
    _, _, lp = _loop('c3')
    _check_ranges('c3', lp, full_c3['wave'], full_c3, _groups('c3'))


def test_c4_ranges_same_bits(full_c4):
    """C4's phase plane passes 2^32 bytes inside window 1012 (range 1004-1024)."""
    _, _, lp = _loop('c4')
    ranges = _groups('c4')
    assert any(a <= 1012 < b for a, b in ranges)
    _check_ranges('c4', lp, full_c4['wave'], full_c4, ranges)


def test_c5_ranges_same_bits(full_c5):
    """C5 crosses everything: the chunk boundary at window 1024 on every iteration of every head, 2^32 bytes of ph
    inside window 1012, 2^31 floats and 2^33 bytes of ph and 2^32 bytes of mag inside window 2024."""
    _, _, lp = _loop('c5')
    ranges = _groups('c5')
    assert any(a < 1024 < b for a, b in ranges) and any(a <= 1012 < b for a, b in ranges) and \
        any(a <= 2024 < b for a, b in ranges)
    _check_ranges('c5', lp, full_c5['wave'], full_c5, ranges)


def test_c5_128_window_ranges_every_bit(full_c5):
    """128 windows take the full batch's iSTFT segment length: EVERY quantity bit for bit, the CQT heads' floats of
    iterations 1-4 included, over the chunk boundary and the 2^32-byte window (1012, 1024) and over the window in which
    ph passes 2^31 floats and 2^33 bytes (2024)."""
    _, _, lp = _loop('c5')
    _check_ranges('c5', lp, full_c5['wave'], full_c5, [(960, 1088), (1920, 2048)], prepare_alone=False)


def test_c5_full_batch_twice_same_bits(full_c5):
    _, _, lp = _loop('c5')
    again = _run(lp, full_c5['wave'], window0=0, refs=full_c5['refs'])
    assert not _differences(full_c5, again)


@pytest.mark.parametrize('mode', [2, 0])
def test_c3_other_conv_modes(mode, full_c3):
    """C3 with every net in split-fp16 without the FFT-domain layers (2) and on the f32 MFMA (0, the value_f32_mfma leg
    of the benchmark): first range, last range and the chunk ranges (C3 is one chunk: there are none)."""
    _, _, lp = _loop('c3')
    wave = full_c3['wave']
    B = wave.shape[0]
    default = {k: n.mode for k, n in lp.nets.items()}
    try:
        for n in lp.nets.values():
            n.set_mode(mode)
        full = _run(lp, wave, window0=0, refs=full_c3['refs'])
        ranges = [r for r in _groups('c3', n_random=0) if r[0] == 0 or r[1] == B or r[0] < 1024 < r[1]]
        _check_ranges('c3 mode %d' % mode, lp, wave, full, ranges, prepare_alone=False)
    finally:
        for k, n in lp.nets.items():
            n.set_mode(default[k])


def test_c3_1030_windows_second_chunk():
    """The smallest batch that sends the timing heads' FFT-domain layers (mode 3) through a second chunk: 6 windows
    behind the first 1024, in the workspace the first chunk used."""
    _need('c3')
    _, _, lp = _loop('c3')
    assert all(n.mode == 3 for n in lp.nets.values())
    wave = _windows('c3', 1030)
    lp.prepare(wave)
    full = _run(lp, wave, window0=0, refs=lp.refs)
    _check_ranges('c3 x 1030', lp, wave, full, [(0, 16), (1016, 1030)])


def test_c3_two_timing_streams(full_c3):
    """timing_end on a second stream under timing_start: the one-stream batch's events, floats and residual, bit for bit
    (bench.py compares the events only)."""
    _, _, lp = _loop('c3')
    lp.timing_streams = 2
    try:
        two = _run(lp, full_c3['wave'], window0=0, refs=full_c3['refs'])
    finally:
        lp.timing_streams = 1
    assert not _differences(full_c3, two)


# ---- (2) oracle-fixture windows inside the full batch --------------------------------------------------------------------
def _fixture_inside(name, full, fx):
    import torch
    from amt_saga.audio import ldf_of
    from test_gpu_fullsize_fixtures import _waves, compare_with_fixture
    wl, p, lp = _loop(name)
    c = fw.CASES[name]
    # the fixture's loop is the workload's loop
    assert (c['heads'], c['iters'], c['groups'], c['hp']) == (wl['heads'], wl['iters'], wl['groups'], dict(N=p.N))
    wave_h = _waves(name, fx)                               # checks the SHA-1 of the re-rendered 24-bit audio
    rows = wp.fixture_rows(wl['B'], p.timing_frames, ldf_of(p.N), bool(lp.needs_phase), wave_h.shape[0])
    wave = full['wave'].clone()
    idx = torch.as_tensor(rows, device=wave.device)
    wave[idx] = torch.from_numpy(wave_h).to(wave.device)
    got = _run(lp, wave, window0=0, refs=None)              # the product's own normalisers, as in the fixture test
    host = lambda t: t[idx].cpu().numpy()
    worst = compare_with_fixture(name, fx, p, wl['iters'], rows, {k: host(v) for k, v in got['refs'].items()},
                                 got['events'][:, idx].cpu().numpy(), [{k: host(v) for k, v in t.items()} for t in got['trace']],
                                 host(got['mag']), host(got['ref_max']))
    # and the rows that were not overwritten are what they were
    keep = torch.ones(wl['B'], dtype=torch.bool, device=wave.device)
    keep[idx] = False
    assert torch.equal(got['events'][:, keep], full['events'][:, keep])
    print('%s: fixture windows at rows %s of the %d-window batch: events bit-exact, worst float distances %s'
          % (name, rows, wl['B'], {k: '%.2g' % v for k, v in worst.items()}))
    return rows


def test_c3_fixture_windows_inside_the_batch(full_c3, fx):
    _fixture_inside('c3', full_c3, fx)


def test_c4_fixture_windows_inside_the_batch(full_c4, fx):
    rows = _fixture_inside('c4', full_c4, fx)
    assert 1012 in rows


def test_c5_fixture_windows_inside_the_batch(full_c5, fx):
    rows = _fixture_inside('c5', full_c5, fx)
    assert 1023 in rows and 1024 in rows and 1012 in rows and 2024 in rows
