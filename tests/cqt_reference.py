"""Helpers and the ONE set of case lists of the constant-Q geometry tests (csrc/amt_cqt.hip).  Test infrastructure, numpy
only: imported by test_cqt_reference_cpu.py (no GPU: the premises the lists rest on) and test_gpu_cqt_geometry.py, so
the two cannot drift apart.  The float64 definition is oracle/cqt.py; nothing here restates the transform.

Targeting.  Both whole-window forms return one number per window, max over bins and frames of |C[k, t]|, which hides
every frame and bin but the argmax.  `matched_burst` moves the argmax where a test wants it: the signal is bin k's own
analysis filter (periodic Hann times the cosine of the integer oscillator phase) centred on frame t.  With short filters
(N_k of a few hundred samples, bpo 12) no other (bin, frame) reaches 0.8 of the target's value
(test_cqt_reference_cpu.py asserts it for every target below), so a kernel that gets the target frame or bin wrong is
off by 20 % where the bar is 1e-4.

Lengths.  `length_table` sets N_k by hand (the kernels take any positive length; `phase_inc` stays that of an ordinary
grid): the block-sum kernel takes its head sums from a snapshot after N_k mod 32 samples (4 groups x 8 cases) and splits
lanes by (N_k mod H) >> 5, which the musical grids only sample."""
import numpy as np

from oracle import cqt as ocqt

SR = 44100
BPO = 12
HOPS = (128, 256, 512, 1024, 2048)


def grid(fmin, n_bins):
    """(phase_inc uint32, length int32) of an ordinary bpo-12 grid at 44100 Hz."""
    inc, length, _ = ocqt.cqt_table(SR, fmin, n_bins, BPO)
    return inc, length


def all_frames(x, inc, length, hop):
    """|C| of every frame: float64 [n_bins, T], T = 1 + len(x) // hop."""
    T = 1 + len(x) // hop
    return ocqt.cqt_frames(x, np.arange(T), inc, length, hop)


def matched_burst(L, k, t, inc, length, hop):
    """float32 [L]: zero except for bin k's analysis filter centred on sample t * hop, clipped to [0, L)."""
    nk, ik = int(length[k]), int(inc[k])
    n = np.arange(nk, dtype=np.uint64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nk) / nk)
    ph = ((n * np.uint64(ik)) & np.uint64(0xFFFFFFFF)).astype(np.float64) * (2.0 * np.pi / 2.0 ** 32)
    a = int(t) * hop - nk // 2
    lo, hi = max(a, 0), min(a + nk, L)
    x = np.zeros(L, np.float32)
    if hi > lo:
        x[lo:hi] = (w * np.cos(ph))[lo - a:hi - a]
    return x


def length_table(base, residues):
    """int32 [len(residues)]: N_k = base + residues[k], every one positive."""
    length = np.asarray([int(base) + int(r) for r in residues], np.int32)
    assert length.min() >= 1
    return length


def cqm_geometry(L, hop):
    """(q, r) of the MFMA whole-window form -- full 8-tile groups per wave, leftover 16-block tiles -- or None where
    amt_cqt_window_max_mfma answers AMT_E_UNSUPPORTED.  Restates cqm_geometry of csrc/amt_cqt.hip."""
    if hop not in (256, 512, 1024, 2048):
        return None
    n_mt = ((L + hop - 1) // hop + 15) // 16
    q, r = n_mt // 8, n_mt % 8
    if r > 2:
        q, r = q + 1, 0
    return None if q > 4 else (q, r)


def blocks_fit_lds(lib, L, hop):
    """Whether the block sums of an L-sample signal fit the LDS (host-only: no launch)."""
    return int(lib.amt_cqt_window_max_workspace(int(L), int(hop), 1, 1)) == 0


def largest_lds_length(lib, hop):
    """The largest L whose block sums fit the LDS, by bisection over blocks_fit_lds."""
    lo, hi = hop, 1 << 24                     # fits / does not
    assert blocks_fit_lds(lib, lo, hop) and not blocks_fit_lds(lib, hi, hop)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if blocks_fit_lds(lib, mid, hop):
            lo = mid
        else:
            hi = mid
    return lo


LDS_HOPS_MAX = 1692                           # what include/amt_saga.h states: the block sums fit while L // hop <= 1692


# ---- hand-set lengths of the slices sweep -----------------------------------------------------------------------------
def length_cases(H):
    """name -> N_k table for hop H.  `edges`: N_k mod H in {0, 1, 31, 32, 33, H - 1}, N_k = H - 1, 2 and 31 (below one
    lane's run of 32 samples), 3 H (whole blocks only), 4 H + 33 and 9 H + 5 (longer than the 777-sample signal at every
    hop).  `r32_lo` / `r32_hi`: N_k mod 32 = 0..15 / 16..31, spread over three values of (N_k mod H) >> 5."""
    return {
        'edges': length_table(H, [0, 1, 31, 32, 33, H - 1, -1, 2 - H, 31 - H, 2 * H, 3 * H + 33, 8 * H + 5]),
        'r32_lo': length_table(H + 64, [r + 32 * (r % 3) for r in range(16)]),
        'r32_hi': length_table(H + 64, [r + 32 * (r % 3) for r in range(16, 32)]),
    }


LENGTH_CASE_NAMES = ('edges', 'r32_lo', 'r32_hi')
SWEEP_FMIN = 220.0                            # phase_inc of the hand-set tables: an ordinary grid from A3
SHORT_L = 777                                 # below 2048 samples: no wave takes the aligned 16-byte fetch


def sweep_lengths(H):
    """Signal lengths of the slices sweep.  A pass of the block-sum workgroup is 4 * 64 / (H / 32) = 8192 / H blocks,
    i.e. 8192 samples at every hop: a bin whose N_k / 2 is a multiple of H has exactly pass - 1, pass and pass + 1 blocks
    that hold samples at the first three lengths, every other bin one block more."""
    return (8192 - H, 8192, 8192 + H, SHORT_L)


def frame_sets(T, frames):
    """int32 [B, frames] of frame indices in -1 .. T - 1: frame 0, frame T - 1, a duplicate, a -1 hole, a compact run, a
    spread set and an all-hole row."""
    c = lambda v: [min(max(int(i), -1), T - 1) for i in v]
    if frames == 1:
        rows = [[0], [T - 1], [-1], [T // 2]]
    elif frames == 3:
        rows = [c([0, T - 1, -1]), c([T // 2] * 3), c([T - 3, T - 2, T - 1]), c([-1, -1, -1])]
    else:
        assert frames == 8
        rows = [c(range(8)), c(np.linspace(0, T - 1, 8).round()), c([T - 1, 0, T - 1, -1, T // 2, T // 2, 1, T - 2]),
                c(np.arange(8) + T - 8), c([-1] * 8), c([-1, -1, T // 3, -1, -1, -1, -1, 2 * T // 3])]
    return np.asarray(rows, np.int32)


def sweep_wave(L, B, seed):
    """float32 [B, L]: white noise plus two tones inside the SWEEP_FMIN grid -- every row of the transform is of
    comparable size, whatever its N_k."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / SR
    return np.stack([0.3 * rng.standard_normal(L) + 0.4 * np.sin(2 * np.pi * 261.6 * t + b) +
                     0.3 * np.sin(2 * np.pi * 370.0 * t + 2 * b) for b in range(B)]).astype(np.float32)


# ---- whole-window maximum by targeting --------------------------------------------------------------------------------
FMIN_OF_HOP = {128: 7040.0, 256: 3520.0, 512: 3520.0, 1024: 1760.0, 2048: 1760.0}     # N_0 = 211, 422, 422, 843, 843


def _length_for_blocks(nblk, hop):
    """ceil(L / hop) = nblk, L no multiple of 4 (the MFMA form's ragged tail), T - 1 = nblk - 1 centred 57 samples
    before the end."""
    return (nblk - 1) * hop + 57 if nblk > 1 else hop


def edge_targets(n_bins, T):
    """(bin, frame) targets: frames 0, 1, T - 2, T - 1, the M-tile edge 15 / 16 / 17, the wave-owned tile edge 127 / 128
    (where T allows), walking bin positions 0..6 of a group of seven; the first and last bin at the first and last
    frame; the first bin of the ragged last group."""
    frames = []
    for f in (0, 1, 15, 16, 17, 127, 128, T - 2, T - 1):
        if 0 <= f < T and f not in frames:
            frames.append(f)
    tg = [(i % 7, f) for i, f in enumerate(frames)]
    last = n_bins - 1
    tg += [(last, T - 1), (last, 0), (0, T - 1), (7 * (last // 7), min(16, T - 1)), (last, min(17, T - 1))]
    if T > 128:
        tg += [(3, 127), (last, 128), (5, 16), (6, 15), (4, 17)]
    out = []
    for kt in tg:
        if kt not in out:
            out.append(kt)
    return out


def _max_case(name, hop, nblk, n_bins, targets=None, forms=('valu', 'mfma'), L=None):
    L = _length_for_blocks(nblk, hop) if L is None else L
    T = 1 + L // hop
    tg = edge_targets(n_bins, T) if targets is None else [(k, t) for k, t in targets if 0 <= t < T]
    tg = [kt for i, kt in enumerate(tg) if kt not in tg[:i]]
    return dict(name=name, hop=hop, L=L, T=T, fmin=FMIN_OF_HOP[hop], n_bins=n_bins, targets=tg, forms=forms)


def _few(n_bins, T, extra=()):
    last = n_bins - 1
    return [(0, 0), (last, T - 1), (3, T - 2), (6, 16), (7, 17), (1, 1)] + list(extra)


# the shortest block count of every (Q, R) instantiation of cqt_max_mfma_kernel (CqmShapes)
QR_BLOCKS = {(0, 1): 1, (0, 2): 17, (1, 0): 33, (1, 1): 129, (1, 2): 145, (2, 0): 161, (2, 1): 257, (2, 2): 273,
             (3, 0): 289, (3, 1): 385, (3, 2): 401, (4, 0): 417, (4, 1): 513, (4, 2): 529}
NEVER_RUN_BEFORE = ((1, 1), (1, 2), (2, 0), (2, 2), (3, 1), (3, 2), (4, 0), (4, 2))


def _wave3(n_bins, T):
    """frames 511, 512, 513 and T - 1 at bin positions 0 and 6 of a group: frames from 512 on are wave 3's, computed from
    the previous bin's buffers one loop iteration later."""
    last = n_bins - 1
    return [(0, 511), (6, 511), (0, 512), (6, 512), (7, 512), (last, 512), (0, 513), (6, 513), (0, T - 1), (6, T - 1),
            (last, T - 1), (7, T - 2)]


def _build_max_cases():
    cases = []
    # every hop, both forms (hop 128: VALU only), the full edge list; 13 = 7 + 6 and 8 = 7 + 1 bins
    for hop, n_bins in ((128, 13), (256, 13), (512, 8), (1024, 13), (2048, 8)):
        cases.append(_max_case('hop%d_edges' % hop, hop, 145, n_bins, forms=('valu',) if hop == 128 else ('valu', 'mfma')))
    cases.append(_max_case('hop256_edges_8bins', 256, 145, 8))
    # one case per (Q, R) at hop 256
    for i, ((q, r), nblk) in enumerate(sorted(QR_BLOCKS.items())):
        n_bins = 13 if i % 2 else 8
        L = _length_for_blocks(nblk, 256)
        T = 1 + L // 256
        cases.append(_max_case('q%dr%d' % (q, r), 256, nblk, n_bins, _few(n_bins, T, _wave3(n_bins, T) if q == 4 else ())))
    # (4, 0) with T = 513: L = 512 hops exactly
    cases.append(_max_case('q4r0_T513', 256, 512, 13, _few(13, 513, _wave3(13, 513)), L=512 * 256))
    # the wave-3 frames at the longest hop (64 k-steps)
    cases.append(_max_case('hop2048_q4r2', 2048, 529, 8, [(0, 0), (0, 511), (6, 512), (0, 513), (7, 528), (6, 527)]))
    for c in cases:
        assert c['n_bins'] <= 16 and c['L'] <= 545 * c['hop'] and 1 <= len(c['targets']) <= 24, c['name']
    return cases


MAX_CASES = _build_max_cases()
MAX_CASE_IDS = [c['name'] for c in MAX_CASES]
SCALED_CASE = 'q4r2'                          # the case that also runs with a louder, a quieter and a silent window
REFUSED_L = 545 * 256                         # one block more than the MFMA form's wave-private slabs hold


def case_grid(case):
    return grid(case['fmin'], case['n_bins'])


def case_waves(case):
    """float32 [targets, L]: window b is the matched burst of target b."""
    inc, length = case_grid(case)
    return np.stack([matched_burst(case['L'], k, t, inc, length, case['hop']) for k, t in case['targets']])
