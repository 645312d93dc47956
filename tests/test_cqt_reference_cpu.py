"""No GPU: the premises the case lists of tests/cqt_reference.py rest on (test_gpu_cqt_geometry.py walks the same lists).

  targeting       every matched burst peaks at its own (bin, frame) and nothing else reaches 0.8 of it: a condition,
                  not a measurement -- it is what turns a wrong frame or bin into a 20 % miss of a 1e-4 bar
  lengths         the hand-set N_k tables reach every snapshot position and lane split of cqt_blocks_kernel
  instantiations  the MFMA cases run exactly the 14 (Q, R) pairs cqt_max_mfma_kernel is built for
"""
import numpy as np
import pytest

import cqt_reference as R
from oracle import cqt as ocqt

RUNNER_UP = 0.8


@pytest.mark.parametrize('case', R.MAX_CASES, ids=R.MAX_CASE_IDS)
def test_targeting_premise(case):
    inc, length = R.case_grid(case)
    assert int(length.max()) < 1000                   # short filters: N_k of a few hundred samples
    waves = R.case_waves(case)
    assert waves.dtype == np.float32 and waves.shape == (len(case['targets']), case['L'])
    for (k, t), x in zip(case['targets'], waves):
        C = R.all_frames(x, inc, length, case['hop'])
        assert C.shape == (case['n_bins'], case['T'])
        assert np.unravel_index(np.argmax(C), C.shape) == (k, t), (case['name'], k, t)
        peak = C[k, t]
        C[k, t] = 0.0
        assert C.max() <= RUNNER_UP * peak, (case['name'], k, t, C.max() / peak)


def test_all_frames_agrees_with_the_window_maximum():
    for name in ('q1r1', 'hop128_edges'):
        case = R.MAX_CASES[R.MAX_CASE_IDS.index(name)]
        inc, length = R.case_grid(case)
        for b in (0, len(case['targets']) - 1):
            x = R.case_waves(case)[b]
            want = ocqt.cqt_window_max(x, inc, length, case['hop'])
            assert abs(R.all_frames(x, inc, length, case['hop']).max() - want) <= 1e-12 * want


def test_target_lists_cover_the_edges():
    by = {c['name']: c for c in R.MAX_CASES}
    for hop in R.HOPS:
        c = by['hop%d_edges' % hop]
        assert ('mfma' in c['forms']) == (hop != 128) and 'valu' in c['forms']
        frames = {t for _, t in c['targets']}
        assert {0, 1, 15, 16, 17, 127, 128, c['T'] - 2, c['T'] - 1} <= frames
        bins = {k for k, _ in c['targets']}
        assert set(range(7)) <= bins and c['n_bins'] - 1 in bins
    assert {by['hop%d_edges' % h]['n_bins'] % 7 for h in R.HOPS} == {1, 6}        # ragged last groups of 1 and of 6 bins
    # the wave-3 frames: every case with T > 512 aims at 511, 512 and T - 1, at bin positions 0 and 6
    for name in ('q4r1', 'q4r2', 'q4r0_T513'):
        c = by[name]
        tg = set(c['targets'])
        for f in (511, 512, c['T'] - 1):
            assert (0, f) in tg and (6, f) in tg, (name, f)
    assert {(0, 513), (6, 513)} <= set(by['q4r2']['targets'])
    assert by['q4r0_T513']['L'] == 512 * 256 and by['q4r0_T513']['T'] == 513
    assert by[R.SCALED_CASE]['T'] > 513


def test_length_tables_cover_every_snapshot_position():
    for H in R.HOPS:
        cases = R.length_cases(H)
        assert tuple(cases) == R.LENGTH_CASE_NAMES
        alln = np.concatenate(list(cases.values()))
        assert all(len(v) <= 16 and v.dtype == np.int32 for v in cases.values())
        assert set(int(n) % 32 for n in alln) == set(range(32))                  # 4 groups x 8 cm_group cases
        # the residues in both r32 tables alone, at more than one lane split (N_k mod H) >> 5
        r32 = np.concatenate([cases['r32_lo'], cases['r32_hi']])
        assert sorted(int(n) % 32 for n in r32) == list(range(32))
        assert len({(int(n) % H) >> 5 for n in r32}) >= 3
        assert {0, 1, 31, 32, 33, H - 1} <= set(int(n) % H for n in alln)
        assert {2, 31, H - 1, H} <= set(int(n) for n in alln)                     # below a lane's run, below and at the hop
        assert any(int(n) % 2 for n in alln) and any(int(n) % H == 0 and n > H for n in alln)
        assert int(alln.max()) > R.SHORT_L                                        # N_k > L at the short signal
        # the lengths: one pass of the workgroup, a block less, a block more; and below one staging run
        pass_blocks = 4 * 64 // (H // 32)
        Ls = R.sweep_lengths(H)
        assert [-(-L // H) for L in Ls[:3]] == [pass_blocks - 1, pass_blocks, pass_blocks + 1] and Ls[3] < 2048
    for frames in (1, 3, 8):
        for T in (1, 2, 4, 7, 65):
            fs = R.frame_sets(T, frames)
            assert fs.shape[1] == frames and fs.min() >= -1 and fs.max() == T - 1 and (fs == 0).any() and (fs == -1).any()
    fs = R.frame_sets(65, 8)
    assert any(len(set(r[r >= 0])) < (r >= 0).sum() for r in fs)                 # a duplicate
    assert (np.diff(fs[0]) == 1).all() and (np.diff(fs[1]) > 1).all()            # a compact run, a spread set


def test_mfma_cases_are_the_built_instantiations():
    shapes = {(q, r) for q in range(5) for r in range(3)} - {(0, 0)}
    assert len(shapes) == 14 and set(R.QR_BLOCKS) == shapes
    for (q, r), nblk in R.QR_BLOCKS.items():
        assert R.cqm_geometry(nblk * 256, 256) == (q, r)
        assert nblk == 1 or R.cqm_geometry((nblk - 1) * 256, 256) != (q, r)      # the shortest of the pair
    ran = {}
    for c in R.MAX_CASES:
        if 'mfma' in c['forms']:
            assert -(-c['L'] // c['hop']) <= 544
            ran.setdefault(R.cqm_geometry(c['L'], c['hop']), []).append(c['name'])
    assert set(ran) == shapes, ran
    for qr in R.NEVER_RUN_BEFORE:
        assert any(n == 'q%dr%d' % qr for n in ran[qr])
    for (q, r), nblk in R.QR_BLOCKS.items():
        c = R.MAX_CASES[R.MAX_CASE_IDS.index('q%dr%d' % (q, r))]
        assert c['hop'] == 256 and -(-c['L'] // 256) == nblk
    assert R.cqm_geometry(R.REFUSED_L, 256) is None and R.cqm_geometry(544 * 256, 256) == (4, 2)
    assert R.cqm_geometry(145 * 128, 128) is None and R.cqm_geometry(145 * 4096, 4096) is None
    for hop in (512, 1024, 2048):
        assert R.cqm_geometry(545 * hop, hop) is None
