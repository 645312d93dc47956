"""CPU: the per-layer restatement (tests/rdcnn_layer_reference.py), chained over a whole net, gives the logits of
oracle.rdcnn.forward at the same dtype -- so the reference the GPU layers are judged against is the oracle's, step by step."""
import numpy as np
import pytest

import rdcnn_layer_reference as lr
from oracle import rdcnn as orc

BY_NAME = {c['name']: c for c in lr.CASES}
# a pooled 4 x 2 net with an average-pooled projected shortcut, an unpooled 4 x 16 net with shortcuts every third layer
# (rank-1 candidate, identity), and the two-tower net (2 x 2 second tower, concatenated dense input)
CHAINED = ['12x10 k4x2', '10x40 k4x16', 'two towers']


def test_case_names_unique():
    assert len(BY_NAME) == len(lr.CASES)


@pytest.mark.parametrize('name', CHAINED)
def test_chained_steps_equal_oracle_forward(name):
    case = BY_NAME[name]
    net = lr.case_net(case)
    lr.assert_weights_not_identity(net.weights)
    xs = lr.case_inputs(case, 5)
    assert all(np.abs(x[4]).max() == 0 and x[2].max() > 1 for x in xs)
    xo = [x[..., None] for x in xs]
    L = net.cfg['convolutional_layer_count']
    for dtype in (np.float64, np.float32):
        ref = orc.forward(net.weights, net.cfg, xo, dtype, return_logits=True)
        lg, blocks = lr.chain(net.weights, net.cfg, xo, dtype)
        assert lg.dtype == dtype and ref.dtype == dtype
        assert lg.shape == (case['B'], case['K'])
        assert np.array_equal(lg, ref), (name, dtype, np.abs(lg - ref).max())
        assert [len(b) for b in blocks] == [L] * len(xs)
        assert all(a.dtype == dtype for b in blocks for a in b)


def test_every_case_builds_and_has_live_parameters():
    for case in lr.CASES:
        net = lr.case_net(case)
        lr.assert_weights_not_identity(net.weights)
        assert not net.calibrated


# ---- conv mode 3 (tests/test_gpu_rdcnn_fft_layers.py): the composed and the pooled-pair references, the case table ----
FFT_BY_NAME = {c['name']: c for c in lr.FFT_CASES}
# a W-pooled layer read by the max pool only (ragged W), one read by a pooled projected shortcut too, hand-over runs of
# two layers without a shortcut, and two towers of 4 x 16 layers
FFT_CHAINED = ['fft 3x17 L4', 'fft 5x24 L6', 'fft 9x72 r1', 'fft 6x25 r0 L4', 'fft two towers']


def test_fft_case_names_unique():
    assert len(FFT_BY_NAME) == len(lr.FFT_CASES)


def test_fft_case_cfg_is_the_nets():
    for case in lr.FFT_CASES:
        cfg = lr.case_net(case).cfg
        assert {k: cfg[k] for k in lr.case_cfg(case)} == lr.case_cfg(case), case['name']


@pytest.mark.parametrize('name', FFT_CHAINED)
def test_fft_composed_and_pooled_references_equal_oracle_forward(name):
    """The walk of the mode-3 test over its own references -- tapped tensors replaced by the reference's, a hand-over run
    composed by run_steps, a W-pooled layer replaced by its pooled pair, read by next_input and shortcut_tensor -- ends
    in the logits of oracle.rdcnn.forward, array_equal in float64 and in float32.  Only where the means of a pooled pair
    feed a shortcut projection (8 columns first, then the projection and the rows: another order of the same sum) the
    logits are held to 1e-12 (float64) and 1e-5 (float32) of their scale instead."""
    case = FFT_BY_NAME[name]
    net = lr.case_net(case)
    cfg, w = net.cfg, net.weights
    xs = lr.case_inputs(case, 5)
    xo = [x[..., None] for x in xs]
    plans = lr.model_fc_plans(cfg, case['B'])
    L = cfg['convolutional_layer_count']
    for dtype in (np.float64, np.float32):
        ref = orc.forward(w, cfg, xo, dtype, return_logits=True)
        flats, two_step_mean = [], False
        for t, x in enumerate(xo):
            tapped = {0: np.asarray(x, dtype)}                       # what a later layer may read as its shortcut source
            start, x_in = 1, tapped[0]
            for i in range(1, L + 1):
                p = plans[t][i - 1]
                if not (p['writes_spatial'] or p['wpooled']):
                    continue                                         # exists only transformed: part of the run
                src = {i: tapped[lr.shortcut_source(cfg, i)]} if lr.closes_shortcut(cfg, i) else {}
                two_step_mean |= bool(src) and lr.shortcut_source(cfg, i) > 0 and plans[t][lr.shortcut_source(cfg, i) - 1]['wpooled']
                out = lr.run_steps(w, cfg, t, start, i, x_in, src, dtype)
                assert out.dtype == dtype
                if p['wpooled']:
                    wavg, wmax = lr.pooled_pair(out)
                    assert np.array_equal(wmax, orc.pool2d(out, (1, 8), 'max')) and np.array_equal(wavg, orc.pool2d(out, (1, 8), 'avg'))
                    W8 = p['W'] // 8
                    assert wmax.shape[2] == W8 and np.array_equal(wmax[:, :, -1], out[:, :, 8 * W8 - 8:8 * W8].max(axis=2))
                    assert np.array_equal(wavg[:, :, 0], out[:, :, :8].mean(axis=2))
                    out = np.stack([wavg, wmax])
                    assert np.array_equal(lr.next_input(cfg, t, i, out, p), lr.layer_input(cfg, t, i + 1, lr.run_steps(
                        w, cfg, t, start, i, x_in, src, dtype)))
                tapped[i] = lr.shortcut_tensor(out, p)
                start, x_in = i + 1, lr.next_input(cfg, t, i, out, p)
            assert start == L + 1                                    # the last layer always leaves something to tap
            flats.append(x_in)
        lg = lr.dense_step(w, flats, dtype)
        if two_step_mean:
            tol = 1e-12 if dtype == np.float64 else 1e-5
            assert np.abs(lg - ref).max() <= tol * max(np.abs(ref).max(), 1.0), (name, dtype, np.abs(lg - ref).max())
        else:
            assert np.array_equal(lg, ref), (name, dtype, np.abs(lg - ref).max())


def test_fft_case_table_covers_every_family_by_the_plan_model():
    """The coverage logic of the mode-3 test on the plans the topology rules predict (no device: the library's own
    report is held to the same model, and to the same families, in tests/test_gpu_rdcnn_fft_layers.py)."""
    rows = [(case, p) for case in lr.FFT_CASES for plans in lr.model_fc_plans(lr.case_cfg(case), case['B']) for p in plans]
    hit = lr.fft_families(rows)
    missing = [f for f in lr.FFT_REQUIRED if f not in hit]
    assert not missing, missing
    # the rules, on the nets whose forms test_gpu_pooled_epilogue.py describes in words
    p4 = lr.model_fc_plans(lr.case_cfg(FFT_BY_NAME['fft 20x44 L4']), 7)[0]
    assert [p['form'] for p in p4] == ['none', 'row', 'row', 'row']
    assert [p['shortcut'] for p in p4] == [None, 'rank1', 'none', 'tensor']
    assert [p['hands_on'] for p in p4] == [False, True, True, False] and [p['have_xf'] for p in p4] == [False, False, True, True]
    assert [p['writes_spatial'] for p in p4] == [True, True, False, False] and p4[3]['wpooled']
    pk = lr.model_fc_plans(lr.case_cfg(FFT_BY_NAME['fft packed 10x64 L4']), 5)[0]
    assert [p['form'] for p in pk] == ['none', 'row', 'none', 'packed'] and pk[3]['wpooled'] and pk[3]['shortcut'] == 'projected'
    assert lr.gemm_chunks_per_wg(112) == 1 and lr.gemm_chunks_per_wg(113) == 2 and lr.gemm_chunks_per_wg(120) == 2
