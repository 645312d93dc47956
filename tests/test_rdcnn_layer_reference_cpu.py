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
