"""Window-major small-image form of the split-fp16 4 x 16 convolution (conv_f16x3w_kernel): parity against the oracle,
the SAME BITS as the masked form it replaces (a net created under AMT_CONV_WMAJOR=0), batch independence over groups of
16 windows that are empty, partial, exact and crossed, and per-window operand scaling.

Shallow nets whose six conv layers all run on the small image: 1 -> 32, 32 -> 32 (rank-1 shortcut), 32 -> 64,
64 -> 64 (projected shortcut), 64 -> 128, 128 -> 128 (projected shortcut)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-4           # the bars of test_gpu_rdcnn._check_head
SHAPES = [(5, 8),    # the workload's tail image
          (5, 4),    # the N = 4096 tail
          (3, 5),    # fewer rows than taps
          (8, 8),    # the H * W = 64 boundary
          (7, 9)]    # odd sizes
NB = 37


def _inputs(shape, B, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((B,) + tuple(shape)) ** 2).astype(np.float32)


def _net(shape, masked_form):
    """A mode-2 net; masked_form: its eligible layers keep the masked kernel.  The switch is read when the native net is
    created -- on first use, here by the flops_per_window property."""
    from amt_saga import rdcnn
    net = rdcnn.res_net(input_shapes=[tuple(shape) + (1,)], output_classes=3, output_range=[3, 40],
                        kernel_sizes=[(4, 16)], pool_sizes=[(2, 2)], convolutional_layer_count=6,
                        feature_expand_frequency=2, pool_layer_frequency=0, residual_layer_frequencies=2,
                        weight_seed=77)
    old = os.environ.get('AMT_CONV_WMAJOR')
    try:
        if masked_form:
            os.environ['AMT_CONV_WMAJOR'] = '0'
        else:
            os.environ.pop('AMT_CONV_WMAJOR', None)
        net.set_mode(2)
        assert net.flops_per_window > 0
    finally:
        if old is None:
            os.environ.pop('AMT_CONV_WMAJOR', None)
        else:
            os.environ['AMT_CONV_WMAJOR'] = old
    return net


@pytest.fixture(scope='module')
def state():
    """Per shape: the window-major net, the 37 windows, and their logits inside the full batch (computed once)."""
    import torch
    assert torch.cuda.is_available()
    from amt_saga import _lib
    _lib.load()
    out = {}
    for i, shape in enumerate(SHAPES):
        net = _net(shape, False)
        x = torch.from_numpy(_inputs(shape, NB, 100 + i)).cuda()
        y, lg = net.predict_device([x], return_logits=True)
        out[shape] = dict(net=net, x=x, y=y, lg=lg)
    return out


@pytest.mark.parametrize('shape', SHAPES)
def test_parity_against_oracle(state, shape):
    from oracle import rdcnn as orc
    net = state[shape]['net']
    cfg = net.cfg
    assert [tuple(s) for s in cfg['input_shapes']] == [tuple(shape) + (1,)]
    x = state[shape]['x'][:6].contiguous()
    xo = [x.cpu().numpy()[..., None]]
    ref_lg = orc.forward(net.weights, cfg, xo, np.float32, return_logits=True)
    ref = orc.forward(net.weights, cfg, xo, np.float32)
    ref_lg64 = orc.forward(net.weights, cfg, xo, np.float64, return_logits=True)
    y, lg = net.predict_device([x], return_logits=True)
    y, lg = y.cpu().numpy(), lg.cpu().numpy()
    scale = max(np.abs(ref_lg).max(), 1.0)
    e_gpu = float(np.abs(lg - ref_lg64).max())
    e_cpu = float(np.abs(ref_lg - ref_lg64).max())
    print('shape %s: |lg - f32| %.3g  e_gpu %.3g  e_cpu %.3g  scale %.3g' % (shape, np.abs(lg - ref_lg).max(), e_gpu, e_cpu, scale))
    assert np.abs(lg - ref_lg).max() / scale < REL
    assert np.abs(y - ref).max() / max(np.abs(ref).max(), 1e-30) < REL
    assert e_gpu <= 2.5 * e_cpu + 2.4e-7 * scale, (shape, e_gpu, e_cpu)


@pytest.mark.parametrize('shape', SHAPES)
def test_same_bits_as_masked_form(state, shape):
    """Results stayed what they were: the reference is the masked kernel."""
    import torch
    old = _net(shape, True)
    y_old, lg_old = old.predict_device([state[shape]['x']], return_logits=True)
    assert torch.equal(lg_old, state[shape]['lg'])
    assert torch.equal(y_old, state[shape]['y'])


@pytest.mark.parametrize('shape', SHAPES)
def test_batch_independence(state, shape):
    """Batches of 1, 15, 16, 17 and 37 windows: a group of 16 that is empty, partial, exact and crossed."""
    import torch
    s = state[shape]
    net, x, lg = s['net'], s['x'], s['lg']
    assert torch.isfinite(lg).all()
    for sl in (slice(5, 12), slice(36, 37), slice(0, 1), slice(0, 15), slice(3, 19), slice(20, 37)):
        _, l2 = net.predict_device([x[sl].contiguous()], return_logits=True)
        assert torch.equal(l2, lg[sl]), (shape, sl)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(NB)).cuda()
    _, lp = net.predict_device([x[perm].contiguous()], return_logits=True)
    assert torch.equal(lp, lg[perm])
    _, again = net.predict_device([x], return_logits=True)
    assert torch.equal(again, lg)


@pytest.mark.parametrize('shape', SHAPES)
def test_per_window_scaling(state, shape):
    """One window x 1e6, one x 1e-6 and one all-zero inside the 37 leave the other windows' bits unchanged."""
    import torch
    s = state[shape]
    x2 = s['x'].clone()
    x2[3] *= 1e6
    x2[17] *= 1e-6
    x2[30] = 0
    y2, l2 = s['net'].predict_device([x2], return_logits=True)
    assert torch.isfinite(l2).all() and torch.isfinite(y2).all()
    keep = torch.ones(NB, dtype=torch.bool, device=l2.device)
    keep[[3, 17, 30]] = False
    assert torch.equal(l2[keep], s['lg'][keep])
