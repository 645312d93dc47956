"""W-pooled epilogue of the FFT-domain forms (fc_row_kernel and pk_row_kernel, EPI = 5): the last 4 x 16 layer in front
of a max pool (ph, 8) leaves max and mean over 8 columns instead of its full-size output, and the max pool and the pooled
shortcut projection of the next block run on those.

  * where only the max pool reads the output, the SAME BITS as the full-size path (a net created under AMT_FC_POOLED=0);
  * with the pooled projected shortcut (the 16-term average is summed in another order), the bars of
    test_gpu_rdcnn._check_head against the oracle; the largest |new - old-path| logit difference per shape is printed
    and recorded in profiles/r06/README.md -- it has no threshold of its own;
  * the fall-backs (a shortcut pool that is not the max pool's window; a pool other than (ph, 8)) keep the old path;
  * the packed-image form (10 x 64, 64 -> 64) under the same two checks;
  * batch independence and per-window operand scaling, bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-4           # the bars of test_gpu_rdcnn._check_head
NB = 37
SHAPES4 = [(20, 44),   # W % 8 = 4, as 516
           (5, 24),    # H odd, W a multiple of 8, one n1 block
           (4, 561),   # the widest row the form accepts
           (3, 17)]    # fewer rows than taps
SHAPES6 = [(20, 44), (5, 24), (3, 17)]
PACKED = (10, 64)    # with feature_expand_frequency = 2, layer 4 is the 64 -> 64 packed-image layer, pooled


def _inputs(shape, B, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((B,) + tuple(shape)) ** 2).astype(np.float32)


def _net(shape, layers, old_path=False, pool=(2, 8), expand=4):
    """A mode-3 net; old_path: created under AMT_FC_POOLED=0.  The switch is read when the native net is created -- on
    first use, here by the fc_pooled_layers property."""
    from amt_saga import rdcnn
    net = rdcnn.res_net(input_shapes=[tuple(shape) + (1,)], output_classes=3, output_range=[3, 40],
                        kernel_sizes=[(4, 16)], pool_sizes=[pool], convolutional_layer_count=layers,
                        feature_expand_frequency=expand, pool_layer_frequency=4, residual_layer_frequencies=2,
                        weight_seed=91)
    old = os.environ.get('AMT_FC_POOLED')
    try:
        if old_path:
            os.environ['AMT_FC_POOLED'] = '0'
        else:
            os.environ.pop('AMT_FC_POOLED', None)
        net.set_mode(3)
        n = net.fc_pooled_layers
        assert n == 0 or not old_path
    finally:
        if old is None:
            os.environ.pop('AMT_FC_POOLED', None)
        else:
            os.environ['AMT_FC_POOLED'] = old
    return net


def _seed(shape, layers):
    return 1000 * layers + 10 * shape[0] + shape[1] % 7


@pytest.fixture(scope='module')
def state():
    """Per (shape, layers): both nets, the 37 windows and both paths' results on the full batch (computed once)."""
    import torch
    assert torch.cuda.is_available()
    from amt_saga import _lib
    _lib.load()
    out = {}
    for layers, shapes in ((4, SHAPES4), (6, SHAPES6)):
        for shape in shapes:
            new, old = _net(shape, layers), _net(shape, layers, old_path=True)
            x = torch.from_numpy(_inputs(shape, NB, _seed(shape, layers))).cuda()
            y, lg = new.predict_device([x], return_logits=True)
            y_old, lg_old = old.predict_device([x], return_logits=True)
            out[(shape, layers)] = dict(net=new, old=old, x=x, y=y, lg=lg, y_old=y_old, lg_old=lg_old)
    for layers in (4, 6):
        new, old = _net(PACKED, layers, expand=2), _net(PACKED, layers, old_path=True, expand=2)
        x = torch.from_numpy(_inputs(PACKED, NB, _seed(PACKED, layers))).cuda()
        y, lg = new.predict_device([x], return_logits=True)
        y_old, lg_old = old.predict_device([x], return_logits=True)
        out[('packed', layers)] = dict(net=new, old=old, x=x, y=y, lg=lg, y_old=y_old, lg_old=lg_old)
    return out


@pytest.mark.parametrize('shape', SHAPES4)
def test_same_bits_where_only_the_max_pool_reads(state, shape):
    """Four layers: layer 4 is FFT-form with an identity shortcut, pooled, and last.  Max is order-independent."""
    import torch
    s = state[(shape, 4)]
    assert s['net'].fc_pooled_layers == 1 and s['old'].fc_pooled_layers == 0
    assert torch.isfinite(s['lg']).all()
    assert torch.equal(s['lg'], s['lg_old'])
    assert torch.equal(s['y'], s['y_old'])


def test_packed_same_bits_where_only_the_max_pool_reads(state):
    """Four layers on 10 x 64: 1 -> 32, 32 -> 32, 32 -> 64, and the packed 64 -> 64 layer with a projected shortcut
    tensor, pooled, and last."""
    import torch
    s = state[('packed', 4)]
    assert s['net'].fc_pooled_layers == 1 and s['old'].fc_pooled_layers == 0
    assert torch.isfinite(s['lg']).all()
    assert torch.equal(s['lg'], s['lg_old'])
    assert torch.equal(s['y'], s['y_old'])


@pytest.mark.parametrize('shape', SHAPES6 + ['packed'])
def test_pooled_projected_shortcut_against_oracle(state, shape):
    """Six layers: layer 6 closes a shortcut from layer 4's output, served from the pooled means."""
    from oracle import rdcnn as orc
    s = state[(shape, 6)]
    net = s['net']
    assert net.fc_pooled_layers == 1 and s['old'].fc_pooled_layers == 0
    cfg = net.cfg
    x = s['x'][:6].contiguous()
    xo = [x.cpu().numpy()[..., None]]
    ref_lg = orc.forward(net.weights, cfg, xo, np.float32, return_logits=True)
    ref = orc.forward(net.weights, cfg, xo, np.float32)
    ref_lg64 = orc.forward(net.weights, cfg, xo, np.float64, return_logits=True)
    y, lg = net.predict_device([x], return_logits=True)
    y, lg = y.cpu().numpy(), lg.cpu().numpy()
    scale = max(np.abs(ref_lg).max(), 1.0)
    e_gpu = float(np.abs(lg - ref_lg64).max())
    e_cpu = float(np.abs(ref_lg - ref_lg64).max())
    d_old = float((s['lg'] - s['lg_old']).abs().max())
    e_old = float(np.abs(s['lg_old'][:6].cpu().numpy() - ref_lg64).max())
    print('shape %s: max |new - old path| logit %.3g (37 windows); |lg - f32| %.3g  e_gpu %.3g (old path %.3g)  e_cpu %.3g  '
          'scale %.3g' % (shape, d_old, np.abs(lg - ref_lg).max(), e_gpu, e_old, e_cpu, scale))
    assert np.abs(lg - ref_lg).max() / scale < REL
    assert np.abs(y - ref).max() / max(np.abs(ref).max(), 1e-30) < REL
    assert e_gpu <= 2.5 * e_cpu + 2.4e-7 * scale, (shape, e_gpu, e_cpu)


@pytest.mark.parametrize('shape,pool', [((6, 20), (2, 8)),     # the shortcut's average pool is (3, 10): not the max pool's
                                        ((20, 44), (2, 2))])   # no pool over 8 columns
def test_fallbacks_keep_the_old_path(shape, pool):
    import torch
    new, old = _net(shape, 6, pool=pool), _net(shape, 6, old_path=True, pool=pool)
    assert new.fc_pooled_layers == 0
    x = torch.from_numpy(_inputs(shape, NB, 7)).cuda()
    y, lg = new.predict_device([x], return_logits=True)
    y_old, lg_old = old.predict_device([x], return_logits=True)
    assert torch.isfinite(lg).all()
    assert torch.equal(lg, lg_old) and torch.equal(y, y_old)


@pytest.mark.parametrize('layers', [4, 6])
def test_batch_independence(state, layers):
    """Slices of the 37 windows, a permutation and a re-run on (20, 44)."""
    import torch
    s = state[((20, 44), layers)]
    net, x, lg = s['net'], s['x'], s['lg']
    assert torch.isfinite(lg).all()
    for sl in (slice(5, 12), slice(36, 37), slice(0, 1), slice(0, 15), slice(3, 19), slice(20, 37)):
        _, l2 = net.predict_device([x[sl].contiguous()], return_logits=True)
        assert torch.equal(l2, lg[sl]), sl
    perm = torch.from_numpy(np.random.default_rng(0).permutation(NB)).cuda()
    _, lp = net.predict_device([x[perm].contiguous()], return_logits=True)
    assert torch.equal(lp, lg[perm])
    _, again = net.predict_device([x], return_logits=True)
    assert torch.equal(again, lg)


@pytest.mark.parametrize('layers', [4, 6])
def test_per_window_scaling(state, layers):
    """One window x 1e6, one x 1e-6 and one all-zero inside the 37 leave the other windows' bits unchanged."""
    import torch
    s = state[((20, 44), layers)]
    x2 = s['x'].clone()
    x2[3] *= 1e6
    x2[17] *= 1e-6
    x2[30] = 0
    y2, l2 = s['net'].predict_device([x2], return_logits=True)
    assert torch.isfinite(l2).all() and torch.isfinite(y2).all()
    keep = torch.ones(NB, dtype=torch.bool, device=l2.device)
    keep[[3, 17, 30]] = False
    assert torch.equal(l2[keep], s['lg'][keep])
