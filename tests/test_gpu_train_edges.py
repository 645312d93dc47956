"""GPU parity of the training step at the edges tests/test_gpu_train.py leaves out:
where shortcuts, pools and channel doublings fall relative to each other (the gradient hand-over), unequal
towers, the shape edges of the weight gradient without im2col, every combination of the three path switches, Adagrad
element for element, the product heads no other test trains, and a batch of one.  Same reference (oracle/train.py, pinned
to PyTorch autograd over these very graphs in tests/test_oracle_train.py) and the same bars as tests/test_gpu_train.py,
whose _compare_step does the comparing."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_oracle_train import CASES, TOPOLOGY_EDGES, WGRAD_WIDTH_EDGES, WGRAD_CHANNEL_EDGE      # noqa: E402
from test_gpu_train import _batch, _opt, _to_act, _compare_step                                   # noqa: E402

SWITCHES = ('AMT_TRAIN_FAST', 'AMT_TRAIN_WGRAD', 'AMT_TRAIN_FUSED_BN')
TRIPLES = {'keras-2.2': (0.01, 1e-7, 0.0), 'tf.keras-1.14': (0.001, 1e-7, 0.1)}


class _OracleOnce:
    """oracle.train with each distinct call computed once: a graph is trained under several environments from the same
    weights and batch, and every one of those runs asks the oracle the same questions.  Keyed by the content of the
    arguments; the results are shared and nobody writes into them."""

    def __init__(self, otr):
        self._otr, self._memo = otr, {}

    @staticmethod
    def _key(*parts):
        h = hashlib.sha1()
        for p in parts:
            if isinstance(p, dict):
                for k in sorted(p):
                    h.update(k.encode())
                    h.update(np.ascontiguousarray(p[k]).tobytes() if isinstance(p[k], np.ndarray) else repr(p[k]).encode())
            elif isinstance(p, (list, tuple)) and p and isinstance(p[0], np.ndarray):
                for a in p:
                    h.update(np.ascontiguousarray(a).tobytes())
            elif isinstance(p, np.ndarray):
                h.update(np.ascontiguousarray(p).tobytes())
            else:
                h.update(repr(p).encode())
            h.update(b'|')
        return h.hexdigest()

    def forward_backward(self, w, cfg, xs, y, dtype=np.float64):
        k = self._key('fb', w, cfg, xs, np.asarray(y), np.dtype(dtype).name)
        if k not in self._memo:
            self._memo[k] = self._otr.forward_backward(w, cfg, xs, y, dtype)
        return self._memo[k]

    def train_on_batch(self, w, cfg, xs, y, acc=None, lr=0.01, eps=1e-7, dtype=np.float32, initial_accumulator=0.1):
        k = self._key('tob', w, cfg, xs, np.asarray(y), acc or {}, lr, eps, np.dtype(dtype).name, initial_accumulator)
        if k not in self._memo:
            self._memo[k] = self._otr.train_on_batch(w, cfg, xs, y, acc=acc, lr=lr, eps=eps, dtype=dtype,
                                                     initial_accumulator=initial_accumulator)
        return self._memo[k]


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available()
    from amt_saga import rdcnn, heads, hyperparams
    from oracle import train as otr, rdcnn as orc
    return dict(torch=torch, rdcnn=rdcnn, heads=heads, hp=hyperparams, otr=_OracleOnce(otr), orc=orc)


def _set_env(monkeypatch, fast_min_m=None, off=()):
    """The trainer reads its switches when it is created (the first train()): set them before that."""
    for k in SWITCHES:
        if k in off:
            monkeypatch.setenv(k, '0')
        else:
            monkeypatch.delenv(k, raising=False)
    if fast_min_m is None:
        monkeypatch.delenv('AMT_TRAIN_FAST_MIN_M', raising=False)
    else:
        monkeypatch.setenv('AMT_TRAIN_FAST_MIN_M', str(fast_min_m))


def _edge_batch(cfg, B, seed):
    """_batch, with class 0 and class K - 1 both among the labels of a multi-class graph (K - 1 alone in a batch of one)."""
    xs, y = _batch(cfg, B, seed)
    K = cfg['output_classes']
    if K > 1:
        y[0], y[-1] = 0, K - 1
    return xs, y


def _one(xs):
    return xs if len(xs) > 1 else xs[0]


def _copy(w):
    return {k: v.copy() for k, v in w.items()}


def _gradient_ratio(env, net, w_before, xs, y):
    """Worst (error / bar) over the tensors, with _compare_step's gradient bar, of the step that just ran (a figure to
    print: _compare_step has already asserted it)."""
    grads = net.gradients()
    _, _, g32, _ = env['otr'].forward_backward(w_before, net.cfg, xs, _to_act(net, y), np.float32)
    _, _, g64, _ = env['otr'].forward_backward(w_before, net.cfg, xs, _to_act(net, y), np.float64)
    gmax = max(np.abs(v).max() for v in g64.values())
    return max(np.abs(grads[k] - gk).max() / (3e-4 * np.abs(gk).max() + 4 * np.abs(g32[k] - gk).max() + 1e-7 * gmax)
               for k, gk in g64.items())


def _assert_per_tap(env, net, w_before, xs, y, tag):
    """Every (dy, dx) slice s of every convolution kernel's gradient on its own:
        |dev - f64| <= 3e-4 max|s64| + 4 max|f32 oracle - f64 oracle| over s + 1e-6 max|tensor64|.
    The first two terms are _compare_step's bar applied to the slice.  The last is the split-fp16 floor: two fp16 planes
    keep about 22 bits of the window's operand scale, so the absolute error follows the tensor, not the tap
    (4 * 2^-22 ~ 1e-6).  A tap whose row is wholly padding (H = 1: every dy but one) has a float64 gradient of exactly
    zero and is held by that last term alone.  Returns the worst error / bar."""
    grads = net.gradients()
    _, _, g32, _ = env['otr'].forward_backward(w_before, net.cfg, xs, _to_act(net, y), np.float32)
    _, _, g64, _ = env['otr'].forward_backward(w_before, net.cfg, xs, _to_act(net, y), np.float64)
    worst = 0.0
    for k, gk in g64.items():
        if not k.endswith('/kernel') or gk.ndim != 4:
            continue
        floor = 1e-6 * np.abs(gk).max()
        for dy in range(gk.shape[0]):
            for dx in range(gk.shape[1]):
                s = gk[dy, dx]
                err = np.abs(grads[k][dy, dx] - s).max()
                bar = 3e-4 * np.abs(s).max() + 4 * np.abs(g32[k][dy, dx] - s).max() + floor
                assert err <= bar, (tag, k, dy, dx, err, bar, np.abs(s).max(), np.abs(gk).max())
                worst = max(worst, err / bar)
    return worst


# ---- topology rules: where shortcuts, pools and doublings fall ---------------------------------------------------------
TOPOLOGY_RUNS = [(i, 3) for i in range(len(TOPOLOGY_EDGES))] + [(3, 1)]


@pytest.mark.parametrize('fast_small', (False, True), ids=('default', 'fast-min-m-0'))
@pytest.mark.parametrize('case,B', TOPOLOGY_RUNS, ids=['graph%d-B%d' % cb for cb in TOPOLOGY_RUNS])
def test_topology_edge_train_step_vs_oracle(env, case, B, fast_small, monkeypatch):
    """One train() on each graph of TOPOLOGY_EDGES (tests/test_oracle_train.py says what each reaches) against the
    oracle: once as the product runs such small layers (GEMM forms) and once with every covered layer on the split-fp16
    kernels and the direct weight gradient.  Then test() -- the inference-mode forward over the moving statistics the
    step just updated -- on a second batch against oracle.rdcnn.forward.  Graph 3 also with a batch of one: each
    BatchNormalization then sees the H W positions of one window (6 for the last layer), bessel = M / (M - 1)."""
    _set_env(monkeypatch, 0 if fast_small else None)
    net = env['rdcnn'].res_net(weight_seed=331 + case, calibrated=False, **TOPOLOGY_EDGES[case])
    net.keras_optimizer_version = 'keras-2.2' if case % 2 == 0 else 'tf.keras-1.14'
    assert _opt(net) == TRIPLES[net.keras_optimizer_version]
    xs, y = _edge_batch(net.cfg, B, 600 + case)
    w0 = _copy(net.weights)
    tag = 'graph %d B %d %s' % (case, B, 'fast' if fast_small else 'default')
    _compare_step(env, net, xs, y, w0, None, tag)
    print('%s: worst gradient error / bar = %.3f' % (tag, _gradient_ratio(env, net, w0, xs, y)))
    net._sync_from_trainer()
    w_now = _copy(net.weights)
    xs2, y2 = _edge_batch(net.cfg, B, 700 + case)
    pred = net.test(_one(xs2), y2)
    ref = env['orc'].forward(w_now, net.cfg, xs2, np.float32)
    assert pred.shape == ref.shape
    assert np.abs(pred - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-6), tag


# ---- shape edges of the weight gradient without im2col -----------------------------------------------------------------
WIDTH_RUNS = [(i, B) for i in range(len(WGRAD_WIDTH_EDGES)) for B in (1, 3)]


def _wgrad_edge_step(env, kw, B, seed, tag, monkeypatch):
    _set_env(monkeypatch, 0)
    net = env['rdcnn'].res_net(weight_seed=seed, calibrated=False, **kw)
    xs, y = _edge_batch(net.cfg, B, seed + 1)
    w0 = _copy(net.weights)
    _compare_step(env, net, xs, y, w0, None, tag)
    print('%s: worst per-tap gradient error / bar = %.3f, per tensor = %.3f'
          % (tag, _assert_per_tap(env, net, w0, xs, y, tag), _gradient_ratio(env, net, w0, xs, y)))


@pytest.mark.parametrize('case,B', WIDTH_RUNS,
                         ids=['%dx%d-B%d' % (WGRAD_WIDTH_EDGES[i]['input_shapes'][0][:2] + (B,)) for i, B in WIDTH_RUNS])
def test_direct_wgrad_width_and_height_edges(env, case, B, monkeypatch):
    """wgrad_kernel's segmenting on a two-layer 4 x 16 net (the 32 -> 32 layer takes it): W = 16 is the smallest width it
    accepts (and with H = B = 1 there is one tile for the partial slots); W = 17 is odd (the k-step pair past the end is
    zero-filled); W = 192 is the widest single segment and 193 the narrowest pair; 385 makes three; with H < 4 whole dy
    rows are padding.  Every tap of every kernel gradient is held on its own (_assert_per_tap)."""
    H, W = WGRAD_WIDTH_EDGES[case]['input_shapes'][0][:2]
    _wgrad_edge_step(env, WGRAD_WIDTH_EDGES[case], B, 800 + 10 * case + B, 'wgrad %d x %d B %d' % (H, W, B), monkeypatch)


def test_direct_wgrad_channel_blocks(env, monkeypatch):
    """32 -> 32, 32 -> 64, 64 -> 64, 64 -> 128 and 128 -> 128 through wgrad_kernel on a 3 x 16 image, batch of 2: up to 64
    (dy, ci block, co block) groups, so eight partial slots for six tiles."""
    _wgrad_edge_step(env, WGRAD_CHANNEL_EDGE, 2, 870, 'wgrad channel blocks', monkeypatch)


# ---- every combination of the three switches ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', (1, 0))
@pytest.mark.parametrize('off', range(8), ids=lambda m: 'off-' + ('+'.join(k[10:] for i, k in enumerate(SWITCHES) if m >> i & 1) or 'none'))
def test_switch_combinations_vs_oracle(env, case, off, monkeypatch):
    """AMT_TRAIN_FAST, AMT_TRAIN_WGRAD and AMT_TRAIN_FUSED_BN each unset or 0, with every covered layer on the fast forms
    (AMT_TRAIN_FAST_MIN_M=0), against the oracle rather than path against path: the generic BatchNormalization
    (colreduce_*, bn_apply_kernel, bn_backward_kernel) behind split-fp16 convolutions -- whose operands then nobody
    measured: operand_amax's own pass, forwards and backwards --, the direct weight gradient beside GEMM convolutions, and
    the rest.  Two steps; the second from the device's own state."""
    _set_env(monkeypatch, 0, off=[k for i, k in enumerate(SWITCHES) if off >> i & 1])
    net = env['rdcnn'].res_net(weight_seed=431 + case, calibrated=False, **CASES[case])
    net.keras_optimizer_version = 'keras-2.2' if case % 2 == 0 else 'tf.keras-1.14'
    xs, y = _edge_batch(net.cfg, 4, 40 + case)
    w0 = _copy(net.weights)
    _, acc = _compare_step(env, net, xs, y, w0, None, 'switches %d step 1' % off)
    r1 = _gradient_ratio(env, net, w0, xs, y)
    w1 = _copy(net.weights)
    xs2, y2 = _edge_batch(net.cfg, 4, 140 + case)
    _compare_step(env, net, xs2, y2, w1, acc, 'switches %d step 2' % off)
    print('case %d switches off %d: worst gradient error / bar = %.3f, %.3f' % (case, off, r1, _gradient_ratio(env, net, w1, xs2, y2)))


# ---- Adagrad, element for element --------------------------------------------------------------------------------------
@pytest.mark.parametrize('version', sorted(TRIPLES))
@pytest.mark.parametrize('case', (0, 1))
def test_adagrad_update_element_for_element(env, case, version, monkeypatch):
    """Two steps; after each, from the device's own float32 values (weights before, gradient, weights after), in float64
    with lr and epsilon as float32:
        acc <- acc + g^2 (from the triple's initial accumulator),   w* = w_before - lr g / (sqrt(acc) + eps)
        |w_after - w*| <= 1e-6 |lr g / (sqrt(acc) + eps)| + 2^-23 max(|w_before|, |w_after|)
    for EVERY element of every trainable tensor.  The step costs six float32 roundings, with sqrtf and the division within
    about 2.5 ulp each: below 1e-6 of the step; the subtraction adds one rounding of |w|.  Epsilon inside the square root
    moves a first keras-2.2 step (acc = g^2, |g| far below sqrt(1e-7)) by orders of magnitude more than that; a dropped
    or restarted accumulator shows in step 2.  The moving statistics follow 0.99 old + 0.01 batch (inside _compare_step,
    2e-5) and test() leaves every tensor bit-identical."""
    _set_env(monkeypatch)
    net = env['rdcnn'].res_net(weight_seed=531 + case, calibrated=False, **CASES[case])
    net.keras_optimizer_version = version
    lr, eps, acc0 = (np.float32(v) for v in _opt(net))
    acc, o_acc, worst = {}, None, 0.0
    for step in (1, 2):
        xs, y = _edge_batch(net.cfg, 4, 50 * step + case)
        w_before = _copy(net.weights)
        _, o_acc = _compare_step(env, net, xs, y, w_before, o_acc, 'adagrad %s step %d' % (version, step))
        g, w_after = net.gradients(), _copy(net.weights)
        for k, gk in g.items():
            if k.rsplit('/', 1)[1] in ('mean', 'var'):
                continue
            gk = gk.astype(np.float64)
            acc[k] = acc.get(k, np.full(gk.shape, np.float64(acc0))) + gk * gk
            delta = np.float64(lr) * gk / (np.sqrt(acc[k]) + np.float64(eps))
            err = np.abs(w_after[k].astype(np.float64) - (w_before[k].astype(np.float64) - delta))
            bar = 1e-6 * np.abs(delta) + 2.0 ** -23 * np.maximum(np.abs(w_before[k]), np.abs(w_after[k])).astype(np.float64)
            bad = err > bar
            assert not bad.any(), (version, step, k, int(bad.sum()), err[bad].max(), bar[bad].min())
            worst = max(worst, (err[bar > 0] / bar[bar > 0]).max(initial=0.0))
    print('case %d %s: worst Adagrad error / bar = %.3f' % (case, version, worst))
    w_now = _copy(net.weights)
    net.test(_one(xs), y)
    net._trained = True                    # pull the device's state back although test() is no train()
    net._sync_from_trainer()
    assert set(net.weights) == set(w_now)
    for k in w_now:
        assert net.weights[k].tobytes() == w_now[k].tobytes(), k


# ---- the heads no other test trains ------------------------------------------------------------------------------------
@pytest.mark.parametrize('head', ('pitch', 'instrument', 'instrument_dual'))
def test_product_head_train_on_batch_vs_oracle(env, head):
    """pitch_classifier (174 x 8, 4 x 2 kernels, 4 x 2 pools, one output), InstrumentClassifier (348 x 8, 8 x 2 pools, 112
    classes) and its two-tower variant at Hyperparams(N=2048), 33 layers each, batch of 2: one train_on_batch against the
    oracle, as for the timing head."""
    p = env['hp'].Hyperparams(N=2048)
    if head == 'pitch':
        h = env['heads'].pitch_classifier(p, calibrated=False)
        assert h.cfg['input_shapes'] == [(174, 8, 1)] and h.cfg['pool_sizes'] == [(4, 2)] and h.output_classes == 1
    else:
        h = env['heads'].InstrumentClassifier(p, head, calibrated=False)
        assert h.cfg['input_shapes'] == [(348, 8, 1)] * (2 if head == 'instrument_dual' else 1)
        assert h.cfg['pool_sizes'][0] == (8, 2) and h.output_classes == 112
    assert h.cfg['convolutional_layer_count'] == 33 and h.cfg['kernel_sizes'][0] == (4, 2)
    xs, y = _edge_batch(h.cfg, 2, 60)
    assert head == 'pitch' or sorted(y) == [0, 111]
    w0 = _copy(h.weights)
    _compare_step(env, h, xs, y, w0, None, head + ' N=2048 B=2')
    print('%s: worst gradient error / bar = %.3f' % (head, _gradient_ratio(env, h, w0, xs, y)))
    assert len(h.metrics_train) == 1
