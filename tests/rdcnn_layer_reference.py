"""One layer step of the RDCNN forward, restated in numpy from the primitives of oracle/rdcnn.py, and the table of small
nets the per-layer tests run (tests/test_rdcnn_layer_reference_cpu.py pins the restatement to oracle.rdcnn.forward;
tests/test_gpu_rdcnn_layers.py judges every conv layer of the HIP forward against it, layer by layer).

Layers are numbered 1 .. L as in the oracle.  The BLOCK OUTPUT of layer i is what oracle.rdcnn.forward holds after the
shortcut add and its BatchNormalization (where a shortcut closes at i) and before the max pool (where one follows)."""
import re

import numpy as np

from oracle.rdcnn import add_shortcut, batchnorm, conv2d_same, pool2d, sigmoid

# The case nets: the ten shapes of test_gpu_rdcnn.test_small_topologies, the five of test_gpu_small_conv.SHAPES (six
# 4 x 16 layers on one small image: the masked and window-major forms), one two-tower net (flat_off) and one one-layer
# net.  B = 7; 17 where layers take the window-major form, so that a group of 16 windows is crossed.
CASES = [
    dict(name='12x10 k4x2', shape=(12, 10), k=(4, 2), pool=(2, 2), L=5, pf=2, ef=2, r=2, K=1, B=7),
    dict(name='9x70 k4x16', shape=(9, 70), k=(4, 16), pool=(2, 8), L=4, pf=2, ef=2, r=2, K=7, B=7),
    dict(name='16x8 k2x2', shape=(16, 8), k=(2, 2), pool=(2, 2), L=6, pf=3, ef=3, r=2, K=1, B=7),
    dict(name='20x70 k4x16', shape=(20, 70), k=(4, 16), pool=(2, 8), L=3, pf=0, ef=0, r=0, K=3, B=7),
    dict(name='11x9 k4x2', shape=(11, 9), k=(4, 2), pool=(2, 2), L=4, pf=4, ef=2, r=1, K=1, B=7),
    dict(name='12x24 k4x16', shape=(12, 24), k=(4, 16), pool=(2, 2), L=6, pf=2, ef=2, r=2, K=3, B=17),
    dict(name='12x24 k4x2', shape=(12, 24), k=(4, 2), pool=(2, 2), L=6, pf=2, ef=2, r=2, K=1, B=7),
    dict(name='12x24 k2x2', shape=(12, 24), k=(2, 2), pool=(2, 2), L=6, pf=2, ef=2, r=2, K=3, B=7),
    dict(name='10x40 k4x16', shape=(10, 40), k=(4, 16), pool=(2, 2), L=6, pf=0, ef=2, r=3, K=1, B=7),
    dict(name='10x40 k2x2', shape=(10, 40), k=(2, 2), pool=(2, 2), L=6, pf=0, ef=2, r=3, K=1, B=7),
    dict(name='5x8 small', shape=(5, 8), k=(4, 16), pool=(2, 2), L=6, pf=0, ef=2, r=2, K=3, B=17),
    dict(name='5x4 small', shape=(5, 4), k=(4, 16), pool=(2, 2), L=6, pf=0, ef=2, r=2, K=3, B=17),
    dict(name='3x5 small', shape=(3, 5), k=(4, 16), pool=(2, 2), L=6, pf=0, ef=2, r=2, K=3, B=17),
    dict(name='8x8 small', shape=(8, 8), k=(4, 16), pool=(2, 2), L=6, pf=0, ef=2, r=2, K=3, B=17),
    dict(name='7x9 small', shape=(7, 9), k=(4, 16), pool=(2, 2), L=6, pf=0, ef=2, r=2, K=3, B=17),
    dict(name='two towers', shape=[(9, 22), (6, 13)], k=[(4, 2), (2, 2)], pool=[(2, 2), (2, 2)], L=4, pf=2, ef=2, r=2,
         K=5, B=7),
    # a kernel size the matrix-pipe kernels are not built for: only a one-layer net can have it (conv1_kernel, the
    # VALU first layer), here with a projected shortcut from the input and a max pool behind it
    dict(name='7x11 k3x5 one layer', shape=(7, 11), k=(3, 5), pool=(2, 2), L=1, pf=1, ef=0, r=1, K=3, B=7),
]
WEIGHT_SEED = 77


def case_net(case):
    """The res_net of a case (no GPU is touched until its first forward)."""
    from amt_saga import rdcnn
    multi = isinstance(case['shape'], list)
    shapes = case['shape'] if multi else [case['shape']]
    return rdcnn.res_net(input_shapes=[tuple(s) + (1,) for s in shapes], output_classes=case['K'], output_range=[3, 40],
                         kernel_sizes=case['k'] if multi else [case['k']],
                         pool_sizes=case['pool'] if multi else [case['pool']], convolutional_layer_count=case['L'],
                         feature_expand_frequency=case['ef'], pool_layer_frequency=case['pf'],
                         residual_layer_frequencies=case['r'], weight_seed=WEIGHT_SEED)


def case_inputs(case, seed):
    """Per tower [B, H, W] float32: rng.random ** 2, window 2 three times as loud, window 4 all zero (the per-window
    operand scaling of the split-fp16 kernels and their zero-amax path)."""
    shapes = case['shape'] if isinstance(case['shape'], list) else [case['shape']]
    rng = np.random.default_rng(seed)
    xs = []
    for s in shapes:
        x = (rng.random((case['B'],) + tuple(s)) ** 2).astype(np.float32)
        x[2] *= 3
        x[4] = 0
        xs.append(x)
    return xs


def assert_weights_not_identity(w):
    """No BatchNormalization and no bias of the net is a no-op: a kernel that dropped one would show."""
    for name, a in w.items():
        kind = name.rsplit('/', 1)[1]
        off = {'gamma': 1.0, 'var': 1.0, 'beta': 0.0, 'mean': 0.0, 'bias': 0.0}.get(kind)
        if off is not None:
            assert np.abs(np.asarray(a, np.float64) - off).min() > 1e-6, name


def _rfreq(cfg):
    rf = cfg['residual_layer_frequencies']
    return rf[0] if rf else 0


def closes_shortcut(cfg, i):
    r = _rfreq(cfg)
    return bool(r) and i % r == 0


def pooled_after(cfg, i):
    pf = cfg['pool_layer_frequency']
    return bool(pf) and i % pf == 0


def shortcut_source(cfg, i):
    """Layer whose block output is the shortcut source of closing layer i; 0 = the tower's input."""
    return i - _rfreq(cfg)


def layer_input(cfg, t, i, prev_block_out):
    """Input of layer i (2 .. L + 1; L + 1 = the tower's contribution to the dense input) from the block output of
    layer i - 1: through the max pool where the topology has one."""
    return pool2d(prev_block_out, cfg['pool_sizes'][t], 'max') if pooled_after(cfg, i - 1) else prev_block_out


def layer_step(w, cfg, t, i, x_in, sc_src, dtype):
    """Block output of layer i of tower t from its input x_in [B, H, W, cin] and, where a shortcut closes at i, the
    shortcut source sc_src (block output of layer shortcut_source(cfg, i), or the tower's input), all in dtype."""
    mine = re.compile(r't%d/(conv|bn|sc|scbn|resbn)%d/' % (t, i))
    w = {k: np.asarray(v, dtype=dtype) for k, v in w.items() if mine.match(k)}
    p1 = conv2d_same(np.asarray(x_in, dtype=dtype), w['t%d/conv%d/kernel' % (t, i)], w['t%d/conv%d/bias' % (t, i)])
    p1 = sigmoid(batchnorm(p1, w, 't%d/bn%d' % (t, i)))
    if closes_shortcut(cfg, i):
        p1 = add_shortcut(w, t, i, np.asarray(sc_src, dtype=dtype), p1)
        p1 = batchnorm(p1, w, 't%d/resbn%d' % (t, i))
    return p1


def dense_step(w, flat_inputs, dtype):
    """Logits from the towers' last activations (layer_input(cfg, t, L + 1, .), [B, h, w, c] each)."""
    flats = [np.asarray(a, dtype=dtype).reshape(a.shape[0], -1) for a in flat_inputs]
    cted = np.concatenate(flats, axis=1) if len(flats) > 1 else flats[0]
    d = {k: np.asarray(w[k], dtype=dtype) for k in ('dense1/kernel', 'dense1/bias', 'dense2/kernel', 'dense2/bias')}
    m = sigmoid(cted @ d['dense1/kernel'] + d['dense1/bias'])
    return m @ d['dense2/kernel'] + d['dense2/bias']


def chain(w, cfg, xs, dtype):
    """The whole forward as a chain of the steps above: (logits, [[block output per layer] per tower])."""
    outs, flats = [], []
    for t, x in enumerate(xs):
        blocks = [np.asarray(x, dtype=dtype)]                      # index 0: the tower's input
        cur = blocks[0]
        for i in range(1, cfg['convolutional_layer_count'] + 1):
            sc = blocks[shortcut_source(cfg, i)] if closes_shortcut(cfg, i) else None
            blocks.append(layer_step(w, cfg, t, i, cur, sc, dtype))
            cur = layer_input(cfg, t, i + 1, blocks[i])
        outs.append(blocks[1:])
        flats.append(cur)
    return dense_step(w, flats, dtype), outs
