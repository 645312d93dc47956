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
    """Per tower [B, H, W] float32: rng.random ** 2, window 2 three times as loud, window 4 all zero -- window 0 where B
    is below 5 (the per-window operand scaling of the split-fp16 kernels and their zero-amax path)."""
    shapes = case['shape'] if isinstance(case['shape'], list) else [case['shape']]
    rng = np.random.default_rng(seed)
    xs = []
    for s in shapes:
        x = (rng.random((case['B'],) + tuple(s)) ** 2).astype(np.float32)
        x[2] *= 3
        x[4 if case['B'] > 4 else 0] = 0
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


# ---- conv mode 3: the FFT-domain forms (tests/test_gpu_rdcnn_fft_layers.py) ------------------------------------------
# The case nets of the per-form test: the 4 x 16 entries of CASES, the nets of test_gpu_pooled_epilogue (four 32 -> 32
# layers with a (2, 8) pool behind the fourth, four and six layers deep, and the 10 x 64 net whose fourth layer is the
# packed 64 -> 64 form) and what the form families of fft_families still ask for.  B = 7; 17 where a group of 8 windows
# (one GEMM chunk) is to be crossed with a ragged last chunk; 3 at W = 561; 5 on the 10 x 64, 64 -> 64 nets (the float64
# reference of those layers is the slow part).
_E = dict(k=(4, 16), pool=(2, 8), pf=4, ef=4, r=2, K=3)             # test_gpu_pooled_epilogue._net
FFT_CASES = [c for c in CASES if c['k'] == (4, 16)] + [
    dict(_E, name='fft 20x44 L4', shape=(20, 44), L=4, B=7),
    dict(_E, name='fft 20x44 L6', shape=(20, 44), L=6, B=7),
    dict(_E, name='fft 5x24 L4', shape=(5, 24), L=4, B=17),
    dict(_E, name='fft 5x24 L6', shape=(5, 24), L=6, B=7),
    dict(_E, name='fft 3x17 L4', shape=(3, 17), L=4, B=17),
    dict(_E, name='fft 3x17 L6', shape=(3, 17), L=6, B=7),
    dict(_E, name='fft 4x561 L4', shape=(4, 561), L=4, B=3),
    dict(_E, name='fft 4x561 L6', shape=(4, 561), L=6, B=3),
    dict(_E, name='fft packed 10x64 L4', shape=(10, 64), L=4, ef=2, B=5),
    dict(_E, name='fft packed 10x64 L6', shape=(10, 64), L=6, ef=2, B=5),
    # a shortcut at every layer, pooled (2, 8) behind layer 2: layer 2 adds the shortcut tensor as is, layer 3 a pooled
    # one (projection kernel).  7 x 13: W < 16, then a 3 x 1 image; 9 x 72: layer 2 leaves the pooled pair for the max
    # pool and layer 3's shortcut, layer 3 hands on, layer 4 (4 x 9) leaves a pair that drops one column
    dict(name='fft 7x13 r1', shape=(7, 13), k=(4, 16), pool=(2, 8), L=3, pf=2, ef=0, r=1, K=3, B=7),
    dict(name='fft 9x72 r1', shape=(9, 72), k=(4, 16), pool=(2, 8), L=4, pf=2, ef=0, r=1, K=3, B=7),
    # no shortcut at all: a run of two layers that exist only transformed, then one with a spatial output (flat row)
    dict(name='fft 6x25 r0 L4', shape=(6, 25), k=(4, 16), pool=(2, 8), L=4, pf=0, ef=0, r=0, K=3, B=17),
    # unpooled, unexpanded, six deep: rank-1 and tensor shortcuts with the hand-over, the last one into the flat row
    dict(name='fft 7x30 r2 L6', shape=(7, 30), k=(4, 16), pool=(2, 8), L=6, pf=0, ef=0, r=2, K=3, B=7),
    # pooled behind the rank-1 layer: rank-1 without a hand-over; layer 4 closes a pooled projected shortcut
    dict(name='fft 8x20 pf2', shape=(8, 20), k=(4, 16), pool=(2, 2), L=4, pf=2, ef=0, r=2, K=3, B=7),
    # two towers of 4 x 16 kernels: the second tower's last layer writes its flat row at flat_off != 0
    dict(name='fft two towers', shape=[(6, 21), (5, 12)], k=[(4, 16), (4, 16)], pool=[(2, 8), (2, 8)], L=4, pf=0, ef=0,
         r=2, K=5, B=7),
    # 10 x 64 with the channels doubled behind layer 3: layers 5 and 6 are packed 64 -> 64, handed over packed to packed
    dict(name='fft packed r2 ef3', shape=(10, 64), k=(4, 16), pool=(2, 8), L=6, pf=0, ef=3, r=2, K=3, B=5),
    dict(name='fft packed r1 ef3', shape=(10, 64), k=(4, 16), pool=(2, 8), L=6, pf=0, ef=3, r=1, K=3, B=5),
    dict(name='fft packed r0 ef3', shape=(10, 64), k=(4, 16), pool=(2, 8), L=6, pf=0, ef=3, r=0, K=3, B=5),
]
FC_CW, FC_NP = 8, 289                   # windows per GEMM chunk and frequency pairs of the row form (amt_fftconv.hip)


def gemm_chunks_per_wg(B):
    """`per` of amt_fftconv_gemm: chunks of 8 windows per workgroup, doubled until the grid has at most 4096 workgroups."""
    nchunks, per = -(-B // FC_CW), 1
    while -(-nchunks // per) * FC_NP > 4096 and per < 16:
        per *= 2
    return per


def case_cfg(case):
    """The cfg dict of a case's res_net, without creating one."""
    multi = isinstance(case['shape'], list)
    shapes = case['shape'] if multi else [case['shape']]
    return dict(input_shapes=[tuple(s) + (1,) for s in shapes], kernel_sizes=case['k'] if multi else [case['k']],
                pool_sizes=case['pool'] if multi else [case['pool']], convolutional_layer_count=case['L'],
                feature_expand_frequency=case['ef'], pool_layer_frequency=case['pf'],
                residual_layer_frequencies=[case['r']] if case['r'] else [], output_classes=case['K'])


def model_fc_plans(cfg, B):
    """What res_net.fc_plans(3, B) must report, restated from the rules of the forward (amt_rdcnn.hip: conv_impl,
    shortcut_is_rank1, fc_wpooled_ok, layer_form) on the topology alone -- [[plan per layer] per tower], each plan with
    H, W, cin, cout beside the keys of fc_plans.  The shortcut kind of a layer that is no FFT-domain form is None (which
    of the other kernels forms a rank-1 shortcut itself is not restated here).  The coverage of FFT_CASES is checked
    against this without a device, and the device test holds the library's report to it."""
    L, ef, r = cfg['convolutional_layer_count'], cfg['feature_expand_frequency'], _rfreq(cfg)
    out = []
    for t, shp in enumerate(cfg['input_shapes']):
        (kh, kw), (ph, pw) = cfg['kernel_sizes'][t], cfg['pool_sizes'][t]
        H, W, cin, cout = shp[0], shp[1], 1, 32
        rows = [dict(H=H, W=W, cout=1)]                                           # index 0: the tower's input
        for i in range(1, L + 1):
            p = dict(tower=t, layer=i, mode=3, H=H, W=W, cin=cin, cout=cout, pool_after=pooled_after(cfg, i),
                     residual=closes_shortcut(cfg, i))
            p['form'] = 'none'
            if (kh, kw) == (4, 16) and cin == cout == 32 and W + 15 <= 576 and H <= 20:
                p['form'] = 'row'
            elif (kh, kw) == (4, 16) and cin == cout == 64 and (H, W) == (10, 64):
                p['form'] = 'packed'
            rows.append(p)
            if p['pool_after']:
                H, W = H // ph, W // pw
                assert H >= 1 and W >= 1, 'the max pool behind layer %d collapses the image' % i
            cin = cout
            if ef and i % ef == 0:
                cout *= 2
        for i in range(1, L + 1):
            p = rows[i]
            fft = p['form'] != 'none'
            hands = lambda q: q['form'] != 'none' and q['layer'] < L and not q['pool_after'] and \
                rows[q['layer'] + 1]['form'] == q['form']
            p['have_xf'] = fft and i > 1 and hands(rows[i - 1])
            p['hands_on'] = fft and hands(p)
            p['out_is_flat_row'] = i == L and not p['pool_after']
            kind = 'none'
            if p['residual']:
                s = rows[shortcut_source(cfg, i)]
                same_image = (s['H'], s['W']) == (p['H'], p['W'])
                if same_image and s['cout'] == p['cout']:
                    kind = 'tensor'
                else:
                    kind = 'rank1' if p['form'] == 'row' and s['cout'] == 1 and same_image else 'projected'
            p['shortcut'] = kind if fft else None
            wp = fft and p['pool_after'] and pw == 8 and p['W'] >= 8 and kind in ('tensor', 'projected')
            if wp:
                nxt = next((q for q in rows[i + 1:] if q['residual']), None)     # the next closing layer reads it
                if nxt is not None:
                    s = rows[shortcut_source(cfg, nxt['layer'])]
                    wp = s is p and (nxt['H'], nxt['W'], nxt['cout']) != (p['H'], p['W'], p['cout']) and \
                        p['W'] // nxt['W'] == 8 and nxt['W'] == p['W'] // 8
            p['wpooled'] = wp
            p['writes_spatial'] = not fft or (not wp and (not p['hands_on'] or p['residual']))
            p['per'] = gemm_chunks_per_wg(min(B, 1024)) if p['form'] == 'row' else 1 if fft else 0
        out.append(rows[1:])
    return out


def pooled_pair(block_out):
    """(wavg, wmax) of a W-pooled layer's block output [B, H, W, C]: mean and max over the columns 8 g .. 8 g + 7 for
    g < W // 8, [B, H, W // 8, C] each; the columns behind 8 (W // 8) are dropped."""
    return pool2d(block_out, (1, 8), 'avg'), pool2d(block_out, (1, 8), 'max')


def next_input(cfg, t, i, block_out, fc_plan=None):
    """Input of layer i + 1 (or, i = L, the tower's part of the dense input) from what layer i left: its block output,
    or -- fc_plan['wpooled'] -- its W-pooled pair [2, B, H, W // 8, C], whose maxima the max pool reads with (ph, 1)."""
    if fc_plan is not None and fc_plan['wpooled']:
        assert pooled_after(cfg, i) and cfg['pool_sizes'][t][1] == 8
        return pool2d(block_out[1], (cfg['pool_sizes'][t][0], 1), 'max')
    return layer_input(cfg, t, i + 1, block_out)


def shortcut_tensor(block_out, fc_plan=None):
    """What a later closing layer takes as its shortcut source from layer i's tapped tensor: the block output, or the
    means of a W-pooled pair (add_shortcut then pools them (sc_ph, 1): the mean over 8 columns is already taken)."""
    return block_out[0] if fc_plan is not None and fc_plan['wpooled'] else block_out


def run_steps(w, cfg, t, first, last, x_in, sources, dtype):
    """Block output of layer `last` from the input x_in of layer `first`, through the layers between (none of which is
    pooled or closes a shortcut: the hand-over layers of an FFT-domain run), in dtype.  sources: {closing layer: source}."""
    cur = np.asarray(x_in, dtype=dtype)
    for i in range(first, last + 1):
        assert i == last or not (pooled_after(cfg, i) or closes_shortcut(cfg, i))
        cur = layer_step(w, cfg, t, i, cur, sources.get(i), dtype)
    return cur


def fft_families(rows):
    """{family: [where]} of the FFT-domain forms, from (case, plan) rows -- plan: a dict of fc_plans() merged with H and W
    of layer_plans() (or of model_fc_plans)."""
    hit = {}

    def add(fam, where):
        hit.setdefault(fam, []).append(where)
    by_case = {}
    for case, p in rows:
        by_case.setdefault((case['name'], p['tower']), []).append(p)
        if p['form'] == 'none':
            continue
        where = '%s tower %d layer %d' % (case['name'], p['tower'], p['layer'])
        f = p['form']
        add('%s: forward from a spatial input' % f if not p['have_xf'] else '%s: have_xf' % f, where)
        if p['hands_on'] and not p['writes_spatial']:
            add('%s: EPI 1' % f, where)
        if p['have_xf']:
            add('%s: %s to %s hand-over' % (f, f, f), where)
        if p['shortcut'] in ('tensor', 'projected'):
            add('%s: shortcut tensor %s hand-over' % (f, 'with' if p['hands_on'] else 'without'), where)
            if not p['wpooled']:
                add('%s: shortcut tensor %s %s hand-over' % (f, 'as is' if p['shortcut'] == 'tensor' else 'projected',
                                                             'with' if p['hands_on'] else 'without'), where)
        if p['shortcut'] == 'projected':
            add('%s: shortcut through proj_kernel' % f, where)
        if p['shortcut'] == 'rank1':
            add('%s: rank-1 %s hand-over' % (f, 'with' if p['hands_on'] else 'without'), where)
        if p['shortcut'] == 'none' and p['writes_spatial']:
            add('%s: no shortcut, spatial output' % f, where)
        if p['out_is_flat_row']:
            add('%s: out_is_flat_row' % f, where)
            if p['tower'] > 0:
                add('%s: out_is_flat_row at flat_off != 0' % f, where)
        if p['wpooled']:
            add('%s: wpooled' % f, where)
        if f == 'row':
            H, W, B = p['H'], p['W'], case['B']
            for fam, yes in (('H = 3', H == 3), ('H odd', H % 2 == 1 and H > 3), ('H = 20', H == 20), ('W < 16', W < 16),
                             ('W % 8 != 0', W % 8 != 0), ('W % 24 != 0', W % 24 != 0), ('W = 561', W == 561),
                             ('B = 17 crosses a chunk of 8, ragged', B > 8 and B % 8 != 0)):
                if yes:
                    add('row geometry: %s' % fam, where)
    for (name, t), ps in by_case.items():
        ps = sorted(ps, key=lambda p: p['layer'])
        for a, b, c in zip(ps, ps[1:], ps[2:]):
            # two layers in a row that exist only transformed: judged together with the tapped layer behind them
            if a['form'] == 'row' and all(q['form'] == 'row' and q['hands_on'] and not q['writes_spatial'] for q in (a, b)):
                add('row: hand-over run of two untapped layers', '%s tower %d layers %d-%d' % (name, t, a['layer'], c['layer']))
        for i, p in enumerate(ps):
            if p['form'] != 'none' and p['wpooled']:
                reader = next((q for q in ps[i + 1:] if q.get('residual', q['shortcut'] not in ('none', None))), None)
                add('%s: wpooled read by %s' % (p['form'], 'the max pool only' if reader is None else
                                                'a pooled projected shortcut'), '%s tower %d layer %d' % (name, t, p['layer']))
    return hit


FFT_REQUIRED = (['row: forward from a spatial input', 'row: have_xf', 'row: EPI 1',
                 'row: shortcut tensor as is with hand-over', 'row: shortcut tensor as is without hand-over',
                 'row: shortcut through proj_kernel', 'row: rank-1 with hand-over', 'row: rank-1 without hand-over',
                 'row: no shortcut, spatial output', 'row: out_is_flat_row', 'row: out_is_flat_row at flat_off != 0',
                 'row: wpooled read by the max pool only', 'row: wpooled read by a pooled projected shortcut',
                 'row: hand-over run of two untapped layers',
                 'packed: forward from a spatial input', 'packed: packed to packed hand-over',
                 'packed: shortcut tensor with hand-over', 'packed: shortcut tensor without hand-over',
                 'packed: no shortcut, spatial output', 'packed: wpooled'] +
                ['row geometry: %s' % g for g in ('H = 3', 'H odd', 'H = 20', 'W < 16', 'W % 8 != 0', 'W % 24 != 0',
                                                  'W = 561', 'B = 17 crosses a chunk of 8, ragged')])
