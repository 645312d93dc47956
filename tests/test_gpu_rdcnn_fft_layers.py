"""Every form of an FFT-domain conv layer that the HIP forward issues in conv mode 3 (amt_rdcnn.hip: layer_form, run_fc;
amt_fftconv.hip, amt_fftpk.hip), judged element by element against float64 -- the mode-3 counterpart of
test_gpu_rdcnn_layers.py, with its tap, its reference, its bar and its records.

One forward per case net (rdcnn_layer_reference.FFT_CASES) with every layer tapped that leaves something to tap: a
spatial output, or the W-pooled pair (res_net.fc_plans: writes_spatial / wpooled).  A layer that exists only transformed
(hands_on and not writes_spatial: EPI = 1 of the row kernels) is judged together with the layers up to the next tapped
one: the reference is the float64 composition of those steps (run_steps) from the GPU's OWN last tapped tensor and the
GPU's own shortcut source, e_cpu the float32 composition of the same steps.  A W-pooled layer is judged half by half
against the mean and the max over 8 columns of its float64 block output (pooled_pair); the layer behind it is fed the
max pool of the GPU's wmax, a later pooled shortcut the GPU's wavg.  The layers of mode 3 that are no FFT-domain form
(the first layer, the split-fp16 kernels) are tapped and judged alone as in the other modes.

The bar is test_gpu_rdcnn_layers.judge, strict for every form, on EVERY element:
    |got - ref64| <= 2.5 * e_cpu + 2.4e-7 * scale,   e_cpu = max |ref32 - ref64|,  scale = max |ref64|
No form is in LOOSE_BAR.  Per (case, tower, run of layers, half) e_gpu, e_cpu, their ratio, e_gpu / bar and the fc_plan
of each layer of the run go to rdcnn_fft_layer_error_vs_f64.json in the run's output directory (committed as
profiles/rdcnn_fft_layer_error_vs_f64.json, quoted in DESIGN.md)."""
import numpy as np
import pytest

import rdcnn_layer_reference as lr
from test_gpu_rdcnn import dump_records
from test_gpu_rdcnn_layers import LOOSE_BAR, _check_sensitivity, judge

pytestmark = pytest.mark.gpu

RECORDS = []
_NETS = {}
FC_KEYS = ('form', 'have_xf', 'hands_on', 'writes_spatial', 'shortcut', 'wpooled', 'out_is_flat_row', 'per')

# Families of rdcnn_layer_reference.FFT_REQUIRED that no res_net reaches, with the reason (none: every one is reached).
UNREACHABLE = {}


@pytest.fixture(scope='module', autouse=True)
def _dump():
    yield
    dump_records('rdcnn_fft_layer_error_vs_f64.json', RECORDS)
    for form in ('row', 'packed', 'none'):
        rs = [r for r in RECORDS if r['form'] == form and r['e_cpu'] > 0]
        if rs:
            a, b = max(rs, key=lambda r: r['ratio']), max(rs, key=lambda r: r['e_gpu_over_bar'])
            print('mode 3 %-6s worst e_gpu/e_cpu %.2f (%s tower %d layers %s %s), worst e_gpu/bar %.2f (%s tower %d layers %s %s)'
                  % (form, a['ratio'], a['case'], a['tower'], a['layers'], a['half'], b['e_gpu_over_bar'], b['case'],
                     b['tower'], b['layers'], b['half']))


def _net(case):
    if case['name'] not in _NETS:
        import torch
        assert torch.cuda.is_available()
        net = lr.case_net(case)
        net.set_mode(3)
        _NETS[case['name']] = net
    return _NETS[case['name']]


def _plans(net, B):
    """fc_plans merged with H, W, cin, cout and the implementation of layer_plans, per tower and layer."""
    return [[dict(f, H=p['H'], W=p['W'], cin=p['cin'], cout=p['cout'], impl=p['impl']) for f, p in zip(fs, ps)]
            for fs, ps in zip(net.fc_plans(B=B), net.layer_plans())]


def _brief(p):
    return {k: p[k] for k in ('layer', 'H', 'W') + FC_KEYS}


@pytest.mark.parametrize('case', lr.FFT_CASES, ids=[c['name'].replace(' ', '_') for c in lr.FFT_CASES])
def test_every_fft_form_against_float64(case):
    import torch
    net = _net(case)
    cfg, w, B = net.cfg, net.weights, case['B']
    lr.assert_weights_not_identity(w)
    L = cfg['convolutional_layer_count']
    plans = _plans(net, B)
    # the library's report is the one the topology rules predict (the model the CPU coverage test runs on)
    for row, mrow in zip(plans, lr.model_fc_plans(cfg, B)):
        for p, m in zip(row, mrow):
            assert (p['H'], p['W'], p['cin'], p['cout']) == (m['H'], m['W'], m['cin'], m['cout'])
            assert p['form'] == {'fft_row': 'row', 'fft_packed': 'packed'}.get(p['impl'], 'none')
            for k in FC_KEYS:
                if m[k] is not None:
                    assert p[k] == m[k], (case['name'], k, _brief(p), m)
    assert any(p['form'] != 'none' for row in plans for p in row), 'no FFT-domain layer in %s' % case['name']
    xs = lr.case_inputs(case, 31)
    dev = [torch.from_numpy(x).cuda() for x in xs]
    taps = [(t, p['layer']) for t, row in enumerate(plans) for p in row if p['writes_spatial'] or p['wpooled']]
    y, lg, acts = net.layer_outputs(dev, layers=taps)
    y2, lg2 = net.predict_device(dev, return_logits=True)           # the tap changes nothing
    assert torch.equal(lg, lg2) and torch.equal(y, y2)
    acts = [[None if a is None else a.cpu().numpy() for a in row] for row in acts]
    failures, probed, tail_probed = [], False, False
    for t, x in enumerate(xs):
        tapped = {0: x[..., None]}                                  # what a later closing layer reads as its source
        start, x_in = 1, tapped[0]
        for i in range(1, L + 1):
            p, got = plans[t][i - 1], acts[t][i - 1]
            if got is None:
                assert p['form'] != 'none' and p['hands_on'] and not p['writes_spatial'] and p['shortcut'] == 'none'
                continue                                            # judged with the run that ends at the next tap
            run = plans[t][start - 1:i]
            src = {i: tapped[lr.shortcut_source(cfg, i)]} if lr.closes_shortcut(cfg, i) else {}
            ref64 = lr.run_steps(w, cfg, t, start, i, x_in, src, np.float64)
            ref32 = lr.run_steps(w, cfg, t, start, i, x_in, src, np.float32)
            assert ref64.shape == (B, p['H'], p['W'], p['cout'])
            if p['wpooled']:
                assert got.shape == (2, B, p['H'], p['W'] // 8, p['cout'])
                halves = list(zip(('wavg', 'wmax'), got, lr.pooled_pair(ref64), lr.pooled_pair(ref32)))
            else:
                assert got.shape == ref64.shape
                halves = [('', got, ref64, ref32)]
            layers = '%d' % i if start == i else '%d-%d' % (start, i)
            impl = p['impl'] if p['form'] == 'none' else None       # no FFT-domain form is in LOOSE_BAR
            assert p['form'] == 'none' or p['impl'] not in LOOSE_BAR
            for half, g, r64, r32 in halves:
                j = judge(g, r64, r32, impl)
                RECORDS.append(dict(case=case['name'], tower=t, layers=layers, half=half, form=p['form'], impl=p['impl'],
                                    e_gpu=j['e_gpu'], e_cpu=j['e_cpu'], ratio=j['e_gpu'] / max(j['e_cpu'], 1e-30),
                                    e_gpu_over_bar=j['e_gpu'] / j['bar'], scale=j['scale'], bar=j['bar'], over=j['over'],
                                    worst=list(j['worst']), windows=B, fc_plan=[_brief(q) for q in run]))
                print('%s tower %d layers %s %-4s %-10s e_gpu %.3g e_cpu %.3g bar %.3g over %d' %
                      (case['name'], t, layers, half, p['impl'], j['e_gpu'], j['e_cpu'], j['bar'], j['over']))
                if j['over']:
                    failures.append('%s tower %d layers %s %s: %d of %d elements over the bar %.3g; worst (b, h, w, c) = %s: '
                                    'e_gpu %.3g, e_cpu %.3g, scale %.3g; fc_plan of the run %s' %
                                    (case['name'], t, layers, half, j['over'], r64.size, j['bar'], j['worst'], j['e_gpu'],
                                     j['e_cpu'], j['scale'], [_brief(q) for q in run]))
                if p['form'] != 'none' and not probed:
                    _check_sensitivity(g, r64, r32, impl, (case['name'], t, layers, half))
            probed |= p['form'] != 'none'
            if p['wpooled'] and p['W'] % 8 and not tail_probed:
                # a pair whose last group took the columns behind 8 (W // 8) instead is rejected
                tail_probed = True
                moved = got[1].copy()
                moved[:, :, -1, :] = ref64[:, :, 8 * (p['W'] // 8):, :].max(axis=2)
                assert judge(moved, halves[1][2], halves[1][3], impl)['over'] >= 1, (case['name'], t, i)
            tapped[i] = lr.shortcut_tensor(got, p)
            start, x_in = i + 1, lr.next_input(cfg, t, i, got, p)
        assert start == L + 1
    assert probed
    assert not failures, '\n'.join(failures)


def test_coverage():
    """Every form family and geometry of rdcnn_layer_reference.FFT_REQUIRED is hit by FFT_CASES, by the plan reports of
    the nets themselves (no kernel runs)."""
    rows = [(case, p) for case in lr.FFT_CASES for row in _plans(_net(case), case['B']) for p in row]
    hit = lr.fft_families(rows)
    missing = [f for f in lr.FFT_REQUIRED if f not in hit and f not in UNREACHABLE]
    assert not missing, 'families no case reaches: %s' % missing
    for fam in UNREACHABLE:
        assert fam in lr.FFT_REQUIRED and fam not in hit, fam


def test_gemm_chunks_per_workgroup_report():
    """fc_plans reports `per` of amt_fftconv_gemm for the forward's B: 1 up to 14 chunks of 8 windows, 2 from 15 on,
    doubled while the grid would still exceed 4096 workgroups, for at most one pass of 1024 windows."""
    net = _net(next(c for c in lr.FFT_CASES if c['name'] == 'fft 3x17 L4'))
    for B, per in ((7, 1), (112, 1), (113, 2), (120, 2), (224, 2), (225, 4), (1024, 16), (5000, 16)):
        got = [p['per'] for p in net.fc_plans(B=B)[0]]
        assert got == [0, per, per, per], (B, got)
        assert per == lr.gemm_chunks_per_wg(min(B, 1024))


def test_pooled_pair_tap_across_passes_and_chunks_per_workgroup():
    """The pair of a forward that takes two passes (1024 + 6 windows) is the pairs of the two passes, wavg first, and the
    untapped logits are the tapped ones: the tap's offsets inside each half.  The pass of 1024 windows runs the GEMM
    with 16 chunks per workgroup; the same windows in forwards of 100 (one chunk per workgroup) and of 120 (two, the
    last workgroup's second chunk past the end) give the same bits."""
    import torch
    case = next(c for c in lr.FFT_CASES if c['name'] == 'fft 3x17 L4')
    net = _net(case)
    plans = _plans(net, 1030)[0]
    assert plans[3]['wpooled'] and plans[3]['per'] == 16 and _plans(net, 100)[0][3]['per'] == 1 and _plans(net, 120)[0][3]['per'] == 2
    rng = np.random.default_rng(5)
    x = torch.from_numpy((rng.random((1030,) + case['shape']) ** 2).astype(np.float32)).cuda()
    y, lg, acts = net.layer_outputs([x], layers=[(0, 4)])
    pair = acts[0][3]
    assert pair.shape == (2, 1030, 3, 2, 32) and acts[0][:3] == [None, None, None]
    y2, lg2 = net.predict_device([x], return_logits=True)
    assert torch.equal(lg, lg2) and torch.equal(y, y2)
    for step in (100, 120):
        for b0 in range(0, 1030, step):
            xb = x[b0:b0 + step].contiguous()
            _, lgb, ab = net.layer_outputs([xb], layers=[(0, 4)])
            assert torch.equal(ab[0][3], pair[:, b0:b0 + step]), (step, b0)
            assert torch.equal(lgb, lg[b0:b0 + step]), (step, b0)


def test_layer_outputs_named_layer_that_cannot_be_tapped():
    """Naming a layer that exists only transformed is refused as before; naming its neighbours is not."""
    import torch
    case = next(c for c in lr.FFT_CASES if c['name'] == 'fft 6x25 r0 L4')
    net = _net(case)
    xs = [torch.from_numpy(x).cuda() for x in lr.case_inputs(case, 3)]
    y, lg = net.predict_device(xs, return_logits=True)
    for layer in (2, 3):
        with pytest.raises(ValueError):
            net.layer_outputs(xs, layers=[(0, layer)])
    y2, lg2, acts = net.layer_outputs(xs, layers=[(0, 1), (0, 4)])
    assert torch.equal(lg2, lg) and torch.equal(y2, y)
    assert acts[0][1] is None and acts[0][2] is None and acts[0][0] is not None and acts[0][3] is not None
