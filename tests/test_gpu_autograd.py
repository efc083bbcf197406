"""yoloret_amd/autograd.py on the device: each torch.autograd.Function against the float64 restatement of tests/convgrad_ref.py, and a
stack of them on top of yolov3_features trained with YoloLoss.call and runtime.adam_step.

The bar is the project's own: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the float32 restatement's deviation from
float64 on the same inputs.  Every comparison prints its figures before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

from tests import convgrad_ref as ref, headtrain_ref, loss_ref, lossgrad_ref
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24


def _ag():
    from yoloret_amd import autograd
    return autograd


def _rt():
    from yoloret_amd import runtime
    return runtime


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.uint32)


def _dev(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(grad)


def _within_bar(what, got, r32, r64):
    e_dev, e_ref = ref.rel_err(got.detach().cpu().numpy(), r64), ref.rel_err(r32, r64)
    print('%s: device %.3e, float32 restatement %.3e, bar %.3e' % (what, e_dev, e_ref, 4 * e_ref + EPS24))
    return e_dev <= 4 * e_ref + EPS24


class Calls:
    """counts the calls of runtime entries that yoloret_amd.autograd makes"""

    def __init__(self, monkeypatch, names):
        self.n = {}
        rt = _rt()
        for name in names:
            self.n[name] = 0
            monkeypatch.setattr(rt, name, self._wrap(name, getattr(rt, name)))

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.n[name] += 1
            return fn(*a, **kw)
        return counted


# ----------------------------------------------------------------------------- per Function
@pytest.mark.parametrize('gx,gw', [(True, True), (True, False), (False, True)])
def test_linear1x1(dev, monkeypatch, gx, gw):
    calls = Calls(monkeypatch, ['linear_forward', 'linear_dgrad', 'linear_wgrad'])
    rng = np.random.default_rng(1)
    cin, cout = 17, 15
    x = rng.standard_normal((2, 5, 7, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    dy = rng.standard_normal((2, 5, 7, cout)).astype(np.float32)
    tx, twt = _dev(x, dev, gx), _dev(ref.pack_wt(w), dev, gw)
    y = _ag().linear1x1(tx, twt)
    assert y.requires_grad and tuple(y.shape) == (2, 5, 7, cout)
    y.backward(_dev(dy, dev))
    torch.cuda.synchronize()
    assert calls.n == {'linear_forward': 1, 'linear_dgrad': int(gx), 'linear_wgrad': int(gw)}
    x2, dy2 = x.reshape(-1, cin), dy.reshape(-1, cout)
    (dx64, dw64), (dx32, dw32) = ref.linear_grads(x2, w, dy2), ref.linear_grads(x2, w, dy2, np.float32)
    ok = [_within_bar('linear1x1 y', y.reshape(-1, cout), ref.linear(x2, w, np.float32), ref.linear(x2, w))]
    if gx:
        ok.append(_within_bar('linear1x1 dx', tx.grad.reshape(-1, cin), dx32, dx64))
    else:
        assert tx.grad is None
    if gw:
        assert tuple(twt.grad.shape) == (cout, 20) and not _bits(twt.grad[:, cin:]).any(), 'pad columns +0'
        ok.append(_within_bar('linear1x1 dwt', twt.grad[:, :cin], dw32, dw64))
    else:
        assert twt.grad is None
    assert all(ok)


@pytest.mark.parametrize('gx,gw', [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize('k,stride,padding', [(3, 2, 'mobilenet'), (5, 1, 'same')])
def test_depthwise(dev, monkeypatch, k, stride, padding, gx, gw):
    calls = Calls(monkeypatch, ['depthwise_forward', 'depthwise_dgrad', 'depthwise_wgrad'])
    rng = np.random.default_rng(k)
    b, h, w, c = 2, 6, 7, 67
    pads, (oh, ow) = ref.geometry(h, w, k, stride, padding)
    x = rng.standard_normal((b, h, w, c)).astype(np.float32)
    taps = rng.standard_normal((k * k, c)).astype(np.float32)
    dy = rng.standard_normal((b, oh, ow, c)).astype(np.float32)
    tx, tw = _dev(x, dev, gx), _dev(taps, dev, gw)
    y = _ag().depthwise(tx, tw, stride=stride, padding='same' if padding == 'same' else pads)
    assert tuple(y.shape) == (b, oh, ow, c)
    y.backward(_dev(dy, dev))
    torch.cuda.synchronize()
    assert calls.n == {'depthwise_forward': 1, 'depthwise_dgrad': int(gx), 'depthwise_wgrad': int(gw)}
    (dx64, dw64), (dx32, dw32) = ref.depthwise_grads(x, taps, dy, k, stride, padding), ref.depthwise_grads(x, taps, dy, k, stride, padding, np.float32)
    ok = [_within_bar('depthwise y', y, ref.depthwise(x, taps, k, stride, padding, np.float32), ref.depthwise(x, taps, k, stride, padding))]
    if gx:
        ok.append(_within_bar('depthwise dx', tx.grad, dx32, dx64))
    else:
        assert tx.grad is None
    if gw:
        ok.append(_within_bar('depthwise dw', tw.grad, dw32, dw64))
    else:
        assert tw.grad is None
    assert all(ok)


@pytest.mark.parametrize('act', [None, 'relu6', 'swish'])
def test_frozen_bn_act(dev, monkeypatch, act):
    calls = Calls(monkeypatch, ['bn_act_forward', 'bn_act_backward'])
    rng = np.random.default_rng(5)
    z = (3 * rng.standard_normal((2, 5, 7, 75))).astype(np.float32)
    scale, shift = rng.uniform(-2, 2, 75).astype(np.float32), rng.standard_normal(75).astype(np.float32)
    da = rng.standard_normal(z.shape).astype(np.float32)
    tz, ts, tb = _dev(z, dev, True), _dev(scale, dev), _dev(shift, dev)
    a = _ag().frozen_bn_act(tz, ts, tb, act)
    a.backward(_dev(da, dev))
    torch.cuda.synchronize()
    assert calls.n == {'bn_act_forward': 1, 'bn_act_backward': 1} and ts.grad is None and tb.grad is None
    a64, u64 = ref.bn_act(z, scale, shift, act)
    a32, u32 = ref.bn_act(z, scale, shift, act, np.float32)
    margin = float(min(np.abs(u64).min(), np.abs(u64 - 6).min()))
    assert float(np.abs(u64).max()) < 87.0 and (act != 'relu6' or margin > 1e-6), 'a kink of ReLU6 within 1e-6, or u beyond the clamp of expf'
    dz64, dz32 = ref.bn_act_backward(da, u32, scale, act), ref.bn_act_backward(da, u32, scale, act, np.float32)
    assert _within_bar('frozen_bn_act %s a' % act, a, a32, a64) and _within_bar('frozen_bn_act %s dz' % act, tz.grad, dz32, dz64)
    # a frozen z: nothing to differentiate, no backward kernel
    out = _ag().frozen_bn_act(_dev(z, dev), ts, tb, act)
    assert not out.requires_grad and calls.n['bn_act_backward'] == 1
    with pytest.raises(ValueError):
        _ag().frozen_bn_act(tz, _dev(scale, dev, True), tb, act)


def test_module_does_not_import_torch_functional():
    import os
    from yoloret_amd import autograd
    src = open(os.path.splitext(autograd.__file__)[0] + '.py').read()
    assert 'torch.nn' not in src and 'functional' not in src


# ----------------------------------------------------------------------------- composition
HW, BATCH, CLASSES = (96, 96), 2, 20
# the boxes of tests/test_gpu_headtrain.py
LABELS = [np.array([[10, 20, 70, 80, 3], [40, 8, 64, 60, 7], [50, 50, 62, 70, 0], [0, 0, 0, 0, 0]], np.float32),
          np.array([[2, 30, 90, 66, 11], [60, 60, 76, 90, 19], [5, 5, 15, 18, 1], [70, 10, 92, 34, 5]], np.float32)]
PARAMS = ('dw', 'wt1', 'wt2')
_shared = {}


def _case(dev):
    """the device's features of the one batch (float32 arrays), the labels, and the initial parameters; computed once, left unchanged"""
    if 'case' not in _shared:
        from oracle import params
        from yoloret_amd import layers as L
        from yoloret_amd.weights import synthetic_weights
        from yoloret_amd.yolo3.model import yolov3_body, yolov3_features
        from yoloret_amd.yolo3.utils import preprocess_true_boxes
        net = yolov3_body(L.Input(shape=[HW[0], HW[1], 3]), 'mobilenetv2x75', 3, num_classes=CLASSES)
        weights = synthetic_weights(net, 1234, 'conditioned')
        feats = yolov3_features(net)
        feats.set_weights(weights)
        images = torch.from_numpy(params.synthetic_images(BATCH, HW[0], HW[1])).to(dev)
        f = [t.clone().cpu().numpy() for t in feats(images)]
        assert [a.shape for a in f] == [(2, 3, 3, 75), (2, 6, 6, 75), (2, 12, 12, 75)]
        per_image = [preprocess_true_boxes(t, HW, ANCHORS, CLASSES, 3) for t in LABELS]
        y_np = [np.stack([per_image[i][s] for i in range(BATCH)]) for s in range(3)]
        rng = np.random.default_rng(77)
        init = []
        for s in range(3):
            init.append({'dw': (rng.standard_normal((9, 75)) / 3).astype(np.float32),
                         'scale1': rng.uniform(.5, 1.5, 75).astype(np.float32), 'shift1': (1 + rng.standard_normal(75)).astype(np.float32),
                         'wt1': ref.pack_wt(rng.standard_normal((75, 75)) / np.sqrt(75)),
                         'scale2': rng.uniform(.5, 1.5, 75).astype(np.float32), 'shift2': (.1 * rng.standard_normal(75)).astype(np.float32),
                         'wt2': ref.pack_wt(rng.standard_normal((75, 75)) / np.sqrt(75))})
        _shared['case'] = (f, y_np, init)
    return _shared['case']


def _device_stack(dev, f, y_np, par):
    """-> the loss (a 0-d device tensor attached to the graph) of the stack on every scale"""
    from yoloret_amd.yolo3.model import YoloLoss
    ag = _ag()
    total = None
    for s in range(3):
        p = par[s]
        t = ag.depthwise(f[s], p['dw'], 1, 'same')
        t = ag.frozen_bn_act(t, p['scale1'], p['shift1'], 'relu6')
        t = ag.linear1x1(t, p['wt1'])
        t = ag.frozen_bn_act(t, p['scale2'], p['shift2'], None)
        t = ag.linear1x1(t, p['wt2'])
        loss = YoloLoss(s, ANCHORS, 3, print_loss=False).call(y_np[s], t.reshape(t.shape[:3] + (3, 5 + CLASSES)))
        total = loss if total is None else total + loss
    return total


def _ref_stack(f, y_np, par, dt, info=None):
    """the same stack restated with torch on the CPU in ``dt``; par: {name: torch tensor} per scale (wt1 / wt2 as [75, 75])"""
    total = 0
    for s in range(3):
        p = par[s]
        x = torch.tensor(f[s], dtype=dt)
        u = ref._depthwise(x, p['dw'], 3, 1, (1, 1, 1, 1)) * p['scale1'] + p['shift1']
        t = ref._linear(torch.clamp(u, 0.0, 6.0).reshape(-1, 75), p['wt1'])
        t = ref._linear(t * p['scale2'] + p['shift2'], p['wt2'])
        out = t.reshape(y_np[s].shape)
        if info is not None:
            info.append((u.detach().numpy(), out.detach().numpy()))
        total = total + lossgrad_ref._forward(torch.tensor(y_np[s], dtype=dt), out, loss_ref.scale_anchors(ANCHORS, s), loss_ref.GRID_STEPS[s], .5)['loss']
    return total


def _ref_params(init, dt, grad=True):
    out = []
    for p in init:
        q = {k: torch.tensor(np.asarray(v, np.float64), dtype=dt) for k, v in p.items()}
        q['wt1'], q['wt2'] = q['wt1'][:, :75].clone(), q['wt2'][:, :75].clone()
        for k in PARAMS:
            q[k].requires_grad_(grad)
        out.append(q)
    return out


def _device_params(dev, init):
    return [{k: _dev(v, dev, k in PARAMS) for k, v in p.items()} for p in init]


def test_stack_gradients_against_float64(dev):
    """d loss / d every parameter of depthwise 3x3 -> BN + ReLU6 -> 1x1 -> BN -> 1x1 -> YoloLoss on the three scales' device features.
    Margins of the case (float64; loss threshold, coordinates, intersection sides, ReLU6 kinks): scale 0 (inf, inf, inf, 5.5e-4: no labelled
    box on the coarsest grid), scale 1 (3.7e-3, 2.1e-2, 1.8e-1, 1.0e-3), scale 2 (2.6e-1, 3.3e-2, 1.6e-2, 1.7e-5).
    Measured on an MI355X (device, E_ref, bar), d loss / d (dw, wt1, wt2):
    scale 0  6.358e-08, 1.079e-07, 4.911e-07;  8.842e-08, 8.842e-08, 4.133e-07;  1.135e-07, 1.135e-07, 5.134e-07
    scale 1  1.215e-07, 1.334e-07, 5.933e-07;  2.308e-07, 2.289e-07, 9.752e-07;  1.269e-07, 1.413e-07, 6.247e-07
    scale 2  1.135e-07, 1.491e-07, 6.561e-07;  1.051e-07, 4.826e-07, 1.990e-06;  1.629e-07, 3.631e-07, 1.512e-06"""
    f, y_np, init = _case(dev)
    info = []
    p64 = _ref_params(init, torch.float64)
    _ref_stack(f, y_np, p64, torch.float64, info).backward()
    for s, (u, logits) in enumerate(info):
        mg = lossgrad_ref.margins(logits, y_np[s], s)
        relu = float(min(np.abs(u).min(), np.abs(u - 6).min()))
        print('scale %d margins: threshold %.3e, coordinates %.3e, intersection sides %.3e, ReLU6 kinks %.3e' % ((s,) + mg + (relu,)))
        assert min(mg) > 1e-5 and relu > 1e-6, 'a kink lies too close - choose another case'
    p32 = _ref_params(init, torch.float32)
    _ref_stack(f, y_np, p32, torch.float32).backward()
    par = _device_params(dev, init)
    feats = [_dev(a, dev) for a in f]
    loss = _device_stack(dev, feats, y_np, par)
    loss.backward()
    torch.cuda.synchronize()
    ok = []
    for s in range(3):
        for k in PARAMS:
            g = par[s][k].grad
            assert g is not None and g.shape == par[s][k].shape
            if k != 'dw':
                assert not _bits(g[:, 75:]).any(), 'pad column of d %s' % k
                g = g[:, :75]
            ok.append(_within_bar('scale %d d loss / d %s' % (s, k), g, p32[s][k].grad.numpy(), p64[s][k].grad.numpy()))
        assert all(par[s][k].grad is None for k in ('scale1', 'shift1', 'scale2', 'shift2'))
    assert all(ok)


def _train(dev, steps=10, lr=1e-3):
    """-> (losses as 0-d device tensors, the parameters after the last step)"""
    rt = _rt()
    f, y_np, init = _case(dev)
    par = _device_params(dev, init)
    feats = [_dev(a, dev) for a in f]
    leaves = [par[s][k] for s in range(3) for k in PARAMS]
    moments = [(torch.zeros_like(w), torch.zeros_like(w)) for w in leaves]
    losses = []
    for t in range(1, steps + 1):
        loss = _device_stack(dev, feats, y_np, par)
        grads = torch.autograd.grad(loss, leaves)
        with torch.no_grad():
            for w, (m, v), g in zip(leaves, moments, grads):
                rt.adam_step(w, m, v, g.contiguous(), rt.adam_alpha(lr, t))
        losses.append(loss.detach())
    return losses, leaves


def test_ten_adam_steps_follow_the_float64_trajectory(dev):
    """One batch, learning rate 1e-3, the loss BEFORE each of 10 steps.  The float64 restatement (torch autograd on the CPU, float64 Adam
    of tests/headtrain_ref.py) is the yardstick; the device must agree with it at the two decimals at which row f-8 states its own
    trajectory (387.03 -> 275.11 next to the device's 387.0298 -> 275.1091): half a unit of the second decimal.  Why not more digits:
    yr_adam_step is Keras Adam in float32, whose 1 - beta2 is 0.0010000467 (tests/test_headtrain_host.py: relative 4.7e-5), so every
    step is 2.3e-5 shorter than the float64 one; with the loss falling by about 100 a step here that alone is 2e-3.
    Measured on an MI355X (float64 / device):
      489.7380 385.2986 300.8814 234.6883 184.4047 147.6103 121.3357 102.3385 88.6035 78.3363
      489.7380 385.2980 300.8804 234.6871 184.4035 147.6093 121.3348 102.3378 88.6029 78.3358"""
    f, y_np, init = _case(dev)
    p64 = _ref_params(init, torch.float64)
    leaves = [p64[s][k] for s in range(3) for k in PARAMS]
    mom = [(np.zeros(tuple(w.shape)), np.zeros(tuple(w.shape))) for w in leaves]
    want = []
    for t in range(1, 11):
        loss = _ref_stack(f, y_np, p64, torch.float64)
        grads = torch.autograd.grad(loss, leaves)
        want.append(float(loss.detach()))
        with torch.no_grad():
            for i, (w, g) in enumerate(zip(leaves, grads)):
                wn, m, v = headtrain_ref.adam_step64(w.numpy(), mom[i][0], mom[i][1], g.numpy(), 1e-3, t)
                mom[i] = (m, v)
                w.copy_(torch.from_numpy(wn))
    losses, _ = _train(dev)
    got = [float(v) for v in losses]
    print('float64: ' + ' '.join('%.4f' % v for v in want))
    print('device:  ' + ' '.join('%.4f' % v for v in got))
    assert want[-1] < want[0] and got[-1] < got[0]
    for a, b in zip(got, want):
        assert abs(a - b) <= 0.005, (a, b)


def test_two_training_runs_agree_bit_for_bit(dev):
    la, pa = _train(dev, steps=4)
    lb, pb = _train(dev, steps=4)
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(la, lb))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(pa, pb))
