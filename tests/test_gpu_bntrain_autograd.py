"""yoloret_amd.autograd.batchnorm_act and fold_batchnorm on the device: the Function alone against the float64 restatement of
tests/bntrain_ref.py, and the stack of tests/test_gpu_autograd.py with both BatchNorms in TRAINING mode - depthwise 3x3 -> BN + ReLU6 ->
1x1 -> BN -> 1x1 -> YoloLoss on the three scales' device features (96 x 96, batch 2: 18, 72 and 288 pixels a scale) - trained with
runtime.adam_step, gamma and beta included, the moving statistics following along.

The bar is the project's own: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the float32 restatement's deviation from
float64 on the same inputs.  Every comparison prints its figures before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

from tests import bntrain_ref as ref, convgrad_ref as cref, headtrain_ref, loss_ref, lossgrad_ref
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
F32 = np.float32
BN_EPS, MOMENTUM = 1e-3, 0.9


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
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    e_dev, e_ref = ref.rel_err(got, r64), ref.rel_err(r32, r64)
    print('%s: device %.3e, float32 restatement %.3e, bar %.3e' % (what, e_dev, e_ref, 4 * e_ref + EPS24))
    return e_dev <= 4 * e_ref + EPS24


# ----------------------------------------------------------------------------- the Function alone
def _alone_case():
    rng = np.random.default_rng(11)
    c = 75
    z = (rng.uniform(-20, 20, c)[None, None, None, :] + rng.uniform(.1, 2, c)[None, None, None, :] * rng.standard_normal((2, 5, 7, c))).astype(F32)
    gamma = (rng.uniform(.5, 1.5, c) * rng.choice([-1, 1], c)).astype(F32)
    beta = (1 + rng.standard_normal(c)).astype(F32)
    da = rng.standard_normal(z.shape).astype(F32)
    return z, gamma, beta, da


@pytest.mark.parametrize('gz,gg,gb', [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True),
                                      (True, False, True), (True, True, False)])
@pytest.mark.parametrize('act', [None, 'relu6', 'swish'])
def test_batchnorm_act(dev, monkeypatch, act, gz, gg, gb):
    """70 pixels, 75 channels, offsets up to 20 next to spreads of 0.1 .. 2.  Measured on an MI355X (device, E_ref, bar), act None / relu6 / swish:
    a            8.918e-07, 1.301e-06, 5.265e-06;  1.070e-06, 1.510e-06, 6.101e-06;  9.868e-07, 1.377e-06, 5.569e-06
    dz           5.111e-07, 5.111e-07, 2.104e-06;  5.142e-07, 5.848e-07, 2.399e-06;  1.512e-06, 2.075e-06, 8.358e-06
    dgamma       3.362e-06, 4.641e-06, 1.863e-05;  5.720e-06, 8.360e-06, 3.350e-05;  3.417e-06, 4.048e-06, 1.625e-05
    dbeta        9.245e-08, 4.639e-07, 1.915e-06;  1.527e-07, 4.581e-07, 1.892e-06;  7.166e-07, 1.593e-06, 6.430e-06
    moving_mean  3.290e-07, 5.762e-07, 2.365e-06;  moving_var 1.002e-07, 1.351e-07, 5.999e-07 (the same for every activation)"""
    rt = _rt()
    seen = []
    fwd, bwd = rt.bn_train_forward, rt.bn_train_backward
    monkeypatch.setattr(rt, 'bn_train_forward', lambda *a, **kw: (seen.append(('forward', None)), fwd(*a, **kw))[1])
    monkeypatch.setattr(rt, 'bn_train_backward', lambda *a, **kw: (seen.append(('backward', kw.get('need_dz'))), bwd(*a, **kw))[1])
    z, gamma, beta, da = _alone_case()
    tz, tg, tb = _dev(z, dev, gz), _dev(gamma, dev, gg), _dev(beta, dev, gb)
    mm, mv = torch.zeros(75, device=dev), torch.ones(75, device=dev)
    a = _ag().batchnorm_act(tz, tg, tb, mm, mv, MOMENTUM, BN_EPS, act)
    assert a.requires_grad and tuple(a.shape) == z.shape
    a.backward(_dev(da, dev))
    torch.cuda.synchronize()
    assert seen == [('forward', None), ('backward', gz)], 'dz is computed only when z needs a gradient'
    z2, da2 = z.reshape(-1, 75), da.reshape(-1, 75)
    r64, r32 = ref.forward64(z2, gamma, beta, BN_EPS, act), ref.forward32(z2, gamma, beta, BN_EPS, MOMENTUM, act, np.zeros(75, F32), np.ones(75, F32))
    margin = float(min(np.abs(r64['u']).min(), np.abs(r64['u'] - 6).min()))
    assert float(np.abs(r64['u']).max()) < 87.0 and (act != 'relu6' or margin > 1e-6), 'a kink of ReLU6 within 1e-6, or u beyond the clamp of expf'
    g64 = ref.backward64(da2, z2, gamma, beta, BN_EPS, act)
    g32 = ref.backward32(da2, z2, gamma, beta, r32['mean'], r32['invstd'], act)
    m64 = ref.moving64(np.zeros(75), np.ones(75), r64['mean'], r64['var'], z2.shape[0], MOMENTUM)
    ok = [_within_bar('batchnorm_act %s a' % act, a.reshape(-1, 75), r32['a'], r64['a']),
          _within_bar('batchnorm_act %s moving_mean' % act, mm, r32['moving_mean'], m64[0]),
          _within_bar('batchnorm_act %s moving_var' % act, mv, r32['moving_var'], m64[1])]
    for name, t, want, i in (('dz', tz, gz, 0), ('dgamma', tg, gg, 1), ('dbeta', tb, gb, 2)):
        if want:
            ok.append(_within_bar('batchnorm_act %s %s' % (act, name), t.grad.reshape(g64[i].shape), g32[i], g64[i]))
        else:
            assert t.grad is None
    assert all(ok)


def test_batchnorm_act_arguments(dev):
    z, gamma, beta, _ = _alone_case()
    tz, tg, tb = _dev(z, dev), _dev(gamma, dev), _dev(beta, dev)
    ag = _ag()
    out = ag.batchnorm_act(tz, tg, tb, act='relu6')          # nothing requires a gradient, no moving statistics
    assert not out.requires_grad and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        ag.batchnorm_act(tz, tg, tb, torch.zeros(75, device=dev, requires_grad=True), torch.ones(75, device=dev))
    with pytest.raises(ValueError):
        ag.batchnorm_act(tz, tg, tb, torch.zeros(75, device=dev), None)
    with pytest.raises(ValueError):
        ag.batchnorm_act(tz, tg, tb, act='sigmoid')
    with pytest.raises(ValueError):
        ag.frozen_bn_act(tz, _dev(gamma, dev, True), tb, None)          # still frozen


@pytest.mark.parametrize('act', [None, 'relu6', 'swish'])
def test_fold_batchnorm_then_frozen_bn_act(dev, act):
    """Measured on an MI355X (device, E_ref, bar): None 2.779e-07, 2.779e-07, 1.171e-06; relu6 1.295e-06, 1.295e-06, 5.240e-06; swish
    3.422e-07, 3.422e-07, 1.428e-06 (the folded vectors are bit-equal, so the device and the float32 restatement share every rounding)."""
    z, gamma, beta, _ = _alone_case()
    rng = np.random.default_rng(3)
    mean, var = z.reshape(-1, 75).mean(0).astype(F32), rng.uniform(.01, 4, 75).astype(F32)
    scale, shift = _ag().fold_batchnorm(_dev(gamma, dev), _dev(beta, dev), _dev(mean, dev), _dev(var, dev), BN_EPS)
    assert scale.dtype == torch.float32 and scale.device.type == 'cuda' and tuple(scale.shape) == tuple(shift.shape) == (75,)
    s64, b64 = ref.fold64(gamma, beta, mean, var, BN_EPS)
    assert np.array_equal(scale.cpu().numpy(), s64.astype(F32)) and np.array_equal(shift.cpu().numpy(), b64.astype(F32))
    a = _ag().frozen_bn_act(_dev(z, dev), scale, shift, act)
    a64, u64 = cref.bn_act(z, s64, b64, act)
    a32, _ = cref.bn_act(z, s64.astype(F32), b64.astype(F32), act, np.float32)
    assert act != 'relu6' or min(np.abs(u64).min(), np.abs(u64 - 6).min()) > 1e-6
    assert _within_bar('fold_batchnorm + frozen_bn_act %s' % act, a, a32, a64)


def test_module_still_does_not_import_torch_functional():
    import os
    from yoloret_amd import autograd
    src = open(os.path.splitext(autograd.__file__)[0] + '.py').read()
    assert 'torch.nn' not in src and 'functional' not in src


# ----------------------------------------------------------------------------- composition
HW, BATCH, CLASSES = (96, 96), 2, 20
# the boxes of tests/test_gpu_headtrain.py
LABELS = [np.array([[10, 20, 70, 80, 3], [40, 8, 64, 60, 7], [50, 50, 62, 70, 0], [0, 0, 0, 0, 0]], np.float32),
          np.array([[2, 30, 90, 66, 11], [60, 60, 76, 90, 19], [5, 5, 15, 18, 1], [70, 10, 92, 34, 5]], np.float32)]
PARAMS = ('dw', 'gamma1', 'beta1', 'wt1', 'gamma2', 'beta2', 'wt2')
MOVING = ('mm1', 'mv1', 'mm2', 'mv2')
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
                         'gamma1': rng.uniform(.5, 1.5, 75).astype(np.float32), 'beta1': rng.uniform(-.5, .5, 75).astype(np.float32),      # (every channel clipped somewhere: see the trajectory test)
                         'wt1': cref.pack_wt(rng.standard_normal((75, 75)) / np.sqrt(75)),
                         'gamma2': rng.uniform(.5, 1.5, 75).astype(np.float32), 'beta2': (.1 * rng.standard_normal(75)).astype(np.float32),
                         'wt2': cref.pack_wt(rng.standard_normal((75, 75)) / np.sqrt(75)),
                         'mm1': np.zeros(75, np.float32), 'mv1': np.ones(75, np.float32), 'mm2': np.zeros(75, np.float32), 'mv2': np.ones(75, np.float32)})
        _shared['case'] = (f, y_np, init)
    return _shared['case']


def _device_stack(dev, f, y_np, par, training=True):
    """-> the loss (a 0-d device tensor attached to the graph) of the stack on every scale; training: BatchNorm on batch statistics, the
    moving statistics of ``par`` updated in place; else the folded inference form"""
    from yoloret_amd.yolo3.model import YoloLoss
    ag = _ag()
    total = None
    for s in range(3):
        p = par[s]
        t = ag.depthwise(f[s], p['dw'], 1, 'same')
        if training:
            t = ag.batchnorm_act(t, p['gamma1'], p['beta1'], p['mm1'], p['mv1'], MOMENTUM, BN_EPS, 'relu6')
        else:
            t = ag.frozen_bn_act(t, *ag.fold_batchnorm(p['gamma1'], p['beta1'], p['mm1'], p['mv1'], BN_EPS), 'relu6')
        t = ag.linear1x1(t, p['wt1'])
        if training:
            t = ag.batchnorm_act(t, p['gamma2'], p['beta2'], p['mm2'], p['mv2'], MOMENTUM, BN_EPS, None)
        else:
            t = ag.frozen_bn_act(t, *ag.fold_batchnorm(p['gamma2'], p['beta2'], p['mm2'], p['mv2'], BN_EPS), None)
        t = ag.linear1x1(t, p['wt2'])
        loss = YoloLoss(s, ANCHORS, 3, print_loss=False).call(y_np[s], t.reshape(t.shape[:3] + (3, 5 + CLASSES)))
        total = loss if total is None else total + loss
    return total


def _ref_stack(f, y_np, par, dt, info=None, stats=None):
    """the same stack, training mode, restated with torch on the CPU in ``dt``; par: {name: torch tensor} per scale (wt1 / wt2 as [75, 75]).
    stats receives per scale (mean1, var1, mean2, var2, pixels) of the batch."""
    total = 0
    for s in range(3):
        p = par[s]
        x = torch.tensor(f[s], dtype=dt)
        z1 = cref._depthwise(x, p['dw'], 3, 1, (1, 1, 1, 1)).reshape(-1, 75)
        u, _, m1, v1, _ = ref._forward64(z1, p['gamma1'], p['beta1'], BN_EPS)
        z2 = cref._linear(torch.clamp(u, 0.0, 6.0), p['wt1'])
        t, _, m2, v2, _ = ref._forward64(z2, p['gamma2'], p['beta2'], BN_EPS)
        out = cref._linear(t, p['wt2']).reshape(y_np[s].shape)
        if info is not None:
            info.append((u.detach().numpy(), out.detach().numpy()))
        if stats is not None:
            stats.append(tuple(v.detach().numpy() for v in (m1, v1, m2, v2)) + (z1.shape[0],))
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
    """d loss / d every parameter - seven kinds a scale - of the training-mode stack.
    Margins of the case (float64; loss threshold, coordinates, intersection sides,
    ReLU6 kinks): scale 0 (inf, inf, inf, 5.0e-5: no labelled box on the coarsest grid), scale 1 (1.3e-2, 1.3e-2, 1.1e-1, 2.1e-5), scale 2
    (3.6e-2, 3.9e-3, 4.2e-2, 3.7e-5).  Measured on an MI355X (device, E_ref, bar), d loss / d (dw, gamma1, beta1, wt1, gamma2, beta2, wt2):
    scale 0  5.318e-07, 5.082e-07, 2.092e-06;  3.506e-07, 3.000e-07, 1.260e-06;  9.439e-07, 7.799e-07, 3.179e-06;  4.913e-07, 4.055e-07, 1.681e-06;
             5.728e-07, 6.863e-07, 2.805e-06;  1.511e-07, 6.640e-08, 3.252e-07;  4.925e-07, 4.011e-07, 1.664e-06
    scale 1  3.493e-07, 3.493e-07, 1.457e-06;  4.799e-07, 4.129e-07, 1.711e-06;  5.178e-07, 4.562e-07, 1.884e-06;  5.506e-07, 2.970e-07, 1.248e-06;
             3.704e-07, 3.007e-07, 1.262e-06;  1.990e-07, 1.072e-07, 4.886e-07;  3.640e-07, 3.188e-07, 1.335e-06
    scale 2  1.867e-07, 2.617e-07, 1.106e-06;  5.285e-07, 3.841e-07, 1.596e-06;  7.017e-07, 6.014e-07, 2.465e-06;  8.062e-07, 8.107e-07, 3.302e-06;
             7.299e-07, 4.046e-07, 1.678e-06;  1.069e-07, 7.981e-08, 3.788e-07;  4.874e-07, 4.835e-07, 1.994e-06"""
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
            if k in ('wt1', 'wt2'):
                assert not _bits(g[:, 75:]).any(), 'pad column of d %s' % k
                g = g[:, :75]
            ok.append(_within_bar('scale %d d loss / d %s' % (s, k), g, p32[s][k].grad.numpy(), p64[s][k].grad.numpy()))
        assert all(par[s][k].grad is None for k in MOVING)
    assert all(ok)


def _train(dev, steps=10, lr=1e-3):
    """-> (losses as 0-d device tensors, the parameters after the last step, the moving statistics after the last step)"""
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
    return losses, leaves, [par[s][k] for s in range(3) for k in MOVING], par


def test_ten_adam_steps_follow_the_float64_trajectory(dev):
    """One batch, learning rate 1e-3, the loss BEFORE each of 10 steps, every parameter of the stack trained and the moving statistics
    updated (momentum 0.9, from mean 0 / variance 1).  The float64 restatement (torch autograd on the CPU, float64 Adam of
    tests/headtrain_ref.py) is the yardstick.  The bar comes from float32 Adam alone, as in tests/test_gpu_autograd.py: yr_adam_step is
    Keras Adam in float32, whose 1 - beta2 is 0.0010000467 (relative 4.7e-5), so the device's steps differ from the float64 ones by
    that fraction and the loss, to first order, by that fraction of what the steps achieve:
        |device - float64| <= 4.7e-5 * (the float64 run's total loss drop) + 2^-20 * (the first loss),
    the second term for the float32 evaluation of the loss itself.  The moving statistics after ten steps: 1e-5 relative (max-norm).
    What the case must provide (asserted on the float64 run before every step): every channel of the first BatchNorm is clipped by
    ReLU6 at some pixel.  A channel that is clipped nowhere passes beta1 straight into the mean of the 1x1 convolution's output, which
    the second BatchNorm removes: d loss / d beta1 is then 0 in exact arithmetic and rounding noise in any floating-point run (1e-17 of
    the largest element in float64), and Adam, which divides by the gradient's own magnitude, turns the SIGN of that noise into steps
    of the full learning rate - in float64 as well as on the device.  Two runs then disagree in beta1 by about the learning rate and in
    the second moving mean by 1e-4 .. 1e-3 relative, with the same loss; a CPU run of the float32 restatement shows the same.  That is
    why beta1 starts in [-0.5, 0.5] here, not around 1 as shift1 of tests/test_gpu_autograd.py.
    Measured on an MI355X (float64 / device): largest deviation 3.569e-04 against a bar of 4.383e-03; the moving statistics 8.3e-08 .. 1.4e-06
    (the largest: scale 1, second moving mean).
      497.6894 485.0184 473.4051 462.7359 453.2676 444.2685 435.9577 428.6172 421.4782 414.5328
      497.6894 485.0183 473.4050 462.7357 453.2673 444.2682 435.9574 428.6169 421.4779 414.5324"""
    f, y_np, init = _case(dev)
    p64 = _ref_params(init, torch.float64)
    leaves = [p64[s][k] for s in range(3) for k in PARAMS]
    mom = [(np.zeros(tuple(w.shape)), np.zeros(tuple(w.shape))) for w in leaves]
    want = []
    for t in range(1, 11):
        stats, info = [], []
        loss = _ref_stack(f, y_np, p64, torch.float64, info, stats)
        assert all((((u <= 0) | (u >= 6)).any(axis=0)).all() for u, _ in info), 'a channel that ReLU6 clips nowhere: its beta1 has no gradient'
        grads = torch.autograd.grad(loss, leaves)
        want.append(float(loss.detach()))
        with torch.no_grad():
            for s, (m1, v1, m2, v2, n) in enumerate(stats):
                for km, kv, m, v in (('mm1', 'mv1', m1, v1), ('mm2', 'mv2', m2, v2)):
                    nm, nv = ref.moving64(p64[s][km].numpy(), p64[s][kv].numpy(), m, v, n, MOMENTUM)
                    p64[s][km].copy_(torch.from_numpy(nm))
                    p64[s][kv].copy_(torch.from_numpy(nv))
            for i, (w, g) in enumerate(zip(leaves, grads)):
                wn, m, v = headtrain_ref.adam_step64(w.numpy(), mom[i][0], mom[i][1], g.numpy(), 1e-3, t)
                mom[i] = (m, v)
                w.copy_(torch.from_numpy(wn))
    losses, _, moving, _ = _train(dev)
    got = [float(v) for v in losses]
    bar = 4.7e-5 * (want[0] - want[-1]) + 2.0 ** -20 * want[0]
    worst = max(abs(a - b) for a, b in zip(got, want))
    print('float64: ' + ' '.join('%.4f' % v for v in want))
    print('device:  ' + ' '.join('%.4f' % v for v in got))
    print('largest deviation %.3e, bar %.3e' % (worst, bar))
    assert want[-1] < want[0] and got[-1] < got[0]
    ok = worst <= bar
    want_moving = [p64[s][k].numpy() for s in range(3) for k in MOVING]
    for i, (a, b) in enumerate(zip(moving, want_moving)):
        e = ref.rel_err(a.cpu().numpy(), b)
        print('scale %d %s: relative deviation %.3e (bar 1e-5)' % (i // 4, MOVING[i % 4], e))
        ok = ok and e <= 1e-5
    assert ok


def test_two_training_runs_agree_bit_for_bit(dev):
    la, pa, ma, _ = _train(dev, steps=4)
    lb, pb, mb, _ = _train(dev, steps=4)
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(la, lb))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(pa, pb))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ma, mb))


def test_trained_stack_evaluates_through_the_fold(dev):
    """after training: fold_batchnorm + frozen_bn_act give the validation-style forward of the same stack"""
    f, y_np, _ = _case(dev)
    _, _, moving, par = _train(dev, steps=4)
    assert all(bool(torch.isfinite(m).all()) for m in moving) and all(bool((par[s]['mv1'] > 0).all() and (par[s]['mv2'] > 0).all()) for s in range(3))
    with torch.no_grad():
        loss = _device_stack(dev, [_dev(a, dev) for a in f], y_np, par, training=False)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and float(loss) > 0
    assert all(not bool((par[s]['mm1'] == 0).all()) for s in range(3)), 'the moving mean moved'
