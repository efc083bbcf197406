"""yoloret_amd.autograd.maxpool, upsample2, weighted_sum, concat and rfcr_module on the device: each Function alone under every
combination of gradient flags (no gradient kernel may run for an input that does not require one), the RFCR module (model.py:146-168)
on synthetic taps against float64 autograd of the restated module (tests/fusegrad_ref.py), and ten Adam steps through the module, a
1x1 convolution per scale and YoloLoss.

The bar is the project's own: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the float32 restatement's deviation from
float64 on the same inputs.  Every comparison prints its figures before it asserts (run with -s).

Not here: the agreement of rfcr_module(training=False) with the shipped inference plan on the model's own backbone taps.  A sub-model
whose outputs are the taps, or the three concatenations, does not compile (the plan compiler accepts only outputs produced by a 1x1
convolution), and the compiler is not changed for a test.  tests/test_gpu_layers_oracle.py compares it with the oracle's RFCR module
on the oracle's taps instead, which needs no plan."""
import itertools

import numpy as np
import pytest
import torch

from tests import bntrain_ref, convgrad_ref as cref, fusegrad_ref as ref, headtrain_ref, loss_ref, lossgrad_ref
from tests.test_gpu_autograd import Calls, _bits, _dev, _within_bar
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

F32 = np.float32


def _ag():
    from yoloret_amd import autograd
    return autograd


def _rt():
    from yoloret_amd import runtime
    return runtime


# ----------------------------------------------------------------------------- each Function alone
@pytest.mark.parametrize('k,h,w', [(2, 7, 9), (4, 9, 11)])
def test_maxpool(dev, monkeypatch, k, h, w):
    calls = Calls(monkeypatch, ['maxpool_forward', 'maxpool_backward'])
    rng = np.random.default_rng(k)
    x = np.clip(3 + 4 * rng.standard_normal((2, h, w, 75)), 0, 6).astype(F32)
    dy = rng.standard_normal((2, h // k, w // k, 75)).astype(F32)
    tx = _dev(x, dev, True)
    y = _ag().maxpool(tx, k)
    assert y.requires_grad and tuple(y.shape) == dy.shape
    y.backward(_dev(dy, dev))
    torch.cuda.synchronize()
    assert calls.n == {'maxpool_forward': 1, 'maxpool_backward': 1}
    y64, dx64 = ref.maxpool_grads64(x, dy, k)
    assert np.array_equal(_bits(y), y64.astype(F32).view(np.uint32)) and np.array_equal(_bits(tx.grad), dx64.astype(F32).view(np.uint32))
    # nothing requires a gradient: the forward alone
    y = _ag().maxpool(_dev(x, dev), k)
    assert not y.requires_grad and calls.n == {'maxpool_forward': 2, 'maxpool_backward': 1}
    # the default is k = 2
    assert tuple(_ag().maxpool(_dev(x, dev)).shape) == (2, h // 2, w // 2, 75)


def test_upsample2(dev, monkeypatch):
    calls = Calls(monkeypatch, ['upsample2_forward', 'upsample2_backward'])
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 7, 75)).astype(F32)
    dy = rng.standard_normal((2, 10, 14, 75)).astype(F32)
    tx = _dev(x, dev, True)
    y = _ag().upsample2(tx)
    assert y.requires_grad and tuple(y.shape) == dy.shape
    y.backward(_dev(dy, dev))
    torch.cuda.synchronize()
    assert calls.n == {'upsample2_forward': 1, 'upsample2_backward': 1}
    y64, dx64 = ref.upsample_grads64(x, dy)
    assert np.array_equal(_bits(y), y64.astype(F32).view(np.uint32))
    assert np.array_equal(_bits(tx.grad), ref.upsample_backward32(dy).view(np.uint32))
    assert _within_bar('upsample2 dx', tx.grad, ref.upsample_backward32(dy), dx64)
    y = _ag().upsample2(_dev(x, dev))
    assert not y.requires_grad and calls.n == {'upsample2_forward': 2, 'upsample2_backward': 1}


@pytest.mark.parametrize('ga', [True, False])
def test_weighted_sum(dev, monkeypatch, ga):
    """every combination of gradient flags of alpha and the four maps; 2 x 5 x 7 x 48.  The maps are saved for the backward only when
    alpha requires a gradient.  Measured on an MI355X: d alpha device 2.5e-07 against E_ref 1.4e-06 (bar 5.6e-06), the same bits whichever maps need a gradient."""
    rt = _rt()
    seen = []
    bwd = rt.wsum_backward
    monkeypatch.setattr(rt, 'wsum_backward', lambda dy, xs, alpha, **kw: (seen.append((xs is not None, tuple(kw['need']), kw['need_alpha'])),
                                                                          bwd(dy, xs, alpha, **kw))[1])
    calls = Calls(monkeypatch, ['wsum_forward'])
    rng = np.random.default_rng(4)
    shape = (2, 5, 7, 48)
    xs = [rng.standard_normal(shape).astype(F32) for _ in range(4)]
    alpha = np.array([1.25, -0.7, 0.0, 0.33], F32)
    dy = rng.standard_normal(shape).astype(F32)
    flat = [x.reshape(-1, 48) for x in xs]
    y64, dx64, da64 = ref.wsum_grads64(flat, alpha, dy.reshape(-1, 48))
    da32 = np.array([ref.seq_dot(dy.reshape(-1, 48), x) for x in flat], F32)
    ok = []
    for n, need in enumerate(itertools.product([True, False], repeat=4)):
        seen.clear()
        tx, ta = [_dev(x, dev, g) for x, g in zip(xs, need)], _dev(alpha, dev, ga)
        y = _ag().weighted_sum(tx, ta)
        assert np.array_equal(_bits(y), ref.wsum32(xs, alpha).view(np.uint32))
        if not (ga or any(need)):
            assert not y.requires_grad
            continue
        saved = y.grad_fn.saved_tensors
        assert len(saved) == (5 if ga else 1), 'the maps are kept only for d alpha'
        y.backward(_dev(dy, dev))
        torch.cuda.synchronize()
        assert seen == [(ga, need, ga)], 'one call, for exactly what requires a gradient'
        for i in range(4):
            if need[i]:
                assert np.array_equal(_bits(tx[i].grad), ref.wsum_dx32(dy, alpha)[i].view(np.uint32))
            else:
                assert tx[i].grad is None
        if ga:
            ok.append(_within_bar('weighted_sum d alpha, maps %r' % (need,), ta.grad, da32, da64))
        else:
            assert ta.grad is None
    assert all(ok) and calls.n['wsum_forward'] == 16
    with pytest.raises(ValueError):
        _ag().weighted_sum([_dev(xs[0], dev)] * 3, _dev(alpha, dev))


def test_concat(dev):
    """three sources of 24 / 96 / 7 channels under every combination of gradient flags: the forward is the bytes of the sources side
    by side, the backward hands out slices of dy"""
    rng = np.random.default_rng(5)
    widths = (24, 96, 7)
    xs = [rng.standard_normal((2, 3, 5, c)).astype(F32) for c in widths]
    dy = rng.standard_normal((2, 3, 5, sum(widths))).astype(F32)
    for need in itertools.product([True, False], repeat=3):
        tx = [_dev(x, dev, g) for x, g in zip(xs, need)]
        y = _ag().concat(tx)
        assert y.is_contiguous() and np.array_equal(_bits(y), np.concatenate(xs, -1).view(np.uint32))
        assert y.requires_grad == any(need)
        if not any(need):
            continue
        y.backward(_dev(dy, dev))
        at = 0
        for t, g, c in zip(tx, need, widths):
            if g:
                assert tuple(t.grad.shape) == tuple(t.shape) and np.array_equal(_bits(t.grad), np.ascontiguousarray(dy[..., at:at + c]).view(np.uint32))
            else:
                assert t.grad is None
            at += c
    with pytest.raises(ValueError):
        _ag().concat([_dev(xs[0], dev), _dev(xs[1][:, :2], dev)])


# ----------------------------------------------------------------------------- rfcr_module on synthetic taps
HW, BATCH, CLASSES = (96, 96), 2, 20
TAP_SHAPES = [(2, 3, 3, 120), (2, 6, 6, 72), (2, 12, 12, 24), (2, 6, 6, 24)]
SEED = 0
# the boxes of tests/test_gpu_headtrain.py
LABELS = [np.array([[10, 20, 70, 80, 3], [40, 8, 64, 60, 7], [50, 50, 62, 70, 0], [0, 0, 0, 0, 0]], np.float32),
          np.array([[2, 30, 90, 66, 11], [60, 60, 76, 90, 19], [5, 5, 15, 18, 1], [70, 10, 92, 34, 5]], np.float32)]
_shared = {}


def host_case(seed=SEED):
    """everything of the case that needs no device, computed once and left unchanged -> dict: taps (float32 arrays), params (the model's
    RFCR parameters in the operators' layouts, float32 arrays), functional (the three arrays of the loss sum_s <out_s, functional_s>),
    heads (1x1 weights [75, cin] per scale), labels"""
    if seed not in _shared:
        from yoloret_amd import autograd, layers as L
        from yoloret_amd.weights import synthetic_weights
        from yoloret_amd.yolo3.model import yolov3_body
        from yoloret_amd.yolo3.utils import preprocess_true_boxes
        net = yolov3_body(L.Input(shape=[HW[0], HW[1], 3]), 'mobilenetv2x75', 3, num_classes=CLASSES)
        net.set_weights(synthetic_weights(net, 1234, 'conditioned'))
        params = {k: v.detach().numpy().copy() for k, v in autograd.rfcr_parameters(net, 'cpu').items()}
        rng = np.random.default_rng(seed)
        taps = [rng.standard_normal(s).astype(F32) for s in TAP_SHAPES]
        out_shapes = [s[:3] + (s[3] + 96,) for s in TAP_SHAPES[:3]]
        functional = [rng.standard_normal(s).astype(F32) for s in out_shapes]
        heads = [cref.pack_wt(rng.standard_normal((75, s[3])) / np.sqrt(s[3])) for s in out_shapes]
        per_image = [preprocess_true_boxes(t, HW, ANCHORS, CLASSES, 3) for t in LABELS]
        labels = [np.stack([per_image[i][s] for i in range(BATCH)]) for s in range(3)]
        _shared[seed] = dict(taps=taps, params=params, functional=functional, heads=heads, labels=labels)
    return _shared[seed]


def ref_gradients(case, dtype):
    """the restated module in ``dtype`` on the CPU -> (record, {name: gradient array} for every trained parameter and 'b1', 'b2', 'b3')"""
    p = ref.rfcr_ref_params(case['params'], dtype)
    taps = [torch.tensor(np.asarray(t, np.float64), dtype=cref.DT[dtype], requires_grad=i < 3) for i, t in enumerate(case['taps'])]
    record = {}
    outs = ref.rfcr_module(*taps, p, record)
    loss = sum((o * torch.tensor(np.asarray(f, np.float64), dtype=cref.DT[dtype])).sum() for o, f in zip(outs, case['functional']))
    loss.backward()
    grads = {k: p[k].grad.numpy() for k in ref.RFCR_TRAINED}
    grads.update({'b%d' % (i + 1): taps[i].grad.numpy() for i in range(3)})
    return record, grads


def margins(rec64, rec32):
    """-> [(what, smallest distance of the float64 run from a decision, 8 x the float32 restatement's deviation there)]: the ReLU6 inputs'
    distance from 0 and 6, and the gap between the two largest values of every pooling window whose top two are not both clipped to
    the same bound"""
    out = []
    for bn in ('rfcr_sep_dw_BN', 'rfcr_sep_pw_BN'):
        u64, u32 = rec64[bn][0], rec32[bn][0]
        out.append(('ReLU6 of ' + bn, float(min(np.abs(u64).min(), np.abs(u64 - 6).min())), 8 * float(np.abs(u32 - u64).max())))
    for name in ('pool_b3c', 'pool_bc'):
        t64, t32 = rec64[name], rec32[name]
        gap, top, second = ref.top_two_gap(t64, 2)
        clipped = (top == second) & ((top == 0) | (top == 6))
        out.append(('max-pooling of ' + name[5:], float(gap[~clipped].min()), 8 * float(np.abs(t32 - t64).max())))
    return out


def test_rfcr_module_gradients_against_float64(dev):
    """B = 2, taps [2,3,3,120], [2,6,6,72], [2,12,12,24], [2,6,6,24] of standard normals, the parameters of a synthetic MobileNetV2 x 0.75
    model at 96 x 96, training=True; the loss a fixed random linear functional of the three outputs.  d loss / d every parameter
    (alpha included) and d loss / d b1, b2, b3.
    What the case provides (asserted on the float64 run; seed 0): the smallest distance from a decision against 8 x the float32
    restatement's deviation at that tensor -
      ReLU6 of rfcr_sep_dw_BN 6.253e-04 against 8.5e-06;  ReLU6 of rfcr_sep_pw_BN 4.054e-04 against 1.1e-05;
      max-pooling of b3c 4.658e-04 against 6.9e-06;  max-pooling of bc 3.295e-04 against 9.9e-06
    and every channel of the first BatchNorm is clipped by ReLU6 somewhere (row f-10 of DESIGN.md: a channel clipped nowhere has no
    gradient for its beta).
    Measured on an MI355X (device, E_ref, bar):
      rfcr_b1c 3.328e-07, 2.813e-07, 1.185e-06;  rfcr_b2c 3.805e-07, 3.647e-07, 1.519e-06;  rfcr_b3c 3.311e-07, 2.760e-07, 1.164e-06;
      rfcr_b4c 2.776e-07, 2.776e-07, 1.170e-06;  alpha 3.358e-07, 1.173e-07, 5.288e-07;  rfcr_sep_dw 2.760e-07, 2.597e-07, 1.098e-06;
      dw_BN gamma 2.840e-07, 3.389e-07, 1.415e-06;  dw_BN beta 2.751e-07, 3.208e-07, 1.343e-06;  rfcr_sep_pw 3.522e-07, 3.367e-07, 1.407e-06;
      pw_BN gamma 3.456e-07, 3.254e-07, 1.361e-06;  pw_BN beta 2.011e-07, 1.186e-07, 5.342e-07;
      b1 4.005e-07, 2.859e-07, 1.203e-06;  b2 2.304e-07, 2.797e-07, 1.178e-06;  b3 2.252e-07, 1.837e-07, 7.943e-07
    (the closest to its bar: alpha, 3.4e-07 against 5.3e-07); the moving statistics after the one forward 5.2e-08 .. 8.6e-08 of the float64 run's."""
    case = host_case()
    rec64, g64 = ref_gradients(case, np.float64)
    rec32, g32 = ref_gradients(case, np.float32)
    for what, distance, margin in margins(rec64, rec32):
        print('%s: smallest distance %.3e, margin %.3e' % (what, distance, margin))
        assert distance > margin, 'a decision lies too close - choose another seed'
    u1 = rec64['rfcr_sep_dw_BN'][0]
    assert (((u1 <= 0) | (u1 >= 6)).any(axis=0)).all(), 'a channel that ReLU6 clips nowhere'
    par = {k: _dev(v, dev, k in ref.RFCR_TRAINED) for k, v in case['params'].items()}
    taps = [_dev(t, dev, i < 3) for i, t in enumerate(case['taps'])]
    before = {k: par[k].clone() for k in ref.RFCR_MOVING}
    outs = _ag().rfcr_module(*taps, par, training=True)
    assert [tuple(o.shape) for o in outs] == [(2, 3, 3, 216), (2, 6, 6, 168), (2, 12, 12, 120)]
    loss = sum((o * _dev(f, dev)).sum() for o, f in zip(outs, case['functional']))
    loss.backward()
    torch.cuda.synchronize()
    ok = []
    for k in ref.RFCR_TRAINED:
        g = par[k].grad
        assert g is not None and g.shape == par[k].shape, k
        ok.append(_within_bar('d loss / d %s' % k, g, g32[k], g64[k]))
    for i in range(3):
        ok.append(_within_bar('d loss / d b%d' % (i + 1), taps[i].grad, g32['b%d' % (i + 1)], g64['b%d' % (i + 1)]))
    assert taps[3].grad is None and all(par[k].grad is None for k in ref.RFCR_MOVING)
    assert all(not torch.equal(par[k], before[k]) for k in ref.RFCR_MOVING), 'the moving statistics moved'
    # the moving statistics against the float64 run's batch statistics
    for bn in ('rfcr_sep_dw_BN', 'rfcr_sep_pw_BN'):
        _, mean, var, n = rec64[bn]
        mm, mv = bntrain_ref.moving64(case['params'][bn + '/moving_mean'], case['params'][bn + '/moving_variance'], mean, var, n, ref.BN_MOMENTUM)
        for name, want in (('moving_mean', mm), ('moving_variance', mv)):
            e = ref.rel_err(par['%s/%s' % (bn, name)].cpu().numpy(), want)
            print('%s/%s: relative deviation %.3e (bar 1e-6)' % (bn, name, e))
            ok.append(e <= 1e-6)
    assert all(ok)


def test_rfcr_module_evaluates_through_the_fold(dev):
    """training=False: the folded BatchNorms on the moving statistics; no gradient reaches gamma and beta, the moving statistics stay"""
    case = host_case()
    par = {k: _dev(v, dev, k in ref.RFCR_TRAINED) for k, v in case['params'].items()}
    taps = [_dev(t, dev) for t in case['taps']]
    outs = _ag().rfcr_module(*taps, par, training=False)
    sum(o.sum() for o in outs).backward()
    torch.cuda.synchronize()
    assert all(torch.equal(par[k], _dev(case['params'][k], dev)) for k in ref.RFCR_MOVING)
    assert all(par[k].grad is None for k in ref.RFCR_TRAINED if k.endswith(('gamma', 'beta'))) and par['rfcr_wsum/alpha'].grad is not None
    p = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in case['params'].items()}
    t64 = [torch.tensor(np.asarray(t, np.float64)) for t in case['taps']]
    # the restated module with the folded form in place of the batch statistics
    b1c, b2c, b3c, b4c = (ref._lin(t, p[n]) for t, n in zip(t64, ref.RFCR_CONVS))
    bc = ref._wsum([ref._upsample(b1c), b2c, ref._maxpool(b3c, 2), b4c], p['rfcr_wsum/alpha'])
    for conv, bn in ((lambda z: cref._depthwise(z, p['rfcr_sep_dw'], 5, 1, (2, 2, 2, 2)), 'rfcr_sep_dw_BN'), (lambda z: ref._lin(z, p['rfcr_sep_pw']), 'rfcr_sep_pw_BN')):
        scale, shift = bntrain_ref.fold64(*(p['%s/%s' % (bn, k)].numpy() for k in ('gamma', 'beta', 'moving_mean', 'moving_variance')), ref.BN_EPS)
        bc = torch.clamp(conv(bc) * torch.tensor(scale) + torch.tensor(shift), 0.0, 6.0)
    want = [torch.cat([t64[0], ref._maxpool(bc, 2)], -1), torch.cat([t64[1], bc], -1), torch.cat([t64[2], ref._upsample(bc)], -1)]
    for i, (o, w) in enumerate(zip(outs, want)):
        e = ref.rel_err(o.detach().cpu().numpy(), w.numpy())
        print('output %d: relative deviation %.3e (bar 1e-5)' % (i + 1, e))
        assert e <= 1e-5


# ----------------------------------------------------------------------------- training through the module
def _leaves(par, heads):
    return [par[k] for k in ref.RFCR_TRAINED] + list(heads)


def _device_loss(dev, taps, par, heads, labels):
    from yoloret_amd.yolo3.model import YoloLoss
    ag = _ag()
    outs = ag.rfcr_module(*taps, par, training=True)
    total = None
    for s in range(3):
        t = ag.linear1x1(outs[s], heads[s])
        loss = YoloLoss(s, ANCHORS, 3, print_loss=False).call(labels[s], t.reshape(tuple(t.shape[:3]) + (3, 5 + CLASSES)))
        total = loss if total is None else total + loss
    return total


def _train(dev, steps=10, lr=1e-3):
    """-> (losses as 0-d device tensors, the trained leaves, the moving statistics, alpha before the first step)"""
    rt = _rt()
    case = host_case()
    par = {k: _dev(v, dev, k in ref.RFCR_TRAINED) for k, v in case['params'].items()}
    heads = [_dev(h, dev, True) for h in case['heads']]
    taps = [_dev(t, dev) for t in case['taps']]
    leaves = _leaves(par, heads)
    moments = [(torch.zeros_like(w), torch.zeros_like(w)) for w in leaves]
    alpha0 = par['rfcr_wsum/alpha'].detach().clone()
    losses = []
    for t in range(1, steps + 1):
        loss = _device_loss(dev, taps, par, heads, case['labels'])
        grads = torch.autograd.grad(loss, leaves)
        with torch.no_grad():
            for w, (m, v), g in zip(leaves, moments, grads):
                rt.adam_step(w, m, v, g.contiguous(), rt.adam_alpha(lr, t))
        losses.append(loss.detach())
    return losses, leaves, [par[k] for k in ref.RFCR_MOVING], alpha0


def test_ten_adam_steps_follow_the_float64_trajectory(dev):
    """One batch, learning rate 1e-3, the loss BEFORE each of 10 steps; every parameter of the module and the three 1x1 heads trained,
    the moving statistics updated (momentum 0.99).  The yardstick is the float64 restatement (torch autograd on the CPU, float64 Adam of
    tests/headtrain_ref.py); the bar is row f-10's, from float32 Adam's 1 - beta2 = 0.0010000467 (relative 4.7e-5):
        |device - float64| <= 4.7e-5 * (the float64 run's total loss drop) + 2^-20 * (the first loss).
    Asserted on the float64 run before every step: every channel of the first BatchNorm is clipped by ReLU6 somewhere.
    Measured on an MI355X (float64 / device):
      460.1370 438.3800 416.6948 397.9865 380.5345 364.2440 348.5417 333.6888 319.7645 306.5112
      460.1370 438.3799 416.6945 397.9861 380.5341 364.2435 348.5411 333.6882 319.7638 306.5105
    largest deviation 7.482e-04 against a bar of 7.659e-03; the moving statistics 2.5e-07 .. 7.0e-07; alpha moved by 2.2e-03 .. 9.9e-03."""
    case = host_case()
    p64 = ref.rfcr_ref_params(case['params'], np.float64)
    heads = [torch.tensor(np.asarray(h, np.float64), requires_grad=True) for h in case['heads']]
    taps = [torch.tensor(np.asarray(t, np.float64)) for t in case['taps']]
    leaves = _leaves(p64, heads)
    mom = [(np.zeros(tuple(w.shape)), np.zeros(tuple(w.shape))) for w in leaves]
    want = []
    for t in range(1, 11):
        record = {}
        outs = ref.rfcr_module(*taps, p64, record)
        u1 = record['rfcr_sep_dw_BN'][0]
        assert (((u1 <= 0) | (u1 >= 6)).any(axis=0)).all(), 'a channel that ReLU6 clips nowhere: its beta has no gradient'
        loss = 0
        for s in range(3):
            logits = cref._linear(outs[s].reshape(-1, outs[s].shape[-1]), heads[s]).reshape(case['labels'][s].shape)
            loss = loss + lossgrad_ref._forward(torch.tensor(case['labels'][s], dtype=torch.float64), logits, loss_ref.scale_anchors(ANCHORS, s),
                                                loss_ref.GRID_STEPS[s], .5)['loss']
        grads = torch.autograd.grad(loss, leaves)
        want.append(float(loss.detach()))
        with torch.no_grad():
            for bn in ('rfcr_sep_dw_BN', 'rfcr_sep_pw_BN'):
                _, mean, var, n = record[bn]
                mm, mv = bntrain_ref.moving64(p64[bn + '/moving_mean'].numpy(), p64[bn + '/moving_variance'].numpy(), mean, var, n, ref.BN_MOMENTUM)
                p64[bn + '/moving_mean'].copy_(torch.from_numpy(mm))
                p64[bn + '/moving_variance'].copy_(torch.from_numpy(mv))
            for i, (w, g) in enumerate(zip(leaves, grads)):
                wn, m, v = headtrain_ref.adam_step64(w.numpy(), mom[i][0], mom[i][1], g.numpy(), 1e-3, t)
                mom[i] = (m, v)
                w.copy_(torch.from_numpy(wn))
    losses, dev_leaves, moving, alpha0 = _train(dev)
    got = [float(v) for v in losses]
    bar = 4.7e-5 * (want[0] - want[-1]) + 2.0 ** -20 * want[0]
    worst = max(abs(a - b) for a, b in zip(got, want))
    print('float64: ' + ' '.join('%.4f' % v for v in want))
    print('device:  ' + ' '.join('%.4f' % v for v in got))
    print('largest deviation %.3e, bar %.3e' % (worst, bar))
    assert want[-1] < want[0] and got[-1] < got[0]
    ok = worst <= bar
    for k, a in zip(ref.RFCR_MOVING, moving):
        e = ref.rel_err(a.cpu().numpy(), p64[k].numpy())
        print('%s: relative deviation %.3e (bar 1e-5)' % (k, e))
        ok = ok and e <= 1e-5
    alpha = dev_leaves[ref.RFCR_TRAINED.index('rfcr_wsum/alpha')]
    moved = (alpha.detach() - alpha0).abs().cpu().numpy()
    print('alpha moved by ' + ' '.join('%.3e' % v for v in moved))
    assert (moved > 0).all(), 'alpha has moved'
    assert ok


def test_two_training_runs_agree_bit_for_bit(dev):
    la, pa, ma, _ = _train(dev, steps=4)
    lb, pb, mb, _ = _train(dev, steps=4)
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(la, lb))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(pa, pb))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ma, mb))
