"""``autograd.detector_neck``: everything ``yolov3_body`` runs behind the backbone (model.py:226-340), differentiated on the device, against
the restatements of tests/neck_ref.py.  2 images at 96 x 96 (maps of 3, 6 and 12), MobileNetV2 x0.75 and EfficientNet-B0, the parameters
those of ``layers_ref.rfcr_case`` taken through ``layers_ref.product_net`` + ``autograd.neck_parameters``.

The bar is the project's own: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the float32 torch restatement's deviation
from the float64 one on the same inputs; against the product's own plan the 1e-4 scaled bar of the float32 plans (tests/util.assert_close).
Every comparison prints its figures before it asserts (run with -s).  What the cases rest on is asserted without a device in
tests/test_neck_host.py."""
import numpy as np
import pytest
import torch

from oracle import params
from tests import bntrain_ref, headtrain_ref as href, layers_ref as lr, neck_ref as nr
from tests.test_gpu_autograd import _bits, _dev, _within_bar
from tests.test_gpu_headtrain import LABELS
from tests.util import ANCHORS, assert_close

pytestmark = pytest.mark.gpu


def _ag():
    from yoloret_amd import autograd
    return autograd


def _setup(dev, model_name):
    values = lr.rfcr_case(model_name)['P'].values
    net = lr.product_net(model_name, values)
    return net, _ag().neck_parameters(net, dev), nr.host_parameters(values)


def _tensors(par):
    return {(g, k): v for g, d in par.items() if g != 'cin' for k, v in d.items() if isinstance(v, torch.Tensor)}


def _images(dev):
    return torch.from_numpy(np.ascontiguousarray(params.synthetic_images(lr.BATCH, lr.RFCR_HW[0], lr.RFCR_HW[1]), np.float32)).to(dev)


@pytest.mark.parametrize('model_name', nr.MODELS)
def test_inference_is_the_oracles_and_the_plans(dev, model_name):
    """``detector_neck(training=False)`` on the oracle's taps: against the float64 restatement within the bar, against the product's own
    plan on the same images within 1e-4 scaled; no parameter changes.
    Measured on an MI355X (device, E_ref, bar / scaled error against the plan):
      MobileNetV2 x0.75  y1 5.598e-07, 5.432e-07, 2.232e-06 / 1.982e-06;  y2 1.015e-06, 9.657e-07, 3.922e-06 / 3.196e-06;  y3 6.671e-07, 7.039e-07, 2.875e-06 / 6.258e-06
      EfficientNet-B0    y1 4.184e-07, 3.583e-07, 1.493e-06 / 2.086e-07;  y2 5.392e-07, 3.909e-07, 1.623e-06 / 2.831e-07;  y3 5.436e-07, 6.248e-07, 2.559e-06 / 2.980e-07"""
    ag = _ag()
    net, par, host = _setup(dev, model_name)
    taps = lr.rfcr_case(model_name)['taps']
    t64, t32 = nr.torch_neck(host, taps, 'float64'), nr.torch_neck(host, taps, 'float32')
    before = {k: v.detach().clone() for k, v in _tensors(par).items()}
    with torch.no_grad():
        ys = ag.detector_neck(*[_dev(t, dev) for t in taps], par, training=False)
    plan = net(_images(dev))
    torch.cuda.synchronize()
    assert [tuple(y.shape) for y in ys] == [(lr.BATCH, s, s, 3, 25) for s in (3, 6, 12)]
    ok = [_within_bar('%s y%d' % (model_name, i + 1), y, t32['y'][i], t64['y'][i]) for i, y in enumerate(ys)]
    for i, (y, p) in enumerate(zip(ys, plan)):
        m = assert_close(y.cpu().numpy().reshape(-1), p.cpu().numpy().reshape(-1), 1e-4, '%s y%d against the plan' % (model_name, i + 1))
        print('%s y%d against the plan: scaled error %.3e' % (model_name, i + 1, m))
    for k, v in _tensors(par).items():
        assert np.array_equal(_bits(v), _bits(before[k])), 'nothing is updated: %s %s' % k
    assert all(ok)


def _check_grads(what, par, tx, g64, g32):
    ok = [_within_bar('%s d b%d' % (what, i + 1), t.grad, g32['taps'][i], g64['taps'][i]) for i, t in enumerate(tx)]
    for (g, k), want in g64['grads'].items():
        got = par[g][k].grad
        assert got is not None and tuple(got.shape) == want.shape, (g, k)
        name = k if g == 'rfcr' else g + k      # the Keras name of the layer
        if name in par['cin']:                  # a 1x1 kernel
            assert not _bits(got[:, par['cin'][name]:]).any(), 'pad columns of d %s %s are +0' % (g, k)
        ok.append(_within_bar('%s d %s %s' % (what, g, k), got, g32['grads'][(g, k)], want))
    return ok


@pytest.mark.parametrize('model_name', nr.MODELS)
def test_inference_gradients_against_float64(dev, model_name):
    """The gradients of sum_i (y_i * f_i).sum() for the four taps and every kernel and bias on the seeded taps, BatchNorms folded: gamma,
    beta and the moving statistics get none.
    Measured on an MI355X (device, E_ref, bar), the 4 taps' and 56 parameters' gradients per model, the closest to its bar and the farthest:
      MobileNetV2 x0.75  d bu1 _mb_se_reduce 1.374e-06, 7.773e-07, 3.169e-06 (0.43 of the bar);  d td3 _conv 4.731e-07, 1.561e-06, 6.305e-06
      EfficientNet-B0    d td1 _mb_se_expand/bias 1.874e-06, 9.356e-07, 3.802e-06 (0.49);  d td3 _conv 6.441e-07, 1.196e-06, 4.842e-06"""
    ag = _ag()
    _, par, host = _setup(dev, model_name)
    taps, fs = nr.seeded_taps(model_name, nr.GRAD_SEEDS[model_name])
    g64, g32 = nr.torch_neck(host, taps, 'float64', False, fs), nr.torch_neck(host, taps, 'float32', False, fs)
    tx = [_dev(t, dev, True) for t in taps]
    ys = ag.detector_neck(*tx, par, training=False)
    sum((y * _dev(f, dev)).sum() for y, f in zip(ys, fs)).backward()
    torch.cuda.synchronize()
    ok = [_within_bar('%s y%d' % (model_name, i + 1), y, g32['y'][i], g64['y'][i]) for i, y in enumerate(ys)]
    ok += _check_grads(model_name, par, tx, g64, g32)
    for (g, k), v in _tensors(par).items():
        if nr.is_bn_affine(k) or nr.is_moving(k):
            assert v.grad is None, 'folded: %s %s' % (g, k)
    assert all(ok)


def test_training_mode_gradients_and_moving_statistics(dev):
    """``detector_neck(training=True)`` on MobileNetV2 x0.75: every gradient, gamma and beta of all 24 BatchNorms included, against float64
    torch autograd over the training-mode restatement; the moving statistics move by ``bntrain_ref.moving64`` with momentum 0.9 in the
    four links and 0.99 elsewhere.  Their bar: moving' = moving (1 - d) + statistic d, so the device's deviation is float32's 2^-24 plus d
    times the statistic's (at most the forward bar, some 4e-6, at d <= 0.1): 1e-6 relative to the largest element.
    Measured on an MI355X (device, E_ref, bar): y1 3.148e-06, 3.323e-06, 1.335e-05;  y2 2.282e-06, 2.457e-06, 9.889e-06;  y3 2.369e-06,
    1.600e-06, 6.459e-06;  of the 108 gradients the closest to its bar is d bu2 _conv_BN/gamma 1.075e-05, 3.275e-06, 1.316e-05 (0.82 of it:
    the sum behind the gamma of a block's first BatchNorm cancels, float32 torch deviates likewise), the farthest d td3 _conv_BN/beta
    1.907e-06, 3.095e-06, 1.244e-05;  the 48 moving statistics between 2.525e-08 and 2.621e-07 (block_20 _BN/moving_variance)."""
    ag = _ag()
    model_name = nr.TRAIN_MODEL
    _, par, host = _setup(dev, model_name)
    taps, fs = nr.seeded_taps(model_name, nr.TRAIN_SEED)
    g64, g32 = nr.torch_neck(host, taps, 'float64', True, fs), nr.torch_neck(host, taps, 'float32', True, fs)
    assert len(g64['stats']) == 24
    tx = [_dev(t, dev, True) for t in taps]
    ys = ag.detector_neck(*tx, par, training=True)
    sum((y * _dev(f, dev)).sum() for y, f in zip(ys, fs)).backward()
    torch.cuda.synchronize()
    ok = [_within_bar('training y%d' % (i + 1), y, g32['y'][i], g64['y'][i]) for i, y in enumerate(ys)]
    ok += _check_grads('training', par, tx, g64, g32)
    assert sum(1 for g, k in g64['grads'] if nr.is_bn_affine(k)) == 48
    for (g, bn), (mean, var, n) in g64['stats'].items():
        momentum = ag.LINK_BN_MOMENTUM if g in nr.LINKS else 0.99
        mm, mv = bntrain_ref.moving64(host[g][bn + '/moving_mean'], host[g][bn + '/moving_variance'], mean, var, n, momentum)
        for part, want in (('moving_mean', mm), ('moving_variance', mv)):
            got = par[g]['%s/%s' % (bn, part)]
            assert not got.requires_grad and got.grad is None
            assert not np.array_equal(_bits(got), host[g]['%s/%s' % (bn, part)].view(np.uint32)), 'the moving statistics move: %s %s/%s' % (g, bn, part)
            e = href.rel_err(got.cpu().numpy(), want)
            print('%s %s/%s: relative deviation %.3e (bar 1e-6)' % (g, bn, part, e))
            ok.append(e <= 1e-6)
    for (g, k), v in _tensors(par).items():
        if not nr.is_moving(k):
            assert np.array_equal(_bits(v), host[g][k].view(np.uint32)), 'no trained parameter changes: %s %s' % (g, k)
    assert all(ok)


def test_ten_adam_steps_lower_the_loss_and_ship(dev):
    """Ten Adam steps (``runtime.adam_step``, lr 1e-3) over every trained tensor of the neck lower ``YoloLoss.call`` on a fixed batch, the
    labels encoded by ``preprocess_true_boxes_device``; afterwards ``neck_weights`` goes into ``model.set_weights`` and the plan's logits
    on the images equal ``detector_neck(training=False)`` on the oracle's taps (the backbone is frozen) within the 1e-4 scaled bar.
    Measured on an MI355X: the loss falls 487.16, 444.11, 416.37, 398.92, 387.98, 376.76, 370.13, 361.84, 355.35, 349.08; the plan's
    logits after the round trip differ by 1.997e-06, 2.876e-06 and 4.470e-06 scaled."""
    from yoloret_amd import runtime as rt
    from yoloret_amd.yolo3.model import YoloLoss
    from yoloret_amd.yolo3.utils import preprocess_true_boxes_device
    ag = _ag()
    model_name = nr.TRAIN_MODEL
    net, par, host = _setup(dev, model_name)
    taps = [_dev(t, dev) for t in lr.rfcr_case(model_name)['taps']]
    labels = preprocess_true_boxes_device(np.stack(LABELS), lr.RFCR_HW, ANCHORS, lr.CLASSES, 3, device=dev)
    leaves = [v for v in _tensors(par).values() if v.requires_grad]
    assert len(leaves) == len(nr.trained_keys(host, True))
    moments = [(torch.zeros_like(w), torch.zeros_like(w)) for w in leaves]
    losses = []
    for t in range(1, 11):
        ys = ag.detector_neck(*taps, par, training=True)
        loss = sum(YoloLoss(s, ANCHORS, 3, print_loss=False).call(labels[s], ys[s]) for s in range(3))
        grads = torch.autograd.grad(loss, leaves)
        with torch.no_grad():
            for w, (m, v), g in zip(leaves, moments, grads):
                rt.adam_step(w, m, v, g.contiguous(), rt.adam_alpha(1e-3, t))
        losses.append(loss.detach())
    losses = [float(v) for v in torch.stack([l.reshape(()) for l in losses]).cpu()]
    print('loss over ten steps: ' + ' '.join('%.4f' % v for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    changed = sum(1 for (g, k), v in _tensors(par).items() if not np.array_equal(_bits(v), host[g][k].view(np.uint32)))
    assert changed == len(_tensors(par)), 'every trained tensor and every moving statistic has moved'
    # what was trained is what is shipped
    w = net.get_weights()
    w.update(ag.neck_weights(par))
    net.set_weights(w)
    with torch.no_grad():
        ys = ag.detector_neck(*taps, par, training=False)
    plan = net(_images(dev))
    torch.cuda.synchronize()
    for i, (y, p) in enumerate(zip(ys, plan)):
        m = assert_close(p.cpu().numpy().reshape(-1), y.cpu().numpy().reshape(-1), 1e-4, 'the plan\'s y%d after training' % (i + 1))
        print('the plan\'s y%d after training: scaled error %.3e' % (i + 1, m))
