"""yolo3.model.yolov3_features and yolo3.train.OutputLayerTrainer on the plans a user gets and at other widths than 75 -> 75.

Plans: with the product defaults (small_batch 4, ksplit_batch 2, mbk_batch 24; tests/conftest.py pins the environment's to 0) a
batch of 1-2 images runs 'nohead_k', 3-4 'nohead', 5-23 'mid', 24 and more 'throughput' - in the feature model as in the body.  Only
the throughput plan merges a feature's two producers into one two-output convolution; the other three run them as separate ops.
Each variant is held to the float32 torch-CPU oracle (every image), to slot independence (image k and k + 2 are the same picture),
to workspace independence (tests/test_gpu_invariance.py's poisoned runs) and through one train step to the restatements of
tests/headtrain_ref.py.

Widths: 80 classes (255 -> 255 channels, kp 256: the blocked 4 x 4 grid of the gradient) and 1 class (18 -> 18, kp 20: TCO = TCI = 2)
at 64 x 64 (grids 2, 4, 8), through logits, one train_step_from_boxes, the float64 gradient of the loss and commit().

Rounding bars are the project's: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24.  Every figure is printed before it is
asserted (run with -s); the measured ones are in the docstrings."""
import numpy as np
import pytest
import torch

from oracle import params
from tests import headtrain_ref as ref, loss_ref, lossgrad_ref
from tests.test_gpu_headtrain import EPS24, LABELS, _bits, _rt, _scaled
from tests.test_gpu_invariance import _assert_same_bits, _oracle, _poisoned_runs
from tests.util import ANCHORS, assert_close

pytestmark = pytest.mark.gpu

NAME = 'mobilenetv2x75'
_shared = {}


def _build(size, classes):
    """(net with the oracle's parameters, the two synthetic images, the oracle's logits of them): computed once per (size, classes)
    and left unchanged - a test that trains builds its own net from the stored parameters."""
    from oracle import torch_ref
    key = (size, classes)
    if key not in _shared:
        P = params.ParamStore(1234, 'conditioned')
        x = params.synthetic_images(2, size, size)
        if classes == 20:
            want = _oracle(P, NAME, x)
        else:
            want = torch_ref.TorchReference(P, NAME, 3, classes)(x)
        _shared[key] = (P.values, x, want)
    values, x, want = _shared[key]
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3.model import yolov3_body
    net = yolov3_body(L.Input(shape=[size, size, 3]), NAME, 3, num_classes=classes)
    net.set_weights(values)
    return net, x, want


def _trainer(net, classes, **kw):
    from yoloret_amd.yolo3.train import OutputLayerTrainer
    return OutputLayerTrainer(net, ANCHORS, classes, 3, **kw)


def _labels(boxes, size, classes):
    """boxes [B,T,5] -> y_true arrays [B,G,G,3,5+C] per scale (the host encoder)"""
    from yoloret_amd.yolo3.utils import preprocess_true_boxes
    per_image = [preprocess_true_boxes(t, (size, size), ANCHORS, classes, 3) for t in boxes]
    return [np.stack([p[s] for p in per_image]) for s in range(3)]


def _np(t):
    return t.cpu().numpy()


def _check_step(tr, feats, dys, w0, what):
    """After ONE step from zero moments: the stored gradients are linear_wgrad(features, dY) byte for byte, (w, m, v) the Adam
    restatement of those bytes, pad columns +0."""
    rt = _rt()
    assert tr.step == 1
    for s, (cin, cout, kp) in enumerate(tr.dims):
        want = rt.linear_wgrad(feats[s], dys[s].reshape(tuple(feats[s].shape[:3]) + (cout,)))
        assert tr.grads[s].shape == (cout, kp)
        assert np.array_equal(_bits(_np(tr.grads[s])), _bits(_np(want))), '%s: gradient of scale %d' % (what, s)
    g = _np(tr.g)
    w, m, v = ref.adam_step(_np(w0), np.zeros_like(g), np.zeros_like(g), g, ref.adam_alpha(1e-3, 1))
    for name, got, exp in (('w', tr.w, w), ('m', tr.m, m), ('v', tr.v, v)):
        assert np.array_equal(_bits(_np(got)), _bits(exp)), '%s: %s' % (what, name)
    for s, (cin, cout, kp) in enumerate(tr.dims):
        for name, views in (('w', tr.weights), ('g', tr.grads), ('m', tr._views(tr.m)), ('v', tr._views(tr.v))):
            assert np.all(_bits(_np(views[s])[:, cin:]) == 0), '%s: pad columns of %s, scale %d, are not +0' % (what, name, s)


# ----------------------------------------------------------------------------- 4. the plans users get
PLAN_CASES = [(2, 'nohead_k'), (3, 'nohead'), (6, 'mid'), (24, 'throughput')]


@pytest.mark.parametrize('b,variant', PLAN_CASES, ids=['b%d-%s' % c for c in PLAN_CASES])
def test_features_and_trainer_on_every_plan_variant(dev, b, variant):
    """96 x 96, 20 classes, the two synthetic images cycled to b.  At 24 images the finest scale has 3456 pixels = 14 chunks of 256:
    the stored gradient of every scale against float64 dY^T X of the device's own features and dY.
    Measured on an MI355X (batch 24): scale 0 (P = 216) device 1.78e-07, E_ref 5.55e-07, bar 2.28e-06; scale 1 (P = 864) device
    1.48e-07, E_ref 6.17e-07, bar 2.53e-06; scale 2 (P = 3456) device 1.30e-07, E_ref 3.68e-07, bar 1.53e-06."""
    from yoloret_amd.yolo3 import model as M
    net, x2, want = _build(96, 20)
    tr = _trainer(net, 20)
    for m in (tr.model, tr.features):
        m.small_batch, m.ksplit_batch, m.mbk_batch = 4, 2, 24          # the product defaults (test_gpu_invariance._product_defaults)
    assert tr.features.variant(b) == variant and tr.model.variant(b) == variant
    what = 'features %s B=%d' % (variant, b)
    order = np.arange(b) % 2
    images = torch.from_numpy(np.ascontiguousarray(x2[order])).to(dev)

    # the oracle: every image
    ys = tr.logits(images)
    feats = tr.features(images)
    torch.cuda.synchronize()
    assert [tuple(f.shape) for f in feats] == [(b, g, g, 75) for g in (3, 6, 12)]
    for s, (y, r) in enumerate(zip(ys, want)):
        assert tuple(y.shape) == (b,) + r.shape[1:]
        for i in range(b):
            assert_close(_np(y[i]), r[order[i]], 1e-4, '%s image %d y%d' % (what, i, s + 1))

    # slot independence: image k and image k + 2 are the same picture
    for s in range(3):
        f, y = _np(feats[s]), _np(ys[s])
        for k in range(b - 2):
            assert np.array_equal(_bits(f[k]), _bits(f[k + 2])), '%s: features of scale %d differ between slots %d and %d' % (what, s, k, k + 2)
            assert np.array_equal(_bits(y[k]), _bits(y[k + 2])), '%s: logits of scale %d differ between slots %d and %d' % (what, s, k, k + 2)

    # workspace independence: NaN, large finite and random workspaces into NaN-filled dense outputs
    runs = _poisoned_runs(tr.features, images)
    _assert_same_bits(runs, what)                       # (finite everywhere: every element of the dense outputs was written)
    for s in range(3):
        assert runs[0][s].shape == (b, 3 << s, 3 << s, 75)
        assert np.array_equal(_bits(runs[0][s]), _bits(_np(feats[s]))), '%s: scale %d differs from the unpoisoned run' % (what, s)

    # one train step
    y_np = _labels([LABELS[i] for i in order], 96, 20)
    y_trues = [torch.from_numpy(y).to(dev) for y in y_np]
    total0, terms0, dys = M.yolo_loss_and_grad(ys, y_trues, ANCHORS, 3)
    w0 = tr.w.clone()
    loss = tr.train_step(images, y_trues)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.equal(loss, total0) and torch.equal(tr.last_terms, terms0)
    _check_step(tr, feats, dys, w0, what)

    if b == 24:
        assert feats[2].numel() // 75 == 3456 and _rt().linear_wgrad_chunk(3456, 75, 75) == 256
        for s in range(3):
            X, dY = _np(feats[s]).reshape(-1, 75), _np(dys[s]).reshape(-1, 75)
            r64 = ref.wgrad64(X, dY)
            e_ref = ref.rel_err(dY.T @ X, r64)
            e_dev = ref.rel_err(_np(tr.grads[s])[:, :75], r64)
            print('stored gradient B=24 scale %d (P=%d): device %.3e, NumPy float32 %.3e, bar %.3e' % (s, X.shape[0], e_dev, e_ref, 4 * e_ref + EPS24))
            assert e_dev <= 4 * e_ref + EPS24


# ----------------------------------------------------------------------------- 5. other widths
# Ground-truth boxes (x_min, y_min, x_max, y_max, class) in pixels of the 64 x 64 input, chosen on the CPU from the oracle's logits
# so that the float64 loss of either class count stays clear of its kinks (margins in the test's docstring).  The class ids are
# fractions of C - 1, so they span 0 .. C - 1.
WIDTH_BOXES = [np.array([[4, 6, 20, 30, 0.0], [30, 8, 62, 40, 1.0], [22, 40, 34, 58, 0.5], [0, 0, 0, 0, 0]], np.float32),
               np.array([[2, 2, 60, 50, 1.0], [40, 36, 52, 62, 0.0], [8, 34, 30, 48, 0.25], [44, 4, 56, 14, 0.75]], np.float32)]


def _width_boxes(classes):
    out = np.stack(WIDTH_BOXES).copy()
    out[..., 4] = np.round(out[..., 4] * (classes - 1))
    return out


@pytest.mark.parametrize('classes', [80, 1])
def test_trainer_at_other_widths(dev, classes):
    """No box of a 64 x 64 input lands on the coarsest grid (the largest box it holds matches the anchor 62 x 45 of scale 1 best), so
    part (c) runs on scales 1 and 2.  Margins of the cases (float64; threshold, coordinates, intersection sides): 80 classes scale 1
    (1.4e-3, 1.2e-1, 7.5e-1), scale 2 (2.9e-3, 4.8e-3, 1.0e-1); 1 class scale 1 (2.7e-2, 7.1e-3, 6.8e-1), scale 2 (4.8e-3, 2.2e-3,
    1.1e-1).  Measured on an MI355X, d loss / d W: 80 classes scale 1 device 1.51e-07, torch float32 1.51e-07, bar 6.62e-07; scale 2
    device 2.16e-07, torch float32 2.16e-07, bar 9.22e-07 (with 80 classes the largest error sits in a class row that one object
    cell feeds: a single product, rounded alike on both sides); 1 class scale 1 device 1.32e-07, torch float32 2.33e-07, bar
    9.90e-07; scale 2 device 8.12e-08, torch float32 2.11e-07, bar 9.04e-07.  Logits against the model's own plan: at most 9.5e-07
    (80 classes), 3.4e-07 (1 class); the same after commit()."""
    from yoloret_amd.yolo3 import model as M
    cw = 3 * (5 + classes)
    kp = (cw + 3) // 4 * 4
    net, x2, want = _build(64, classes)
    tr = _trainer(net, classes)
    assert tr.dims == [(cw, cw, kp)] * 3 and kp == {80: 256, 1: 20}[classes]
    assert tr.model.variant(2) == 'throughput' and tr.features.variant(2) == 'throughput'          # the suite's default plan
    images = torch.from_numpy(x2).to(dev)
    what = '%d classes' % classes

    # logits: against the model's own plan and against the oracle
    own = [y.clone() for y in tr.model(images)]
    ys = tr.logits(images)
    feats = tr.features(images)
    torch.cuda.synchronize()
    for s, (y, o, r) in enumerate(zip(ys, own, want)):
        assert tuple(y.shape) == (2, 2 << s, 2 << s, 3, 5 + classes) == tuple(o.shape) == r.shape
        err = _scaled(y, o)
        print('%s: trainer logits against the model\'s plan, scale %d: %.3e' % (what, s, err))
        assert err <= 1e-4
        assert_close(_np(y), r, 1e-4, '%s y%d against the oracle' % (what, s + 1))

    # the state's layout: scale s starts s * cout * kp floats into the one tensor, rows are kp apart
    host = tr.model.get_weights()
    for s, name in enumerate(tr.kernel_names):
        for flat, views in ((tr.w, tr.weights), (tr.g, tr.grads)):
            assert views[s].data_ptr() == flat.data_ptr() + 4 * s * cw * kp and tuple(views[s].shape) == (cw, kp) and views[s].stride() == (kp, 1)
        assert np.array_equal(_bits(_np(tr.weights[s])[:, :cw]), _bits(host[name].reshape(cw, cw).T))
    assert tr.w.numel() == 3 * cw * kp

    # one train_step_from_boxes
    boxes_np = _width_boxes(classes)
    assert boxes_np[..., 4].min() == 0 and boxes_np[..., 4].max() == classes - 1
    boxes = torch.from_numpy(boxes_np).to(dev)
    total0, terms0, dys = M.yolo_loss_and_grad_from_boxes(ys, boxes, ANCHORS, classes, 3)
    w0 = tr.w.clone()
    loss = tr.train_step_from_boxes(images, boxes)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and torch.equal(loss, total0) and torch.equal(tr.last_terms, terms0)
    print('%s: loss %.4f' % (what, float(loss)))
    _check_step(tr, feats, dys, w0, what)

    # d loss / d W against torch float64 autograd, on every scale where a box lands
    y_np = _labels(boxes_np, 64, classes)
    landed = [s for s in range(3) if y_np[s][..., 4].any()]
    assert len(landed) >= 2, 'the boxes land on scales %s only' % landed
    for s in landed:
        X = _np(feats[s]).reshape(-1, cw)
        W0 = _np(w0)[s * cw * kp:(s + 1) * cw * kp].reshape(cw, kp)[:, :cw]
        an, step = loss_ref.scale_anchors(ANCHORS, s), loss_ref.GRID_STEPS[s]
        logits = (X.astype(np.float64) @ W0.astype(np.float64).T).reshape(y_np[s].shape)
        mg = lossgrad_ref.margins(logits, y_np[s], s)
        print('%s scale %d margins threshold %.3e, coordinates %.3e, intersection sides %.3e' % ((what, s) + mg))
        assert min(mg) > 1e-5, 'a kink lies within 1e-5 - choose another case'
        grads = {}
        for dt in (torch.float64, torch.float32):
            Wt = torch.tensor(W0, dtype=dt, requires_grad=True)
            out = (torch.tensor(X, dtype=dt) @ Wt.T).reshape(y_np[s].shape)
            lossgrad_ref._forward(torch.tensor(y_np[s], dtype=dt), out, an, step, .5)['loss'].backward()
            grads[dt] = Wt.grad.numpy()
        e_ref = ref.rel_err(grads[torch.float32], grads[torch.float64])
        e_dev = ref.rel_err(_np(tr.grads[s])[:, :cw], grads[torch.float64])
        print('%s d loss / d W scale %d: device %.3e, torch float32 %.3e, bar %.3e' % (what, s, e_dev, e_ref, 4 * e_ref + EPS24))
        assert e_dev <= 4 * e_ref + EPS24

    # commit
    tr.commit()
    weights = tr.model.get_weights()
    for s, name in enumerate(tr.kernel_names):
        assert weights[name].shape == (1, 1, cw, cw)
        assert np.array_equal(_bits(weights[name].reshape(cw, cw)), _bits(_np(tr.weights[s])[:, :cw].T)), name
        assert not np.array_equal(weights[name], host[name])
    after = tr.logits(images)
    got = tr.model(images)
    torch.cuda.synchronize()
    for s in range(3):
        err = _scaled(got[s], after[s])
        print('%s: committed model scale %d: %.3e' % (what, s, err))
        assert err <= 1e-4
