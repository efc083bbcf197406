"""Host side of the loss gradient (no GPU): what pins tests/lossgrad_ref.py - its forward equals tests/loss_ref.py, its
float64 gradient agrees with central finite differences of loss_ref.yolo_loss, and hand-derived answers hold -, the
condition every GPU case depends on (no kink within 1e-5), and the public surface (the C-ABI entry)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import loss_ref, lossgrad_ref
from tests.util import ANCHORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(logits, y_true, s, ignore_thresh=.5):
    an, step = loss_ref.scale_anchors(ANCHORS, s), loss_ref.GRID_STEPS[s]
    return loss_ref.yolo_loss(y_true, logits, an, step, ignore_thresh), lossgrad_ref.loss_and_grad(y_true, logits, an, step, ignore_thresh)


@pytest.fixture(scope='module')
def cases():
    return lossgrad_ref.parity_cases() + [('disjoint scale %d' % s, s, l, y) for s, (l, y) in lossgrad_ref.disjoint_case().items()]


# ----------------------------------------------------------------------------- the forward is loss_ref's
def test_forward_equals_loss_ref(cases):
    for name, s, logits, y_true in cases:
        r, (t, _) = _both(logits, y_true, s)
        for k in ('loss', 'giou', 'conf', 'cls'):
            assert abs(t[k] - r[k]) <= 1e-12 * abs(r[k]), '%s %s: %r != %r' % (name, k, t[k], r[k])
        assert t['ignore_sum'] == r['ignore_sum'], name
        assert np.array_equal(t['best_iou'] < .5, r['best_iou'] < .5) and np.allclose(t['best_iou'], r['best_iou'], rtol=0, atol=1e-12), name


# ----------------------------------------------------------------------------- finite differences
def test_gradient_agrees_with_finite_differences():
    """Central differences of loss_ref.yolo_loss (float64, step 1e-6) at every box and confidence logit of every object cell
    and at 64 random other elements, per scale of random_case(0, 2, (64, 96), 80).  Relative to the element's own value, with
    the floor the difference quotient's own rounding sets: the loss is a float64 sum of a few hundred, so a quotient over
    2e-6 carries up to ~1e-13 / 2e-6 = 5e-8 of noise whatever the element's size; 1e-6 of the largest checked gradient is
    above that floor and is what a small element is allowed instead."""
    h = 1e-6
    for s, (logits, y_true) in loss_ref.random_case(0, 2, (64, 96), 80, ANCHORS).items():
        an, step = loss_ref.scale_anchors(ANCHORS, s), loss_ref.GRID_STEPS[s]
        _, grad = lossgrad_ref.loss_and_grad(y_true, logits, an, step)
        assert grad.dtype == np.float64 and grad.shape == logits.shape
        idx = [tuple(c) + (k,) for c in np.argwhere(y_true[..., 4] != 0) for k in range(5)]
        rs = np.random.RandomState(100 + s)
        idx += [tuple(rs.randint(n) for n in logits.shape) for _ in range(64)]
        assert len(idx) >= 64 + 5
        x = logits.astype(np.float64)
        worst, top = 0.0, max(abs(grad[i]) for i in idx)
        for i in idx:
            keep = x[i]
            x[i] = keep + h
            up = loss_ref.yolo_loss(y_true, x, an, step)['loss']
            x[i] = keep - h
            dn = loss_ref.yolo_loss(y_true, x, an, step)['loss']
            x[i] = keep
            fd = (up - dn) / (2 * h)
            err = abs(fd - grad[i]) / max(abs(grad[i]), top)
            worst = max(worst, err)
            assert err <= 1e-6, 'scale %d element %s: autograd %r, finite difference %r' % (s, i, grad[i], fd)
        print('scale %d: %d elements, worst relative difference %.3e' % (s, len(idx), worst))


# ----------------------------------------------------------------------------- known answers
def _zero_case():
    shape = (1, 13, 13, 3, 25)
    return np.zeros(shape, np.float32), np.zeros(shape, np.float32)


def test_known_answer_no_labelled_box():
    """Every cell is ignored-eligible (best IoU over no box is -inf): d conf / d x4 = sigmoid(0) - 0 = 0.5, m = 1."""
    logits, y_true = _zero_case()
    _, g = lossgrad_ref.loss_and_grad(y_true, logits, loss_ref.scale_anchors(ANCHORS, 0), 32)
    assert np.all(g[..., 4] == 0.5) and np.all(g[..., :4] == 0) and np.all(g[..., 5:] == 0)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_known_answer_one_box_and_its_neighbours(dtype):
    """The box of tests/test_gpu_loss.py::_one_box: prediction == label in slot 0 of cell (6, 6).  GIoU has a kink there (its
    one-sided derivatives with respect to the size logits are -1 and +1), and the answer 0 is what BOTH tie rules give AT the
    tie - so the label is written in the dtype the reference runs in: a float32 label under a float64 prediction is 1e-9 off the
    tie and gets a one-sided derivative."""
    logits, y_true = _zero_case()
    y_true = y_true.astype(dtype)
    y_true[0, 6, 6, 0, :5] = (dtype(6.5) / dtype(13), dtype(6.5) / dtype(13), dtype(116) / dtype(416), dtype(90) / dtype(416), 1)
    y_true[0, 6, 6, 0, 5 + 3] = 1
    res, g = lossgrad_ref.loss_and_grad(y_true, logits, loss_ref.scale_anchors(ANCHORS, 0), 32, dtype=dtype)
    row = g[0, 6, 6, 0]
    assert row[4] == -0.5 and row[5 + 3] == -0.5
    assert np.all(np.delete(row[5:], 3) == 0.5)
    assert np.all(np.abs(row[:4]) <= 1e-6)                   # the GIoU gradient vanishes at giou == 1 under either tie rule
    # the horizontal neighbours of slot 0 overlap the label by 84 of 116 pixels, IoU 0.568 >= 0.5 (tests/test_loss_host.py): they
    # are neither objects nor background and drop out of the confidence term; the cell's own other slots (anchors 156x198 and
    # 373x326, IoU 0.34 and 0.09) are background like every remaining cell
    assert g[0, 6, 5, 0, 4] == 0 and g[0, 6, 7, 0, 4] == 0
    conf = g[..., 4].copy()
    conf[0, 6, 6, 0] = conf[0, 6, 5, 0] = conf[0, 6, 7, 0] = 0.5
    assert np.all(conf == 0.5)
    others = g.copy()
    others[0, 6, 6, 0] = 0
    assert np.all(others[..., :4] == 0) and np.all(others[..., 5:] == 0)


def test_known_answer_label_inside_the_prediction():
    """The 1x1 grid of tests/test_gpu_loss.py::test_known_answer_giou_term: the label lies strictly inside the prediction, so
    union = enclosing box = the prediction and giou = 0.5 / (pw * ph): d loss / d x2 = d loss / d x3 = +0.5 / (pw * ph), and
    moving the centre changes nothing."""
    logits = np.zeros((1, 1, 1, 3, 6), np.float32)
    y_true = np.zeros_like(logits)
    y_true[0, 0, 0, 0] = (0.25, 0.5, 0.5, 1.0, 1, 1)
    m = lossgrad_ref.margins(logits, y_true, 0)
    assert min(m) > 1e-5, m
    _, g = lossgrad_ref.loss_and_grad(y_true, logits, loss_ref.scale_anchors(ANCHORS, 0), 32)
    want = 0.5 / (116 * 90 / 1024)
    assert g[0, 0, 0, 0, 2] == pytest.approx(want, rel=1e-12) and g[0, 0, 0, 0, 3] == pytest.approx(want, rel=1e-12)
    assert abs(g[0, 0, 0, 0, 0]) <= 1e-12 and abs(g[0, 0, 0, 0, 1]) <= 1e-12
    assert np.all(g[0, 0, 0, 1:, :4] == 0) and np.all(g[0, 0, 0, 1:, 5:] == 0)
    assert g[0, 0, 0, 0, 4] == -0.5 and g[0, 0, 0, 0, 5] == -0.5
    assert g[0, 0, 0, 1, 4] == 0.5 and g[0, 0, 0, 2, 4] == 0.5      # IoU 0.017 and 0.004: counted as background


# ----------------------------------------------------------------------------- the GPU cases keep clear of every kink
def test_margins_of_every_gpu_case(cases):
    low = [np.inf] * 3
    for name, s, logits, y_true in cases:
        m = lossgrad_ref.margins(logits, y_true, s)
        print('%-20s margins: threshold %.2e, coordinates %.2e, intersection sides %.2e' % ((name,) + m))
        assert min(m) > 1e-5, '%s: %r' % (name, m)
        low = [min(a, b) for a, b in zip(low, m)]
    print('minima: %.2e %.2e %.2e' % tuple(low))


def test_disjoint_case_has_a_disjoint_object_cell():
    logits, y_true = lossgrad_ref.disjoint_case()[2]
    res, g = lossgrad_ref.loss_and_grad(y_true, logits, loss_ref.scale_anchors(ANCHORS, 2), 8)
    obj = y_true[..., 4] != 0
    apart = obj & ((res['raw_w'] <= 0) | (res['raw_h'] <= 0))
    assert apart.sum() >= 1
    assert np.abs(g[apart][:, :4]).max() > 0      # the enclosing-box term still pulls such a prediction towards its label


# ----------------------------------------------------------------------------- public surface
def test_c_abi_declares_and_exports_the_gradient():
    from yoloret_amd import build, runtime as rt
    header = open(os.path.join(ROOT, 'include', 'yoloret_hip.h')).read()
    assert re.search(r'\bint\s+yr_yolo_loss_grad\s*\(', header)
    assert 'yr_yolo_loss_grad' in rt.EXPORTS
    L = ctypes.CDLL(build.build())
    assert hasattr(L, 'yr_yolo_loss_grad')
    # argument errors are reported before anything is launched (no device is needed to reach them)
    g = L.yr_yolo_loss_grad
    g.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                                           ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 4
    L.yr_last_error.restype = ctypes.c_char_p
    an = (ctypes.c_float * 6)(*[1.0] * 6)
    fake = ctypes.c_void_p(4096)
    assert g(fake, fake, 1, 13, 13, 3, 20, an, 416, 416, .5, fake, 1 << 20, None, fake, None, None) == -1 and b'dfeats' in L.yr_last_error()
    assert g(None, fake, 1, 13, 13, 3, 20, an, 416, 416, .5, fake, 1 << 20, None, fake, fake, None) == -1 and b'null' in L.yr_last_error()
    assert g(fake, fake, 1, 13, 13, 9, 20, an, 416, 416, .5, fake, 1 << 20, None, fake, fake, None) == -1 and b'num_anchors' in L.yr_last_error()
    assert g(fake, fake, 1, 13, 13, 3, 20, an, 416, 416, .5, fake, 64, None, fake, fake, None) == -1 and b'workspace' in L.yr_last_error()


def test_gradient_kernel_uses_no_scratch():
    from yoloret_amd import build as b
    b.build()
    rows = [r for r in b.kernel_resources()['loss.hip'] if 'loss_main_kernel' in r[0]]
    assert len(rows) == 2, rows                   # the forward and the gradient instantiation
    assert all(scratch == 0 for _, _, scratch, _, _ in rows), rows


def test_python_surface():
    from yoloret_amd import runtime as rt
    from yoloret_amd.yolo3 import model as m
    assert callable(rt.yolo_loss_grad) and callable(m.yolo_loss_and_grad) and callable(m.yolo_loss_and_grad_from_boxes)
    assert callable(m.YoloLoss(0, ANCHORS, 3, print_loss=False).gradient)
    with pytest.raises(ValueError):
        m.YoloLoss(0, ANCHORS, 3, print_loss=False).gradient(np.zeros((1, 13, 13, 3, 25), np.float32), np.zeros((1, 13, 13, 3, 25), np.float32))
