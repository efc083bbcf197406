"""The YoloLoss gradient on the device (loss_main_kernel<true> of yoloret_amd/csrc/loss.hip behind yr_yolo_loss_grad) against
tests/lossgrad_ref.py (torch-CPU float64, torch.autograd).

Conditions, asserted on the float64 reference BEFORE anything is compared (torch splits a tie of Maximum / Minimum evenly,
TensorFlow - whose rule the kernel follows - does not, so the reference is valid only away from ties): the smallest
|best_iou - thresh|, the smallest |pred coordinate - true coordinate| over the object cells and the smallest |raw
intersection side| over the object cells all exceed 1e-5.  No element is excluded from any comparison.

Bar, per channel group (box 0-3, confidence 4, class 5..), the rule of tests/test_gpu_loss.py:
    max |device - ref64| / max |ref64|  <=  4 x (the same quantity of the reference run in float32) + 4 * 2^-24.
Elements that are structurally zero - box and class channels where the object flag is 0, confidence where a cell is ignored and
not an object - must be exactly 0.  Every direct call of the C entry runs between the guards of tests/fence.py with dfeats
pre-filled with NaN.  Every case prints its figures before it asserts: run with -s to see them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fence, loss_ref, lossgrad_ref
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

ULPS4 = 4 * 2.0 ** -24


def _model():
    from yoloret_amd.yolo3 import model
    return model


def _rt():
    from yoloret_amd import runtime
    return runtime


def _fenced_grad(dev, s, logits, y_true, ignore_thresh=.5, upstream=None, num_scales=3):
    """yr_yolo_loss_grad through tests/fence.run -> (out5 [5], dfeats) as arrays, and the device tensors (f, y)."""
    rt = _rt()
    f, y = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev)
    b, gh, gw, a, ch = f.shape
    an = np.ascontiguousarray(loss_ref.scale_anchors(ANCHORS, s, num_scales))
    step = loss_ref.GRID_STEPS[s]
    need = rt.yolo_loss_workspace_bytes(b, gh, gw, a)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    out5 = torch.full((5,), float('nan'), dtype=torch.float32, device=dev)
    dfeats = torch.full(f.shape, float('nan'), dtype=torch.float32, device=dev)
    up = None if upstream is None else torch.full((1,), upstream, dtype=torch.float32, device=dev)

    def call(moved):
        p = lambda t: rt._ptr(moved(t))
        rt.check(rt.lib().yr_yolo_loss_grad(p(f), p(y), b, gh, gw, a, ch - 5, an.ctypes.data_as(ctypes.c_void_p), gh * step, gw * step,
                                            ignore_thresh, p(ws), need, rt._ptr(up), p(out5), p(dfeats), rt.stream_ptr(dev)))
    with torch.cuda.device(dev):
        fence.run(call, writes=[dfeats, out5], reads=[f, y], scratch=[ws], batch=b)
    torch.cuda.synchronize()
    return out5.cpu().numpy(), dfeats.cpu().numpy(), f, y, an


def _check_against_reference(got, logits, y_true, s, what, ignore_thresh=.5):
    """got: the device's dfeats.  Asserts the margins, prints every figure, then asserts the bar and the exact zeros."""
    an, step = loss_ref.scale_anchors(ANCHORS, s), loss_ref.GRID_STEPS[s]
    m = lossgrad_ref.margins(logits, y_true, s, ignore_thresh)
    print('%s: margins threshold %.3e, coordinates %.3e, intersection sides %.3e' % ((what,) + m))
    assert min(m) > 1e-5, '%s: a kink lies within 1e-5 (%r) - choose another case' % (what, m)
    r64, g64 = lossgrad_ref.loss_and_grad(y_true, logits, an, step, ignore_thresh, np.float64)
    _, g32 = lossgrad_ref.loss_and_grad(y_true, logits, an, step, ignore_thresh, np.float32)
    assert got.shape == g64.shape and got.dtype == np.float32 and np.isfinite(got).all(), '%s: shape / dtype / a NaN survived' % what
    dev_err, ref_err = lossgrad_ref.group_errors(got, g64), lossgrad_ref.group_errors(g32, g64)
    bad = []
    for name in dev_err:
        bar = 4 * ref_err[name] + ULPS4
        print('%s %-5s device %.3e  (float32 reference %.3e, bar %.3e)' % (what, name, dev_err[name], ref_err[name], bar))
        if not dev_err[name] <= bar:
            bad.append('%s: %.3e > %.3e' % (name, dev_err[name], bar))
    om = y_true[..., 4]
    assert np.all(got[om == 0][:, :4] == 0) and np.all(got[om == 0][:, 5:] == 0), '%s: box / class gradient in a cell without an object' % what
    assert np.all(got[(om == 0) & (r64['ignore_mask'] == 0)][:, 4] == 0), '%s: confidence gradient in an ignored cell' % what
    assert not bad, '%s: %s' % (what, '; '.join(bad))
    return r64


def _forward_bits(f, y, an, hw, ignore_thresh=.5):
    t = _rt().yolo_loss(f, y, an, hw, ignore_thresh)
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------- known answers (tests/test_lossgrad_host.py derives them)
def _zero_case(batch=1):
    shape = (batch, 13, 13, 3, 25)
    return np.zeros(shape, np.float32), np.zeros(shape, np.float32)


def test_known_answer_no_labelled_box(dev):
    logits, y_true = _zero_case()
    out5, g, f, y, an = _fenced_grad(dev, 0, logits, y_true)
    assert np.all(g[..., 4] == 0.5)
    assert np.all(g[..., :4] == 0) and np.all(g[..., 5:] == 0)
    assert np.array_equal(out5.view(np.uint32), _forward_bits(f, y, an, (416, 416)))


def test_known_answer_one_box_and_its_neighbours(dev):
    """tests/test_gpu_loss.py::_one_box: prediction == label bit for bit in float32, an exact tie on every Maximum / Minimum."""
    logits, y_true = _zero_case()
    y_true[0, 6, 6, 0, :5] = (6.5 / 13, 6.5 / 13, 116 / 416, 90 / 416, 1)
    y_true[0, 6, 6, 0, 5 + 3] = 1
    out5, g, f, y, an = _fenced_grad(dev, 0, logits, y_true)
    row = g[0, 6, 6, 0]
    print('one box: object row', row)
    assert row[4] == -0.5 and row[5 + 3] == -0.5 and np.all(np.delete(row[5:], 3) == 0.5)
    assert np.all(np.abs(row[:4]) <= 1e-6)
    # ignored (IoU 0.568 >= 0.5 with the label, tests/test_loss_host.py): slot 0 of the two horizontal neighbours; the cell's own
    # other slots reach 0.34 and 0.09 and are background like every remaining cell
    assert g[0, 6, 5, 0, 4] == 0 and g[0, 6, 7, 0, 4] == 0
    conf = g[..., 4].copy()
    conf[0, 6, 6, 0] = conf[0, 6, 5, 0] = conf[0, 6, 7, 0] = 0.5
    assert np.all(conf == 0.5)
    others = g.copy()
    others[0, 6, 6, 0] = 0
    assert np.all(others[..., :4] == 0) and np.all(others[..., 5:] == 0)
    assert np.array_equal(out5.view(np.uint32), _forward_bits(f, y, an, (416, 416)))


def test_known_answer_label_inside_the_prediction(dev):
    """The 1x1 grid of tests/test_gpu_loss.py::test_known_answer_giou_term: giou = 0.5 / (pw * ph)."""
    logits = np.zeros((1, 1, 1, 3, 6), np.float32)
    y_true = np.zeros_like(logits)
    y_true[0, 0, 0, 0] = (0.25, 0.5, 0.5, 1.0, 1, 1)
    assert min(lossgrad_ref.margins(logits, y_true, 0)) > 1e-5
    out5, g, f, y, an = _fenced_grad(dev, 0, logits, y_true)
    want = 0.5 / (116 * 90 / 1024)
    print('1x1 grid: slot 0', g[0, 0, 0, 0], 'expected size gradients', want)
    assert g[0, 0, 0, 0, 2] == pytest.approx(want, rel=1e-6) and g[0, 0, 0, 0, 3] == pytest.approx(want, rel=1e-6)
    assert abs(g[0, 0, 0, 0, 0]) <= 1e-7 and abs(g[0, 0, 0, 0, 1]) <= 1e-7
    assert np.all(g[0, 0, 0, 1:, :4] == 0) and np.all(g[0, 0, 0, 1:, 5:] == 0)
    assert g[0, 0, 0, 0, 4] == -0.5 and g[0, 0, 0, 0, 5] == -0.5 and g[0, 0, 0, 1, 4] == 0.5 and g[0, 0, 0, 2, 4] == 0.5


# ----------------------------------------------------------------------------- random parity
def _parity(dev, case, what):
    for s, (logits, y_true) in case.items():
        out5, g, f, y, an = _fenced_grad(dev, s, logits, y_true)
        name = '%s scale %d' % (what, s)
        _check_against_reference(g, logits, y_true, s, name)
        hw = (logits.shape[1] * loss_ref.GRID_STEPS[s], logits.shape[2] * loss_ref.GRID_STEPS[s])
        assert np.array_equal(out5.view(np.uint32), _forward_bits(f, y, an, hw)), '%s: out5 differs from yr_yolo_loss' % name


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_parity_416(dev, seed):
    """13^2 x 3 x 3 = 1521 predictions: the last workgroup is partial; 52^2 x 27: many workgroups."""
    _parity(dev, loss_ref.random_case(seed, 3, (416, 416), 20, ANCHORS), '416 seed %d' % seed)


def test_parity_non_square_grid_and_wide_rows(dev):
    """Grids 2x3 .. 8x12 with rows of 85 floats: 256 is no multiple of the row, a workgroup holds fewer rows than lanes."""
    _parity(dev, loss_ref.random_case(0, 2, (64, 96), 80, ANCHORS), '64x96')


def test_parity_batch_8_scale_2(dev):
    logits, y_true = lossgrad_ref.batch8_case()
    _parity(dev, {2: (logits, y_true)}, 'batch 8')


def test_parity_disjoint_prediction(dev):
    """An object cell whose prediction does not meet its label: the intersection passes no gradient, the enclosing box does."""
    case = lossgrad_ref.disjoint_case()
    logits, y_true = case[2]
    res, _ = lossgrad_ref.loss_and_grad(y_true, logits, loss_ref.scale_anchors(ANCHORS, 2), 8)
    apart = (y_true[..., 4] != 0) & ((res['raw_w'] <= 0) | (res['raw_h'] <= 0))
    assert apart.sum() >= 1
    _parity(dev, case, 'disjoint')


# ----------------------------------------------------------------------------- reproducibility and upstream
def test_bit_reproducible_across_calls_streams_and_workspaces(dev):
    rt = _rt()
    logits, y_true = lossgrad_ref.batch8_case()
    f, y = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev)
    an = loss_ref.scale_anchors(ANCHORS, 2)
    first = rt.yolo_loss_grad(f, y, an, (416, 416), .5)
    again = rt.yolo_loss_grad(f, y, an, (416, 416), .5)
    need = rt.yolo_loss_workspace_bytes(8, 52, 52, 3)
    results = []
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    for pattern in (0xFF, 0x7B, 'random'):      # NaN bits (and a box count of 2^32 - 1), large finite values, random bytes
        ws = torch.empty((need + 64,), dtype=torch.uint8, device=dev)
        if pattern == 'random':
            ws.random_(0, 256)
        else:
            ws.fill_(pattern)
        out = torch.full(f.shape, float('nan'), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            results.append(rt.yolo_loss_grad(f, y, an, (416, 416), .5, workspace=ws, out=out))
        side.synchronize()
        assert results[-1][1] is out
    torch.cuda.synchronize()
    bits = lambda r: (r[0].cpu().numpy().view(np.uint32), r[1].cpu().numpy().view(np.uint32))
    t0, g0 = bits(first)
    assert np.isfinite(first[1].cpu().numpy()).all()
    assert np.array_equal(t0, _forward_bits(f, y, an, (416, 416)))
    for r in [again] + results:
        t, g = bits(r)
        assert np.array_equal(t, t0) and np.array_equal(g, g0)


def test_upstream_scales_exactly(dev):
    logits, y_true = loss_ref.random_case(0, 3, (416, 416), 20, ANCHORS)[1]
    _, g1, _, _, _ = _fenced_grad(dev, 1, logits, y_true)
    out5, gq, f, y, an = _fenced_grad(dev, 1, logits, y_true, upstream=0.25)
    assert np.array_equal(np.float32(0.25) * g1, gq)
    assert np.array_equal(out5.view(np.uint32), _forward_bits(f, y, an, (416, 416)))                  # the loss itself is not scaled


# ----------------------------------------------------------------------------- YoloLoss.gradient and torch.autograd
def test_layer_gradient_and_autograd(dev):
    m = _model()
    logits, y_true = loss_ref.random_case(2, 3, (416, 416), 20, ANCHORS)[0]
    y = torch.from_numpy(y_true).to(dev)
    layer = m.YoloLoss(0, ANCHORS, 3, print_loss=False)
    x = torch.from_numpy(logits).to(dev)
    plain = layer(y, x)
    assert plain.grad_fn is None and not plain.requires_grad
    plain_bits = layer.last_terms.cpu().numpy().view(np.uint32)
    g = layer.gradient(y, x)
    assert tuple(g.shape) == tuple(x.shape) and np.array_equal(layer.last_terms.cpu().numpy().view(np.uint32), plain_bits)
    g4 = layer.gradient(y, x.reshape(3, 13, 13, 75))                     # the 4-D form a serialised plan emits
    assert tuple(g4.shape) == (3, 13, 13, 75) and torch.equal(g4.reshape(x.shape), g)
    gq = layer.gradient(y, x, upstream=0.25)
    # loss.backward()
    xg = x.clone().requires_grad_(True)
    loss = layer(y, xg)
    assert loss.grad_fn is not None and loss.dim() == 0 and loss.dtype == torch.float32
    assert np.array_equal(layer.last_terms.cpu().numpy().view(np.uint32), plain_bits) and loss.item() == plain.item()
    loss.backward()
    assert xg.grad is not None and torch.equal(xg.grad, g)
    # an explicit cotangent, through the 4-D form
    x4 = x.reshape(3, 13, 13, 75).clone().requires_grad_(True)
    loss = layer(y, x4)
    torch.autograd.backward(loss, torch.tensor(0.25, device=dev))
    assert tuple(x4.grad.shape) == (3, 13, 13, 75) and torch.equal(x4.grad.reshape(x.shape), gq)
    with torch.no_grad():
        assert layer(y, xg).grad_fn is None
    torch.cuda.synchronize()
    _check_against_reference(g.cpu().numpy(), logits, y_true, 0, 'YoloLoss.gradient')


def test_gradient_never_prints(dev, capsys):
    logits, y_true = _zero_case()
    layer = _model().YoloLoss(0, ANCHORS, 3)      # print_loss defaults to True
    layer.gradient(y_true, torch.from_numpy(logits).to(dev))
    torch.cuda.synchronize()
    assert capsys.readouterr().out == ''


# ----------------------------------------------------------------------------- the whole path
def test_loss_and_grad_of_model_logits(dev):
    """yolov3_body -> logits on the device -> yolo_loss_and_grad, against the reference on the SAME logits copied to the host;
    the labels of tests/test_gpu_loss.py::test_loss_of_model_logits."""
    from oracle import model as om, params
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3.utils import preprocess_true_boxes
    m = _model()
    hw, b, c = (96, 96), 2, 20
    net = m.yolov3_body(L.Input(shape=[hw[0], hw[1], 3]), 'mobilenetv2x75', 3, num_classes=c)
    P = params.ParamStore(1234)
    x = params.synthetic_images(b, hw[0], hw[1])
    om.yolov3_body(P, x, 'mobilenetv2x75', 3, c)      # (draws the synthetic weights)
    net.set_weights(P.values)
    ys = net(torch.from_numpy(x).to(dev))
    labels = [np.array([[10, 20, 70, 80, 3], [40, 8, 64, 60, 7], [50, 50, 62, 70, 0], [0, 0, 0, 0, 0]], np.float32),
              np.array([[2, 30, 90, 66, 11], [60, 60, 76, 90, 19], [5, 5, 15, 18, 1], [70, 10, 92, 34, 5]], np.float32)]
    per_image = [preprocess_true_boxes(t, hw, ANCHORS, c, 3) for t in labels]
    y_trues = [np.stack([per_image[i][s] for i in range(b)]) for s in range(3)]
    total0, terms0 = m.yolo_loss(ys, [torch.from_numpy(y).to(dev) for y in y_trues], ANCHORS, 3)
    total, terms, grads = m.yolo_loss_and_grad(ys, [torch.from_numpy(y).to(dev) for y in y_trues], ANCHORS, 3)
    total2, terms2, grads2 = m.yolo_loss_and_grad_from_boxes(ys, np.stack(labels), ANCHORS, c, 3)
    torch.cuda.synchronize()
    assert torch.equal(terms, terms0) and torch.equal(total, total0)
    assert torch.equal(terms2, terms) and torch.equal(total2, total)
    assert len(grads) == len(grads2) == 3
    for s in range(3):
        assert grads[s].shape == ys[s].shape
        assert np.array_equal(grads2[s].cpu().numpy().view(np.uint32), grads[s].cpu().numpy().view(np.uint32))
        logits = ys[s].cpu().numpy().reshape(y_trues[s].shape)
        _check_against_reference(grads[s].cpu().numpy().reshape(y_trues[s].shape), logits, y_trues[s], s, 'model logits scale %d' % s)


# ----------------------------------------------------------------------------- error paths
def test_error_paths(dev):
    rt = _rt()
    logits, y_true = _zero_case()
    f, y = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev)
    an = loss_ref.scale_anchors(ANCHORS, 0)
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(torch.from_numpy(logits), y, an, (416, 416), .5)                # CPU logits
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(f, torch.from_numpy(y_true), an, (416, 416), .5)                # CPU labels
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(f, y, an, (416, 416), .5, out=torch.empty((1, 13, 13, 3, 24), dtype=torch.float32, device=dev))    # shape
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(f, y, an, (416, 416), .5, out=torch.empty(f.shape, dtype=torch.float64, device=dev))               # dtype
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(f, y, an, (416, 416), .5, out=torch.empty(f.shape, dtype=torch.float32))                           # device
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(f, y, an, (416, 416), .5, out=torch.empty((1, 13, 13, 3, 50), dtype=torch.float32, device=dev)[..., ::2])   # strided
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(f, y, an, (416, 416), .5, upstream=torch.ones(2, dtype=torch.float32, device=dev))                 # two elements
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(f, y, an, (416, 416), .5, upstream=torch.ones(1, dtype=torch.float32))                             # CPU upstream
    with pytest.raises(ValueError):
        rt.yolo_loss_grad(f, y, an, (416, 416), .5, workspace=torch.empty(16, dtype=torch.uint8, device=dev))
    # the C entry's own checks (through the binding's error type)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    out5 = torch.empty(5, dtype=torch.float32, device=dev)
    d = torch.empty_like(f)
    args = lambda ws_bytes, dptr: (rt._ptr(f), rt._ptr(y), 1, 13, 13, 3, 20, an.ctypes.data, 416, 416, .5, rt._ptr(ws), ws_bytes, None,
                                   rt._ptr(out5), dptr, rt.stream_ptr(dev))
    with pytest.raises(rt.YoloretHipError, match='workspace'):
        rt.check(rt.lib().yr_yolo_loss_grad(*args(64, rt._ptr(d))))
    with pytest.raises(rt.YoloretHipError, match='dfeats'):
        rt.check(rt.lib().yr_yolo_loss_grad(*args(1 << 16, None)))
    torch.cuda.synchronize()
