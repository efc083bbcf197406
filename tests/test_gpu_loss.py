"""The YoloLoss forward on the device (yoloret_amd/csrc/loss.hip behind yr_yolo_loss) against tests/loss_ref.py.

Bars.  ``ignore_sum`` must be EQUAL, under a condition that is asserted on the float64 reference first: no best IoU
within 1e-5 of the threshold (float32 IoUs carry errors of a few 1e-7).  No prediction is excluded from any comparison; a
seed that violates the condition is replaced here, on the CPU (seeds 0-3 of the batch-64 case do: margins 2.8e-6 .. 9.5e-6;
seed 4 has 1.3e-5).  The three sums and their total: relative error against float64 <= 4 x (the error of the SAME reference
evaluated in float32, the precision of the reference's TensorFlow graph) + 4 float32 ulps (4 * 2^-24 = 2.4e-7); the GIoU term
on max(|ref|, 1), being a sum of 1 - giou differences.

Every case prints its figures (device value, float64 value, relative error, the float32 reference's error, the bar)
before it asserts: run with -s to see them."""
import numpy as np
import pytest
import torch

from tests import loss_ref
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

ULPS4 = 4 * 2.0 ** -24
LN2 = float(np.log(2.0))


def _model():
    from yoloret_amd.yolo3 import model
    return model


def _device_terms(dev, s, logits, y_true, num_scales=3, **kw):
    layer = _model().YoloLoss(s, ANCHORS, num_scales, print_loss=False, **kw)
    loss = layer(torch.from_numpy(y_true).to(dev), torch.from_numpy(logits).to(dev))
    torch.cuda.synchronize()
    t = layer.last_terms.cpu().numpy()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.item() == t[0]
    assert t.dtype == np.float32 and t.shape == (5,)
    return t


def _check_against_reference(got, logits, y_true, s, what, ignore_thresh=.5):
    """got: the device's five float32 words.  Prints every figure before it asserts."""
    an, step = loss_ref.scale_anchors(ANCHORS, s), loss_ref.GRID_STEPS[s]
    r64 = loss_ref.yolo_loss(y_true, logits, an, step, ignore_thresh, np.float64)
    r32 = loss_ref.yolo_loss(y_true, logits, an, step, ignore_thresh, np.float32)
    margin = loss_ref.threshold_margin(r64, ignore_thresh)
    print('%s: min |best_iou - thresh| = %.3e, ignored %d of %d' % (what, margin, r64['best_iou'].size - r64['ignore_sum'], r64['best_iou'].size))
    assert margin > 1e-5, '%s: a best IoU lies within 1e-5 of the threshold - choose another seed' % what
    t64, t32 = loss_ref.terms(r64), loss_ref.terms(r32)
    bad = []
    for i, name in enumerate(('loss', 'giou', 'conf', 'class')):
        scale = max(abs(t64[i]), 1.0) if name == 'giou' else abs(t64[i])
        if scale == 0:
            assert got[i] == 0, '%s %s: %r, the reference is exactly 0' % (what, name, got[i])
            continue
        err, err32 = abs(float(got[i]) - t64[i]) / scale, abs(t32[i] - t64[i]) / scale
        bar = 4 * err32 + ULPS4
        print('%s %-5s device %.9g  float64 %.12g  rel err %.3e  (float32 reference %.3e, bar %.3e)' % (what, name, got[i], t64[i], err, err32, bar))
        if not err <= bar:
            bad.append('%s: %.3e > %.3e' % (name, err, bar))
    print('%s ignore_sum device %d reference %d' % (what, got[4], t64[4]))
    assert got[4] == t64[4], '%s: ignore_sum %r, reference %r' % (what, got[4], t64[4])
    assert not bad, '%s: %s' % (what, '; '.join(bad))
    return r64


# ----------------------------------------------------------------------------- known answers (tests/test_loss_host.py derives them)
def _zero_case(batch):
    shape = (batch, 13, 13, 3, 25)
    return np.zeros(shape, np.float32), np.zeros(shape, np.float32)


def _one_box(y_true, image):
    y_true[image, 6, 6, 0, :5] = (6.5 / 13, 6.5 / 13, 116 / 416, 90 / 416, 1)
    y_true[image, 6, 6, 0, 5 + 3] = 1


def test_known_answer_no_labelled_box(dev):
    t = _device_terms(dev, 0, *_zero_case(1))
    assert t[1] == 0 and t[3] == 0 and t[4] == 507
    assert t[2] == pytest.approx(507 * LN2, rel=3e-7) and t[0] == pytest.approx(507 * LN2, rel=3e-7)


def test_known_answer_one_box_and_its_neighbours(dev):
    logits, y_true = _zero_case(1)
    _one_box(y_true, 0)
    t = _device_terms(dev, 0, logits, y_true)
    assert t[4] == 504
    assert t[2] == pytest.approx(505 * LN2, rel=3e-7) and t[3] == pytest.approx(20 * LN2, rel=3e-7) and abs(t[1]) <= 1e-6
    assert t[0] == pytest.approx(525 * LN2, rel=3e-7)


def test_known_answer_batch_wide_gather(dev):
    logits, y_true = _zero_case(2)
    _one_box(y_true, 1)
    t = _device_terms(dev, 0, logits, y_true)
    assert t[4] == 1008
    assert t[2] == pytest.approx(1009 * LN2 / 2, rel=3e-7) and t[3] == pytest.approx(10 * LN2, rel=3e-7) and abs(t[1]) <= 1e-6


def test_known_answer_giou_term(dev):
    """A GIoU term that is not 0.  Grid 1x1 at input 32, one class; slot 0 of scale 0 is the 116x90 anchor, so logits 0
    predict a box centred (0.5, 0.5) of size (116/32, 90/32).  The label (x 0.25, y 0.5, w 0.5, h 1) is the left half of
    the input, area 0.5, and lies inside that prediction: union = enclosing box = the prediction, so giou = iou =
    0.5 / (116*90/1024) and the term is 1 - iou.  The other two slots reach IoU 0.017 and 0.004: all three cells are ignored."""
    logits = np.zeros((1, 1, 1, 3, 6), np.float32)
    y_true = np.zeros_like(logits)
    y_true[0, 0, 0, 0] = (0.25, 0.5, 0.5, 1.0, 1, 1)
    t = _device_terms(dev, 0, logits, y_true)
    area = 116 * 90 / 1024
    iou = 0.5 / area                      # union = the prediction, which contains the label
    assert t[1] == pytest.approx(1 - iou, rel=1e-6)        # enclose == union: giou == iou
    assert t[3] == pytest.approx(LN2, rel=3e-7) and t[4] == 3
    r = loss_ref.yolo_loss(y_true, logits, loss_ref.scale_anchors(ANCHORS, 0), 32)
    assert r['giou'] == pytest.approx(1 - iou, rel=1e-12) and r['ignore_sum'] == 3


# ----------------------------------------------------------------------------- random parity
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_parity_416(dev, seed):
    case = loss_ref.random_case(seed, 3, (416, 416), 20, ANCHORS)
    for s, (logits, y_true) in case.items():
        _check_against_reference(_device_terms(dev, s, logits, y_true), logits, y_true, s, '416 seed %d scale %d' % (seed, s))


def test_parity_non_square_grid(dev):
    case = loss_ref.random_case(0, 2, (64, 96), 80, ANCHORS)
    for s, (logits, y_true) in case.items():
        assert logits.shape[1:3] == (64 // loss_ref.GRID_STEPS[s], 96 // loss_ref.GRID_STEPS[s])
        _check_against_reference(_device_terms(dev, s, logits, y_true), logits, y_true, s, '64x96 scale %d' % s)


def test_parity_batch_64_scale_2(dev):
    """519 168 predictions x 256 labelled boxes: the size the kernel is for."""
    logits, y_true = loss_ref.random_case(4, 64, (416, 416), 20, ANCHORS, scales=(2,))[2]
    assert int((y_true[..., 4] != 0).sum()) > 240
    _check_against_reference(_device_terms(dev, 2, logits, y_true), logits, y_true, 2, 'batch 64 scale 2')


def test_other_threshold_and_scale_subset(dev):
    """ignore_thresh is passed through; num_scales = 2 selects the anchors of scales 1 and 2 with steps 32 and 16 (model.py:596-605)."""
    logits, y_true = loss_ref.random_case(0, 3, (416, 416), 20, ANCHORS)[0]
    t = _device_terms(dev, 0, logits, y_true, ignore_thresh=.3)
    r = loss_ref.yolo_loss(y_true, logits, loss_ref.scale_anchors(ANCHORS, 0), 32, .3)
    assert loss_ref.threshold_margin(r, .3) > 1e-5 and t[4] == r['ignore_sum']
    assert r['ignore_sum'] < loss_ref.yolo_loss(y_true, logits, loss_ref.scale_anchors(ANCHORS, 0), 32, .5)['ignore_sum']
    t2 = _device_terms(dev, 0, logits, y_true, num_scales=2)
    r2 = loss_ref.yolo_loss(y_true, logits, loss_ref.scale_anchors(ANCHORS, 0, 2), 32, .5)
    assert loss_ref.threshold_margin(r2) > 1e-5 and t2[4] == r2['ignore_sum']
    assert t2[2] == pytest.approx(r2['conf'], rel=1e-6) and t2[1] == pytest.approx(r2['giou'], rel=1e-5)


# ----------------------------------------------------------------------------- yolo_head(calc_loss=True)
def test_yolo_head_calc_loss(dev):
    m = _model()
    feats = torch.from_numpy(np.random.RandomState(5).randn(2, 2, 3, 3, 9).astype(np.float32)).to(dev)
    an = loss_ref.scale_anchors(ANCHORS, 1)
    grid, xy, wh, conf = m.yolo_head(feats, an, (64, 96), calc_loss=True)
    xy0, wh0, conf0, _ = m.yolo_head(feats, an, (64, 96))
    torch.cuda.synchronize()
    assert torch.equal(xy, xy0) and torch.equal(wh, wh0) and torch.equal(conf, conf0)
    assert tuple(grid.shape) == (2, 3, 1, 2) and grid.dtype == torch.float32 and grid.is_cuda
    g = grid.cpu().numpy()
    assert all(tuple(g[j, i, 0]) == (i, j) for j in range(2) for i in range(3))
    _, rxy, rwh, rconf = loss_ref.yolo_head(feats.cpu().numpy(), an, (64, 96))
    assert np.allclose(xy.cpu().numpy(), rxy, rtol=2e-6, atol=0) and np.allclose(wh.cpu().numpy(), rwh, rtol=2e-6, atol=0)
    assert np.allclose(conf.cpu().numpy(), rconf, rtol=2e-6, atol=0)


# ----------------------------------------------------------------------------- reproducibility
def test_bit_reproducible_across_calls_streams_and_workspaces(dev):
    from yoloret_amd import runtime as rt
    logits, y_true = loss_ref.random_case(1, 8, (416, 416), 20, ANCHORS, scales=(2,))[2]
    f, y = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev)
    an = loss_ref.scale_anchors(ANCHORS, 2)
    first = rt.yolo_loss(f, y, an, (416, 416), .5)
    again = rt.yolo_loss(f, y, an, (416, 416), .5)
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
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            results.append(rt.yolo_loss(f, y, an, (416, 416), .5, workspace=ws))
        side.synchronize()
    torch.cuda.synchronize()
    a = first.cpu().numpy().view(np.uint32)
    assert np.isfinite(first.cpu().numpy()).all()
    assert np.array_equal(again.cpu().numpy().view(np.uint32), a)
    for r in results:
        assert np.array_equal(r.cpu().numpy().view(np.uint32), a)


# ----------------------------------------------------------------------------- the whole path
def test_loss_of_model_logits(dev):
    """yolov3_body -> logits on the device -> yolo_loss, against the reference on the SAME logits copied to the host
    (which isolates the loss from the model's own 1e-4 bar)."""
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
    assert sum(int((y[..., 4] != 0).sum()) for y in y_trues) == 7
    total, terms = m.yolo_loss(ys, [torch.from_numpy(y).to(dev) for y in y_trues], ANCHORS, 3)
    torch.cuda.synchronize()
    terms = terms.cpu().numpy()
    assert terms.shape == (3, 5) and total.dim() == 0
    ref_total = 0.0
    for s in range(3):
        r = _check_against_reference(terms[s], ys[s].cpu().numpy(), y_trues[s], s, 'model logits scale %d' % s)
        ref_total += r['loss']
    assert total.item() == pytest.approx(ref_total, rel=1e-6)


def test_print_loss_line(dev, capsys):
    logits, y_true = _zero_case(1)
    layer = _model().YoloLoss(0, ANCHORS, 3)      # print_loss defaults to True, as in the reference
    layer(y_true, torch.from_numpy(logits).to(dev))     # (a NumPy y_true is copied to the logits' device)
    out = capsys.readouterr().out.strip().split()
    assert out[0] == '0:' and len(out) == 5
    assert float(out[1]) == 0 and float(out[2]) == pytest.approx(507 * LN2, rel=3e-7) and float(out[3]) == 0 and float(out[4]) == 507


# ----------------------------------------------------------------------------- error paths
def test_error_paths(dev):
    from yoloret_amd import runtime as rt
    m = _model()
    logits, y_true = _zero_case(1)
    f, y = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev)
    an = loss_ref.scale_anchors(ANCHORS, 0)
    with pytest.raises(ValueError):
        rt.yolo_loss(torch.from_numpy(logits), y, an, (416, 416), .5)                # CPU logits
    with pytest.raises(ValueError):
        rt.yolo_loss(f, torch.from_numpy(y_true), an, (416, 416), .5)                # CPU labels
    with pytest.raises(ValueError):
        rt.yolo_loss(f, y[:, :12], an, (416, 416), .5)                               # wrong y_true shape
    with pytest.raises(ValueError):
        rt.yolo_loss(f, y.double(), an, (416, 416), .5)                              # wrong dtype
    with pytest.raises(ValueError):
        rt.yolo_loss(f, y, ANCHORS, (416, 416), .5)                                  # 9 anchors for 3 slots
    with pytest.raises(ValueError):
        rt.yolo_loss(f.reshape(1, 13, 13, 75), y.reshape(1, 13, 13, 75), an, (416, 416), .5)    # anchors not split off
    with pytest.raises(ValueError):
        rt.yolo_loss(f, y, an, (416, 416), .5, workspace=torch.empty(16, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        m.YoloLoss(0, ANCHORS, 3, print_loss=False)(y, logits)                       # NumPy logits
    # the C entry's own checks (through the binding's error type)
    with pytest.raises(rt.YoloretHipError, match='workspace'):
        ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)
        rt.check(rt.lib().yr_yolo_loss(rt._ptr(f), rt._ptr(y), 1, 13, 13, 3, 20, an.ctypes.data, 416, 416, .5, rt._ptr(ws), 64, rt._ptr(out),
                                       rt.stream_ptr(dev)))
    torch.cuda.synchronize()
