"""torch-CPU restatement of the reference's loss, differentiated by torch.autograd: YoloLoss.call, GIOU branch
(code/yolo3/model.py:607-671), yolo_head(calc_loss=True) (:344-369) and do_giou_calculate (code/yolo3/utils.py:9-53), written
from those lines (not from the kernel) in ``dtype`` float64 - the yardstick of tests/test_gpu_lossgrad.py - or float32, whose
distance from the float64 result is the unit the bars are expressed in.  best_iou (:644-648) is computed under ``no_grad``:
ignore_mask comes from a comparison and passes no gradient.

UNPINNED by the reference, like tests/loss_ref.py (no TensorFlow where this is tested); pinned by tests/test_lossgrad_host.py:
its forward equals loss_ref.yolo_loss to 1e-12, its gradient agrees with central finite differences of loss_ref.yolo_loss, and
hand-derived answers hold.

TIES.  At a tie of a Maximum / Minimum torch.autograd splits the gradient evenly where TensorFlow sends all of it to one
operand, so this reference is valid only AWAY from ties.  ``margins`` returns, from the float64 run, how far a case is from
each kind of kink; every GPU case asserts that all three exceed 1e-5 before it compares anything."""
import numpy as np
import torch

from tests import loss_ref
from tests.util import ANCHORS


def _div_no_nan(a, b):
    safe = torch.where(b != 0, b, torch.ones_like(b))
    return torch.where(b != 0, a / safe, torch.zeros_like(a))


def _giou_parts(b1, b2):
    """(y_min, x_min, y_max, x_max) on the last axis -> dict of the intermediate tensors of utils.py:21-53."""
    zero = torch.zeros((), dtype=b1.dtype)
    b1_ymin, b1_xmin, b1_ymax, b1_xmax = b1.unbind(-1)
    b2_ymin, b2_xmin, b2_ymax, b2_xmax = b2.unbind(-1)
    b1_area = torch.maximum(zero, b1_xmax - b1_xmin) * torch.maximum(zero, b1_ymax - b1_ymin)
    b2_area = torch.maximum(zero, b2_xmax - b2_xmin) * torch.maximum(zero, b2_ymax - b2_ymin)
    raw_w = torch.minimum(b1_xmax, b2_xmax) - torch.maximum(b1_xmin, b2_xmin)
    raw_h = torch.minimum(b1_ymax, b2_ymax) - torch.maximum(b1_ymin, b2_ymin)
    inter = torch.maximum(zero, raw_w) * torch.maximum(zero, raw_h)
    union = b1_area + b2_area - inter
    iou = _div_no_nan(inter, union)
    enc_w = torch.maximum(zero, torch.maximum(b1_xmax, b2_xmax) - torch.minimum(b1_xmin, b2_xmin))
    enc_h = torch.maximum(zero, torch.maximum(b1_ymax, b2_ymax) - torch.minimum(b1_ymin, b2_ymin))
    enclose = enc_w * enc_h
    return {'iou': iou, 'giou': iou - _div_no_nan(enclose - union, enclose), 'raw_w': raw_w, 'raw_h': raw_h}


def _sce(labels, logits):
    """tf.nn.sigmoid_cross_entropy_with_logits, in TensorFlow's own form: both max(x, 0) and -|x| are selects on x >= 0, so that
    the derivative at x == 0 is sigmoid(0) - z (torch's abs has derivative 0 there, which would give 1 - z)."""
    cond = logits >= 0
    relu_logits = torch.where(cond, logits, torch.zeros_like(logits))
    neg_abs_logits = torch.where(cond, -logits, logits)
    return (relu_logits - logits * labels) + torch.log1p(torch.exp(neg_abs_logits))


def _corners(xy, wh):
    return torch.cat([(xy - wh / 2.).flip(-1), (xy + wh / 2.).flip(-1)], -1)      # :631-633


def _forward(y_true, out, anchors, grid_step, ignore_thresh, chunk=16):
    """y_true, out: torch tensors of one dtype, [B,gh,gw,A,5+C] -> dict of 0-d tensors and the tensors ``margins`` reads."""
    dtype = out.dtype
    mf = float(out.shape[0])
    gh, gw = out.shape[1:3]
    anchors = torch.as_tensor(np.asarray(anchors, np.float64), dtype=dtype).reshape(1, 1, 1, -1, 2)
    object_mask = y_true[..., 4:5]
    grid = torch.stack(torch.meshgrid(torch.arange(gh, dtype=dtype), torch.arange(gw, dtype=dtype), indexing='ij')[::-1], -1)[:, :, None, :]
    pred_xy = (torch.sigmoid(out[..., :2]) + grid) / torch.tensor([gw, gh], dtype=dtype)        # :363-364
    pred_wh = torch.exp(out[..., 2:4]) * anchors / torch.tensor([gw * grid_step, gh * grid_step], dtype=dtype)   # :365-366, :628
    pred_box = _corners(pred_xy, pred_wh)
    true_box = torch.clamp(_corners(y_true[..., :2], y_true[..., 2:4]), 0, 1)                   # :640
    with torch.no_grad():                                                                       # :643-649
        listed = true_box[object_mask[..., 0] != 0]
        best_iou = torch.full(pred_box.shape[:-1], -np.inf, dtype=dtype)
        for k0 in range(0, listed.shape[0], chunk):
            iou = _giou_parts(pred_box.detach()[..., None, :], listed[k0:k0 + chunk])['iou']
            best_iou = torch.maximum(best_iou, iou.max(-1).values)
        ignore_mask = (best_iou < torch.tensor(ignore_thresh, dtype=dtype)).to(dtype)[..., None]
    ce = _sce(object_mask, out[..., 4:5])
    conf = object_mask * ce + (1 - object_mask) * ce * ignore_mask                              # :653-657
    cls = object_mask * _sce(y_true[..., 5:], out[..., 5:])                                     # :658-659
    parts = _giou_parts(pred_box, true_box)
    gl = object_mask * (1 - parts['giou'][..., None])                                           # :666-667
    res = {'giou': gl.sum() / mf, 'conf': conf.sum() / mf, 'cls': cls.sum() / mf, 'ignore_sum': float(ignore_mask.sum()),
           'best_iou': best_iou, 'pred_box': pred_box.detach(), 'true_box': true_box, 'raw_w': parts['raw_w'].detach(),
           'raw_h': parts['raw_h'].detach(), 'ignore_mask': ignore_mask[..., 0]}
    res['loss'] = res['giou'] + res['conf'] + res['cls']
    return res


def loss_and_grad(y_true, logits, anchors, grid_step, ignore_thresh=.5, dtype=np.float64):
    """One scale.  -> (res, grad): res as loss_ref.yolo_loss returns it (floats, best_iou as an array, plus the arrays
    pred_box, true_box, raw_w, raw_h, ignore_mask), grad = d res['loss'] / d logits as an array of ``dtype``."""
    tdt = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    x = torch.tensor(np.asarray(logits), dtype=tdt, requires_grad=True)
    y = torch.tensor(np.asarray(y_true), dtype=tdt)
    res = _forward(y, x, anchors, grid_step, ignore_thresh)
    res['loss'].backward()
    out = {k: (float(v.detach()) if v.dim() == 0 else v.numpy()) if isinstance(v, torch.Tensor) else v for k, v in res.items()}
    return out, x.grad.numpy()


def margins(logits, y_true, s, ignore_thresh=.5, anchors=ANCHORS, num_scales=3):
    """Distance of a case of scale ``s`` from the kinks, from float64: (a) the smallest |best_iou - thresh|, (b) the smallest
    |pred coordinate - true coordinate| over the object cells, (c) the smallest |raw intersection width or height| over the
    object cells.  (b) and (c) are +inf for a case without an object cell."""
    res, _ = loss_and_grad(y_true, logits, loss_ref.scale_anchors(anchors, s, num_scales), loss_ref.GRID_STEPS[s], ignore_thresh)
    obj = np.asarray(y_true)[..., 4] != 0
    a = float(np.min(np.abs(res['best_iou'] - ignore_thresh)))
    if not obj.any():
        return a, np.inf, np.inf
    b = float(np.min(np.abs(res['pred_box'][obj] - res['true_box'][obj])))
    c = float(min(np.min(np.abs(res['raw_w'][obj])), np.min(np.abs(res['raw_h'][obj]))))
    return a, b, c


# ----------------------------------------------------------------------------- the cases of the GPU tests, chosen on the CPU
def parity_cases():
    """[(name, scale, logits, y_true)]: the random parity cases of tests/test_gpu_lossgrad.py (recipes of loss_ref.random_case)."""
    cases = []
    for seed in (0, 1, 2):
        for s, (logits, y_true) in loss_ref.random_case(seed, 3, (416, 416), 20, ANCHORS).items():
            cases.append(('416 seed %d scale %d' % (seed, s), s, logits, y_true))
    for s, (logits, y_true) in loss_ref.random_case(0, 2, (64, 96), 80, ANCHORS).items():      # grids 2x3 .. 8x12, rows of 85 floats
        cases.append(('64x96 scale %d' % s, s, logits, y_true))
    logits, y_true = batch8_case()
    cases.append(('batch 8 scale 2', 2, logits, y_true))
    return cases


def batch8_case():
    return loss_ref.random_case(1, 8, (416, 416), 20, ANCHORS, scales=(2,))[2]


def disjoint_case():
    """{scale: (logits, y_true)}: random_case(3, 2, (64, 96), 3) with logit channels 2 and 3 of every object cell at -3.0, which
    shrinks the predictions of the object cells until (at scale 2) one no longer meets its label."""
    case = loss_ref.random_case(3, 2, (64, 96), 3, ANCHORS)
    for s, (logits, y_true) in case.items():
        logits[..., 2:4][y_true[..., 4] != 0] = -3.0
    return case


def group_errors(got, ref):
    """max |got - ref| / max |ref| per channel group -> {'box': , 'conf': , 'class': } (a group whose reference is all zero: the
    largest |got|, which must then be 0)."""
    out = {}
    for name, sl in (('box', slice(0, 4)), ('conf', slice(4, 5)), ('class', slice(5, None))):
        r = np.asarray(ref, np.float64)[..., sl]
        g = np.asarray(got, np.float64)[..., sl]
        if r.size == 0:
            continue
        scale = np.max(np.abs(r))
        out[name] = float(np.max(np.abs(g - r)) / scale) if scale > 0 else float(np.max(np.abs(g)))
    return out
