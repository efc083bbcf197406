"""torch-CPU restatement of the reference's loss, differentiated by torch.autograd: YoloLoss.call, GIOU branch
(code/yolo3/model.py:607-671), yolo_head(calc_loss=True) (:344-369) and do_giou_calculate (code/yolo3/utils.py:9-53), written
from those lines (not from the kernel) in ``dtype`` float64 - the yardstick of tests/test_gpu_lossgrad.py - or float32, whose
distance from the float64 result is the unit the bars are expressed in.  best_iou (:644-648) is computed under ``no_grad``:
ignore_mask comes from a comparison and passes no gradient.

UNPINNED by the reference, like tests/loss_ref.py (no TensorFlow where this is tested); pinned by tests/test_lossgrad_host.py:
its forward equals loss_ref.yolo_loss to 1e-12, its gradient agrees with central finite differences of loss_ref.yolo_loss, and
hand-derived answers hold.

TIES.  Every Maximum / Minimum of do_giou_calculate is written as a select (``torch.where(a >= b, a, b)``, ``torch.where(a <= b,
a, b)``, and ``tf.maximum(zero, v)`` as ``torch.where(zero >= v, zero, v)``), so torch.autograd sends the whole gradient to the
FIRST operand at a tie - TensorFlow's rule, which the kernel follows (torch.maximum / torch.minimum would split it evenly).  The
reference is therefore valid AT ties of Maximum / Minimum too: tests/test_lossgrad_edges_host.py shows that away from ties the
selects give the bits torch.maximum / torch.minimum gave, and that hand-derived answers hold at ties.  What is pinned on the
device through it (tests/test_gpu_lossgrad_edges.py): the tie rules (all 13 x 13 interval relations of label against prediction,
zero-size labels), the threshold on its last bit, box lists of up to three LDS chunks, rows of 5 to 305 floats, A from 1 to 8.
The threshold comparison of best_iou remains a kink of its own, and a float32 run can land on the other side of a Maximum /
Minimum than the float64 run when two coordinates are closer than float32 resolves: ``margins`` returns, from the float64 run,
how far a case is from each kind of kink; every GPU case of random numbers asserts that all three exceed 1e-5 before it
compares anything (the tie cases are built from dyadic numbers instead: a tie is a tie in both precisions and on the device).
Outside the contract: non-finite inputs, and logits beyond the clamp of the device's exp ([-87, 88])."""
import numpy as np
import torch

from tests import loss_ref
from tests.util import ANCHORS


def _div_no_nan(a, b):
    safe = torch.where(b != 0, b, torch.ones_like(b))
    return torch.where(b != 0, a / safe, torch.zeros_like(a))


def _max(a, b):
    """tf.maximum as a select: the gradient goes to ``a`` where a >= b, else to ``b``."""
    return torch.where(a >= b, a, b)


def _min(a, b):
    """tf.minimum as a select: the gradient goes to ``a`` where a <= b, else to ``b``."""
    return torch.where(a <= b, a, b)


def _giou_parts(b1, b2):
    """(y_min, x_min, y_max, x_max) on the last axis -> dict of the intermediate tensors of utils.py:21-53.  ``zero`` is the first
    operand of every tf.maximum(zero, v), as in the reference: v receives gradient only where v > 0."""
    zero = torch.zeros((), dtype=b1.dtype)
    b1_ymin, b1_xmin, b1_ymax, b1_xmax = b1.unbind(-1)
    b2_ymin, b2_xmin, b2_ymax, b2_xmax = b2.unbind(-1)
    b1_area = _max(zero, b1_xmax - b1_xmin) * _max(zero, b1_ymax - b1_ymin)
    b2_area = _max(zero, b2_xmax - b2_xmin) * _max(zero, b2_ymax - b2_ymin)
    raw_w = _min(b1_xmax, b2_xmax) - _max(b1_xmin, b2_xmin)
    raw_h = _min(b1_ymax, b2_ymax) - _max(b1_ymin, b2_ymin)
    inter = _max(zero, raw_w) * _max(zero, raw_h)
    union = b1_area + b2_area - inter
    iou = _div_no_nan(inter, union)
    enc_w = _max(zero, _max(b1_xmax, b2_xmax) - _min(b1_xmin, b2_xmin))
    enc_h = _max(zero, _max(b1_ymax, b2_ymax) - _min(b1_ymin, b2_ymin))
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


def margins_of(logits, y_true, anchors, grid_step, ignore_thresh=.5):
    """Distance of a case from the kinks, from float64: (a) the smallest |best_iou - thresh|, (b) the smallest
    |pred coordinate - true coordinate| over the object cells, (c) the smallest |raw intersection width or height| over the
    object cells.  (b) and (c) are +inf for a case without an object cell.  anchors: the A anchors of the call."""
    res, _ = loss_and_grad(y_true, logits, anchors, grid_step, ignore_thresh)
    obj = np.asarray(y_true)[..., 4] != 0
    a = float(np.min(np.abs(res['best_iou'] - ignore_thresh)))
    if not obj.any():
        return a, np.inf, np.inf
    b = float(np.min(np.abs(res['pred_box'][obj] - res['true_box'][obj])))
    c = float(min(np.min(np.abs(res['raw_w'][obj])), np.min(np.abs(res['raw_h'][obj]))))
    return a, b, c


def margins(logits, y_true, s, ignore_thresh=.5, anchors=ANCHORS, num_scales=3):
    """``margins_of`` for a case of scale ``s`` of the model's anchors."""
    return margins_of(logits, y_true, loss_ref.scale_anchors(anchors, s, num_scales), loss_ref.GRID_STEPS[s], ignore_thresh)


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


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_lossgrad_edges.py
# Each is (name, logits, y_true, anchors [A,2], grid_step): explicit anchors instead of a scale of the model's nine.
#
# The dyadic layout of the tie and threshold cases: input 512 x 512, grid 16 x 16 (step 32), B = 1, A = 1, C = 1, anchor (16, 16),
# every logit 0.  sigmoid(0) = 0.5 and exp(0) = 1 are exact (on the device too), so the prediction of cell (j, i) is the square of
# side 1/32 centred ((i + 1/2) / 16, (j + 1/2) / 16).  In units of TIE_UNIT = 1/256 its interval on an axis is [16 k + 4, 16 k + 12]
# for cell index k, and a label interval is given RELATIVE to that start as integers (lo, hi): every coordinate, centre, size,
# area and product below is a dyadic number with a short numerator - no rounding in float32 or float64, a tie is a tie in both.
DYADIC_ANCHORS = np.array([[16, 16]], np.float32)
DYADIC_GRID, DYADIC_STEP, TIE_UNIT = 16, 32, 1.0 / 256
# the 13 relations of an interval (the label) to another (the prediction, [0, 8]); index 0 needs lo >= -4 to stay inside [0, 1]
TIE_RELATIONS = [('equal', 0, 8),
                 ('apart, before', -6, -2), ('apart, after', 10, 14),
                 ('touching, before', -8, 0), ('touching, after', 8, 16),
                 ('overlapping the start', -4, 4), ('overlapping the end', 4, 12),
                 ('inside', 2, 6), ('inside, shared start', 0, 4), ('inside, shared end', 4, 8),
                 ('containing', -2, 10), ('containing, shared start', 0, 12), ('containing, shared end', -4, 8)]


def _dyadic_zero():
    shape = (1, DYADIC_GRID, DYADIC_GRID, 1, 6)
    return np.zeros(shape, np.float32), np.zeros(shape, np.float32)


def _dyadic_label(y_true, store, at, xr, yr, flag=1.0):
    """Writes into cell ``store`` = (j, i) of y_true the label whose x / y intervals are xr / yr = (lo, hi) in TIE_UNIT relative
    to the start of the prediction of cell ``at`` = (j, i).  Integer arithmetic up to the last division by a power of two."""
    x0, y0 = 16 * at[1] + 4, 16 * at[0] + 4
    cx2, cy2 = 2 * x0 + xr[0] + xr[1], 2 * y0 + yr[0] + yr[1]          # twice the centre
    assert 0 <= x0 + xr[0] and x0 + xr[1] <= 256 and 0 <= y0 + yr[0] and y0 + yr[1] <= 256      # the clip to [0, 1] never acts
    y_true[0, store[0], store[1], 0] = (cx2 / 512.0, cy2 / 512.0, (xr[1] - xr[0]) / 256.0, (yr[1] - yr[0]) / 256.0, flag, 1)


def tie_grid_case():
    """Cell (j, i) with j, i < 13 holds a label in relation TIE_RELATIONS[j] on y and TIE_RELATIONS[i] on x to the cell's own
    prediction: 169 object cells, 256 predictions - one full workgroup, one chunk of labelled boxes."""
    logits, y_true = _dyadic_zero()
    for j, (_, ylo, yhi) in enumerate(TIE_RELATIONS):
        for i, (_, xlo, xhi) in enumerate(TIE_RELATIONS):
            _dyadic_label(y_true, (j, i), (j, i), (xlo, xhi), (ylo, yhi))
    return 'tie grid', logits, y_true, DYADIC_ANCHORS, DYADIC_STEP


ZERO_SIZE_POINTS = [('inside', 4), ('on the start', 0), ('on the end', 8), ('before', -2), ('after', 10)]


def zero_size_case():
    """Labels of no width (row 0), no height (row 1) and neither (rows 2 and 3) with the object flag set; column i places the
    degenerate side(s) at ZERO_SIZE_POINTS[i] of the prediction - inside it, on either edge, outside on either side.  The other
    side is the interval [2, 6] (inside) in rows 0 and 1; row 3 shifts the y position by two columns against the x position."""
    logits, y_true = _dyadic_zero()
    n = len(ZERO_SIZE_POINTS)
    for i, (_, p) in enumerate(ZERO_SIZE_POINTS):
        q = ZERO_SIZE_POINTS[(i + 2) % n][1]
        _dyadic_label(y_true, (0, i), (0, i), (p, p), (2, 6))
        _dyadic_label(y_true, (1, i), (1, i), (2, 6), (p, p))
        _dyadic_label(y_true, (2, i), (2, i), (p, p), (p, p))
        _dyadic_label(y_true, (3, i), (3, i), (p, p), (q, q))
    return 'zero-size labels', logits, y_true, DYADIC_ANCHORS, DYADIC_STEP


# Hand-derived answers of five cells of the two cases above (asserted in float64 to 1e-12 on the host, to 1e-6 on the device).
_R = {name: k for k, (name, _, _) in enumerate(TIE_RELATIONS)}
# With every logit 0 in the dyadic layout: s = 1/32 is the prediction's side, d px / d x0 = 0.25 / 16, d pw / d x2 = s, m = 1, and
# loss = 1 - giou.  With g = d giou / d (y_min, x_min, y_max, x_max) of the prediction:
#     channel 0 = -(g.x_min + g.x_max) / 64, 1 = -(g.y_min + g.y_max) / 64, 2 = -(g.x_max - g.x_min) s / 2, 3 = -(g.y_max - g.y_min) s / 2
# and d giou = (u di - i du) / u^2 + (e du - u de) / e^2 (i, u, e: intersection, union, enclosing area; du = d area1 - di).
#
# equal (y: equal, x: equal): i = u = e = s^2.  Every tie goes to the prediction: per corner di = d area1 = de (each +-s), du = 0:
#     (u di) / u^2 - (u de) / e^2 = 0.  Box gradient (0, 0, 0, 0).
# touching (y: equal, x: label [p0 - s, p0]): i = 0 and raw_w = 0 passes nothing; u = e = 2 s^2, so d giou = (du - de) / (2 s^2).
#     x_min: du = -s, the enclosing start is the label's: de = 0 -> -1/(2s).   x_max: du = s, de = +s (the end is the prediction's) -> 0.
#     y_min: du = -s, the tie gives the enclosing start to the prediction: de = -2s -> +1/(2s).   y_max: du = s, de = 2s -> -1/(2s).
#     channels (16 / 64, 0, -(0 + 1/(2s)) s / 2, -(-1/(2s) - 1/(2s)) s / 2) = (0.25, 0, -0.25, 0.5).
# containing, shared start (y: equal, x: label [p0, p0 + 1.5 s]) - a tie of the ENCLOSING box's start (and of the intersection's):
#     i = s^2, u = e = 1.5 s^2, giou = 2/3.  x_min: di = -s and de = -s (both ties to the prediction), d area1 = -s, du = 0:
#     -1.5 s^3 / 2.25 s^4 + 1.5 s^3 / 2.25 s^4 = 0.   x_max: di = s (the prediction's end is the smaller), de = 0, du = 0 -> 2/(3s).
#     y_min: di = -s, de = -1.5 s, du = 0 -> -2/(3s) + 1/s = 1/(3s).   y_max: -1/(3s).
#     channels (-(2/(3s)) / 64, 0, -(2/(3s)) s / 2, -(-2/(3s)) s / 2) = (-1/3, 0, -1/3, 1/3).
#     (torch.maximum / torch.minimum halve di and de at every tied corner and give -5/18 in channel 0.)
# zero-size label on the prediction's start (zero_size_case row 2, column 1: the point (p0, p0)): i = 0, u = s^2, e = s^2 (the
#     enclosing box is the prediction, by ties at both starts), giou = 0 - 0.  d giou = (e du - u de) / e^2 = (du - de) / s^2 with
#     du = d area1 = de at every corner: (0, 0, 0, 0).
# zero-size label outside (row 2, column 3: the point (p0 - s/4, p0 - s/4)): u = s^2, e = (1.25 s)^2, both starts of the enclosing
#     box are the label's (de = 0 there), both ends the prediction's (de = +1.25 s).  x_min, y_min: du = -s -> -s e / e^2 = -1/(1.5625 s);
#     x_max, y_max: (e s - u 1.25 s) / e^2 = (1.5625 - 1.25) s^3 / (1.5625^2 s^4) = 0.128 / s.
#     channel 0 = -(0.128 - 0.64) * 32 / 64 = 0.256, channel 2 = -(0.128 + 0.64) / 2 = -0.384; y likewise.
KNOWN_TIE_ANSWERS = [('tie', (_R['equal'], _R['equal']), (0, 0, 0, 0)),
                     ('tie', (_R['equal'], _R['touching, before']), (0.25, 0, -0.25, 0.5)),
                     ('tie', (_R['equal'], _R['containing, shared start']), (-1 / 3, 0, -1 / 3, 1 / 3)),
                     ('zero', (2, 1), (0, 0, 0, 0)),
                     ('zero', (2, 3), (0.256, 0.256, -0.384, -0.384))]


def known_tie_answers():
    """[(case tuple, cell (j, i), the four box gradients)]"""
    built = {'tie': tie_grid_case(), 'zero': zero_size_case()}
    return [(built[k], cell, np.array(want, np.float64)) for k, cell, want in KNOWN_TIE_ANSWERS]


THRESHOLD_P, THRESHOLD_Q = (5, 5), (9, 9)


def threshold_case():
    """Cell P holds no object; the only label of the call is stored in cell Q and is the left half of P's prediction:
    IoU = (s^2 / 2) / s^2 = 0.5 exactly in float32 and float64 (s = 1/32).  No other prediction meets the label."""
    logits, y_true = _dyadic_zero()
    _dyadic_label(y_true, THRESHOLD_Q, THRESHOLD_P, (0, 4), (0, 8))
    return 'threshold', logits, y_true, DYADIC_ANCHORS, DYADIC_STEP


def _keep_objects(y_true, keep):
    """A copy of y_true with whole rows of object cells cleared, in raster order from the end, until ``keep`` are left."""
    y = y_true.copy()
    flat = y.reshape(-1, y.shape[-1])
    idx = np.flatnonzero(flat[:, 4] != 0)
    assert len(idx) >= keep
    flat[idx[keep:]] = 0
    return y


# name -> (batch, seed, labelled boxes to keep or None for all): lists of labelled boxes that span more than one LDS chunk of 256
# (loss_main_kernel).  random_case at grid 8 x 12 (scale 2 of input 64 x 96, 288 predictions per image, rows of 8 floats) with
# 250 draws per image: 332 / 338 / 342 boxes at B = 2 (two chunks), 663 at B = 4 (three); and B = 2 seed 0 cut down to 257 and
# to 256 boxes: one past the chunk boundary, and on it.
CHUNK_RECIPES = {
    'chunks B=2 seed 0': (2, 0, None),
    'chunks B=2 seed 1': (2, 1, None),
    'chunks B=2 seed 2': (2, 2, None),
    'chunks B=4 seed 0': (4, 0, None),
    'chunks B=2 seed 0 cut to 257': (2, 0, 257),
    'chunks B=2 seed 0 cut to 256': (2, 0, 256),
}


def chunk_case(name):
    batch, seed, keep = CHUNK_RECIPES[name]
    logits, y_true = loss_ref.random_case(seed, batch, (64, 96), 3, ANCHORS, scales=(2,), boxes_per_image=250)[2]
    if keep is not None:
        y_true = _keep_objects(y_true, keep)
    return name, logits, y_true, loss_ref.scale_anchors(ANCHORS, 2), 8


# name -> (seed, batch, input_hw, C, A, object flag of every second object cell): the row and slot edges of the gradient kernel's
# second phase.  Random logits, random_case with explicit anchors (the first A of ANCHORS), grid step 32, 2 boxes per image.  The
# last case sets the object flag to 0.5 in every second object cell (any non-zero flag is an object and multiplies its terms).
EDGE_RECIPES = {
    'row of 5 (C=0)': (0, 2, (64, 96), 0, 3, 1),
    'row of 256 (C=251)': (0, 2, (64, 96), 251, 3, 1),
    'row of 257 (C=252)': (0, 2, (64, 96), 252, 3, 1),
    'row of 305 (C=300)': (0, 2, (64, 96), 300, 3, 1),
    'A=1': (0, 2, (64, 96), 20, 1, 1),
    'A=2': (0, 2, (64, 96), 20, 2, 1),
    'A=5': (0, 2, (64, 96), 20, 5, 1),
    'A=8': (0, 2, (64, 96), 20, 8, 1),
    'total 3 (grid 1x1)': (0, 1, (32, 32), 20, 3, 1),
    'total 256 (grid 8x8, A=4)': (0, 1, (256, 256), 20, 4, 1),
    'object flag 0.5': (0, 2, (64, 96), 20, 3, 0.5),
}


def edge_case(name):
    seed, batch, hw, c, a, flag = EDGE_RECIPES[name]
    an = np.ascontiguousarray(ANCHORS[:a])
    logits, y_true = loss_ref.random_case(seed, batch, hw, c, None, scales=(0,), boxes_per_image=2, slot_anchors=an)[0]
    if flag != 1:
        flat = y_true.reshape(-1, y_true.shape[-1])
        flat[np.flatnonzero(flat[:, 4] != 0)[::2], 4] = flag
    return name, logits, y_true, an, 32
