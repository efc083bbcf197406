"""NumPy restatement of the reference's loss forward: YoloLoss.call, GIOU branch (code/yolo3/model.py:607-671),
yolo_head(calc_loss=True) (:344-369) and do_giou_calculate (code/yolo3/utils.py:9-53), written from those lines.

``dtype=np.float64`` is the yardstick the HIP kernels are measured against; ``dtype=np.float32`` runs the SAME code with
every intermediate in float32 - the precision the reference's float32 TensorFlow graph carries -, and its distance from
the float64 result is the unit the tests' bars are expressed in.

TensorFlow is not available where this project is tested, so like the rest of the oracle this file is UNPINNED by the
reference itself: it is pinned by the hand-derived known answers of tests/test_loss_host.py (the empty-label case, the
single box with its two ignored neighbours, the batch-wide gather, the GIoU of disjoint squares).

Also here: the recipe of the random parity cases (``random_case``), so that the condition the GPU tests depend on - no
best IoU within 1e-5 of the threshold - can be checked for a seed without a GPU."""
import numpy as np

ANCHOR_MASKS = [[6, 7, 8], [3, 4, 5], [0, 1, 2]]
GRID_STEPS = [32, 16, 8]


def scale_anchors(anchors, idx, num_scales=3):
    """The anchors YoloLoss(idx, anchors, num_scales) works with (model.py:596-605)."""
    return np.asarray(anchors, np.float32).reshape(-1, 2)[ANCHOR_MASKS[-num_scales:][idx]]


def _div_no_nan(a, b):
    a, b = np.broadcast_arrays(a, b)
    out = np.zeros(a.shape, a.dtype)
    np.divide(a, b, out=out, where=b != 0)
    return out


def giou(b1, b2, mode='giou'):
    """(y_min, x_min, y_max, x_max) boxes on the last axis, in the dtype of b1 (utils.py:21-53)."""
    zero = b1.dtype.type(0)
    w1 = np.maximum(zero, b1[..., 3] - b1[..., 1])
    h1 = np.maximum(zero, b1[..., 2] - b1[..., 0])
    w2 = np.maximum(zero, b2[..., 3] - b2[..., 1])
    h2 = np.maximum(zero, b2[..., 2] - b2[..., 0])
    area1, area2 = w1 * h1, w2 * h2
    iw = np.maximum(zero, np.minimum(b1[..., 3], b2[..., 3]) - np.maximum(b1[..., 1], b2[..., 1]))
    ih = np.maximum(zero, np.minimum(b1[..., 2], b2[..., 2]) - np.maximum(b1[..., 0], b2[..., 0]))
    inter = iw * ih
    union = area1 + area2 - inter
    iou = _div_no_nan(inter, union)
    if mode == 'iou':
        return iou
    ew = np.maximum(zero, np.maximum(b1[..., 3], b2[..., 3]) - np.minimum(b1[..., 1], b2[..., 1]))
    eh = np.maximum(zero, np.maximum(b1[..., 2], b2[..., 2]) - np.minimum(b1[..., 0], b2[..., 0]))
    enclose = ew * eh
    return iou - _div_no_nan(enclose - union, enclose)


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def yolo_head(feats, anchors, input_hw, dtype=np.float64):
    """yolo_head(calc_loss=True): -> grid [gh,gw,1,2] (x, y), box_xy, box_wh [B,gh,gw,A,2], box_confidence [B,gh,gw,A,1]."""
    feats = np.asarray(feats).astype(dtype)
    anchors = np.asarray(anchors).astype(dtype).reshape(1, 1, 1, -1, 2)
    gh, gw = feats.shape[1:3]
    grid = np.empty((gh, gw, 1, 2), dtype)
    grid[..., 0] = np.arange(gw).reshape(1, gw, 1)
    grid[..., 1] = np.arange(gh).reshape(gh, 1, 1)
    box_xy = (_sigmoid(feats[..., :2]) + grid) / np.array([gw, gh], dtype)
    box_wh = np.exp(feats[..., 2:4]) * anchors / np.array([input_hw[1], input_hw[0]], dtype)
    return grid, box_xy, box_wh, _sigmoid(feats[..., 4:5])


def _sce(labels, logits):
    """tf.nn.sigmoid_cross_entropy_with_logits."""
    zero = logits.dtype.type(0)
    return (np.maximum(logits, zero) - logits * labels) + np.log1p(np.exp(-np.abs(logits)))


def _corners(xy, wh):
    two = xy.dtype.type(2)
    return np.concatenate([(xy - wh / two)[..., ::-1], (xy + wh / two)[..., ::-1]], -1)


def yolo_loss(y_true, yolo_output, anchors, grid_step, ignore_thresh=.5, dtype=np.float64, chunk=16):
    """One scale.  anchors: the A anchors of this scale.  -> dict with loss, giou, conf, cls (each divided by B),
    ignore_sum, and best_iou [B,gh,gw,A] (-inf everywhere when the call holds no labelled box)."""
    y_true = np.asarray(y_true).astype(dtype)
    out = np.asarray(yolo_output).astype(dtype)
    m = dtype(out.shape[0])
    object_mask = y_true[..., 4:5]
    input_hw = (out.shape[1] * grid_step, out.shape[2] * grid_step)
    _, pred_xy, pred_wh, _ = yolo_head(out, anchors, input_hw, dtype)
    pred_box = _corners(pred_xy, pred_wh)
    true_box = np.clip(_corners(y_true[..., :2], y_true[..., 2:4]), dtype(0), dtype(1))
    listed = true_box[object_mask[..., 0] != 0]                 # over the WHOLE batch (model.py:643)
    best_iou = np.full(pred_box.shape[:-1], -np.inf, dtype)
    for k0 in range(0, listed.shape[0], chunk):                 # (chunks only bound the memory of the all-pairs table)
        iou = giou(pred_box[..., None, :], listed[k0:k0 + chunk], mode='iou')
        best_iou = np.maximum(best_iou, iou.max(-1))
    ignore_mask = (best_iou < dtype(ignore_thresh)).astype(dtype)[..., None]
    ce = _sce(object_mask, out[..., 4:5])
    conf = object_mask * ce + (1 - object_mask) * ce * ignore_mask
    cls = object_mask * _sce(y_true[..., 5:], out[..., 5:])
    gl = object_mask * (1 - giou(pred_box, true_box)[..., None])
    res = {'giou': np.sum(gl) / m, 'conf': np.sum(conf) / m, 'cls': np.sum(cls) / m,
           'ignore_sum': float(np.sum(ignore_mask)), 'best_iou': best_iou}
    res['loss'] = res['giou'] + res['conf'] + res['cls']
    return res


def terms(res):
    """-> [loss, giou, conf, cls, ignore_sum] as float64, the order of the device's five words."""
    return np.array([res['loss'], res['giou'], res['conf'], res['cls'], res['ignore_sum']], np.float64)


def random_case(seed, batch, input_hw, num_classes, anchors, scales=(0, 1, 2), boxes_per_image=4, slot_anchors=None):
    """The parity recipe: RandomState(seed).randn logits; per image and scale `boxes_per_image` labelled boxes at random
    cells and slots, size = the slot's anchor x U(0.6, 1.6) per side, centre uniform inside the cell, one class bit (none
    with num_classes == 0).  -> {scale: (logits, y_true)} float32 [B,gh,gw,A,5+C].
    A = 3 and the slots' anchors are scale_anchors(anchors, s), unless ``slot_anchors`` ([A,2], any A) names them: then every
    scale of ``scales`` (which only sets the grid step) works with those A anchors and ``anchors`` is not read.  The defaults
    draw what they always drew: the cases of the existing tests keep their bytes."""
    rs = np.random.RandomState(seed)
    case = {}
    for s in scales:
        gh, gw = input_hw[0] // GRID_STEPS[s], input_hw[1] // GRID_STEPS[s]
        an = scale_anchors(anchors, s) if slot_anchors is None else np.asarray(slot_anchors, np.float32).reshape(-1, 2)
        na = an.shape[0]
        logits = rs.randn(batch, gh, gw, na, 5 + num_classes).astype(np.float32)
        y_true = np.zeros_like(logits)
        for b in range(batch):
            for _ in range(boxes_per_image):
                j, i, k = rs.randint(gh), rs.randint(gw), rs.randint(na)
                w, h = an[k] * rs.uniform(0.6, 1.6, 2)
                cx, cy = (i + rs.uniform()) / gw, (j + rs.uniform()) / gh
                y_true[b, j, i, k] = 0
                y_true[b, j, i, k, :5] = (cx, cy, w / input_hw[1], h / input_hw[0], 1)
                if num_classes:
                    y_true[b, j, i, k, 5 + rs.randint(num_classes)] = 1
        case[s] = (logits, y_true)
    return case


def threshold_margin(res, ignore_thresh=.5):
    """Smallest distance of any best IoU from the threshold: the GPU tests require > 1e-5 of the float64 result."""
    return float(np.min(np.abs(res['best_iou'] - ignore_thresh)))
