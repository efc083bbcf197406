"""Helpers adjacent to the detection path (reference code/yolo3/utils.py)."""
import os
from functools import reduce

import numpy as np

_MODEL_DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'model_data')


def compose(*funcs):
    """Compose arbitrarily many functions, evaluated left to right (utils.py:56-64)."""
    if funcs:
        return reduce(lambda f, g: lambda *a, **kw: g(f(*a, **kw)), funcs)
    raise ValueError('Composition of empty sequence not supported.')


def _resolve(path):
    """Accepts the reference's relative ``model_data/...`` paths as well as real paths."""
    if os.path.exists(path):
        return path
    alt = os.path.join(_MODEL_DATA, os.path.basename(path))
    if os.path.exists(alt):
        return alt
    if os.path.exists(alt + '.txt'):  # yolo.py:174's default lacks the extension
        return alt + '.txt'
    raise FileNotFoundError(path)


def get_anchors(anchors_path):
    """float32 [9,2] (w,h) anchors (utils.py:100-104)."""
    with open(_resolve(anchors_path)) as f:
        anchors = f.readline()
    anchors = [float(x) for x in anchors.split(',')]
    return np.array(anchors, np.float32).reshape(-1, 2)


def get_classes(classes_path):
    """class names, one per line (utils.py:115-120)."""
    with open(_resolve(classes_path)) as f:
        class_names = f.readlines()
    return [c.strip() for c in class_names]


def _divide_no_nan(a, b):
    """tf.math.divide_no_nan: 0 where the denominator is 0."""
    a, b = np.broadcast_arrays(a, b)
    out = np.zeros(a.shape, a.dtype)
    np.divide(a, b, out=out, where=b != 0)
    return out


def do_giou_calculate(b1, b2, mode='giou'):
    """IoU / GIoU of boxes (y_min, x_min, y_max, x_max) on the last axis, broadcasting over the others (utils.py:9-53).
    Host NumPy in the dtype of ``b1`` - the label encoding below uses it; the loss itself runs in the HIP kernels."""
    b1 = np.asarray(b1)
    b2 = np.asarray(b2, b1.dtype)
    zero = b1.dtype.type(0)
    b1_ymin, b1_xmin, b1_ymax, b1_xmax = (b1[..., i] for i in range(4))
    b2_ymin, b2_xmin, b2_ymax, b2_xmax = (b2[..., i] for i in range(4))
    b1_area = np.maximum(zero, b1_xmax - b1_xmin) * np.maximum(zero, b1_ymax - b1_ymin)
    b2_area = np.maximum(zero, b2_xmax - b2_xmin) * np.maximum(zero, b2_ymax - b2_ymin)
    intersect_width = np.maximum(zero, np.minimum(b1_xmax, b2_xmax) - np.maximum(b1_xmin, b2_xmin))
    intersect_height = np.maximum(zero, np.minimum(b1_ymax, b2_ymax) - np.maximum(b1_ymin, b2_ymin))
    intersect_area = intersect_width * intersect_height
    union_area = b1_area + b2_area - intersect_area
    iou = _divide_no_nan(intersect_area, union_area)
    if mode == 'iou':
        return iou
    enclose_width = np.maximum(zero, np.maximum(b1_xmax, b2_xmax) - np.minimum(b1_xmin, b2_xmin))
    enclose_height = np.maximum(zero, np.maximum(b1_ymax, b2_ymax) - np.minimum(b1_ymin, b2_ymin))
    enclose_area = enclose_width * enclose_height
    return iou - _divide_no_nan(enclose_area - union_area, enclose_area)


def preprocess_true_boxes(true_boxes, input_shape, anchors, num_classes, num_scales):
    """Labelled boxes of ONE image -> the y_true arrays the loss reads (utils.py:298-376).

    true_boxes [T,5]: x_min, y_min, x_max, y_max, class id, in pixels of the network input; input_shape (h,w), multiples of
    32; anchors [9,2] (w,h).  Returns float32 arrays [gh,gw,3,5+num_classes], one per scale (a single array for
    num_scales == 1, else a tuple): (x, y, w, h) relative to the input, object flag, one class bit.  Stack them over the batch.

    The reference's behaviour is kept where it is peculiar: centres come from a floor division (:321), a box is valid when its
    WIDTH is positive (:342), argmax ties go to the first anchor, the last writer of a (cell, slot) wins, and the index that
    runs over the valid boxes addresses the unfiltered array (:356-366) - right when the zero padding rows come last, which is
    how the reference's pipeline pads."""
    anchor_mask = [[6, 7, 8], [3, 4, 5], [0, 1, 2]][-1 * num_scales:]
    true_boxes = np.array(true_boxes, dtype='float32')
    input_shape = np.array(input_shape, dtype='int32')
    boxes_xy = (true_boxes[..., 0:2] + true_boxes[..., 2:4]) // 2
    boxes_wh = true_boxes[..., 2:4] - true_boxes[..., 0:2]
    true_boxes[..., 0:2] = boxes_xy / input_shape[::-1]
    true_boxes[..., 2:4] = boxes_wh / input_shape[::-1]
    grid_steps = [32, 16, 8]
    grid_shapes = [np.round(input_shape / grid_steps[l]).astype(np.int32) for l in range(num_scales)]
    y_true = [np.zeros((grid_shapes[l][0], grid_shapes[l][1], len(anchor_mask[l]), 5 + num_classes), dtype='float32')
              for l in range(num_scales)]
    # the anchor whose shape, centred on the box, overlaps it most
    anchor_maxes = np.expand_dims(np.asarray(anchors), 0) / 2.
    wh = np.expand_dims(boxes_wh[boxes_wh[..., 0] > 0], -2)
    box_maxes = wh / 2.
    anchor_box = np.stack([-anchor_maxes[..., 1], -anchor_maxes[..., 0], anchor_maxes[..., 1], anchor_maxes[..., 0]], axis=-1)
    bbox = np.stack([-box_maxes[..., 1], -box_maxes[..., 0], box_maxes[..., 1], box_maxes[..., 0]], axis=-1)
    best_anchor = np.argmax(do_giou_calculate(anchor_box, bbox, mode='iou'), axis=-1)
    slot_of = {n: (l, k) for l, mask in enumerate(anchor_mask) for k, n in enumerate(mask)}   # anchor -> (scale, slot)
    for t, n in enumerate(best_anchor):      # t counts the VALID boxes but indexes the unfiltered rows (see above)
        if int(n) not in slot_of:
            continue                         # (an anchor of a scale that num_scales leaves out)
        l, k = slot_of[int(n)]
        gh, gw = grid_shapes[l]
        col = int(np.floor(true_boxes[t, 0] * gw))
        row = int(np.floor(true_boxes[t, 1] * gh))
        entry = y_true[l][row, col, k]       # a later box of the same cell and slot overwrites the box; class bits accumulate
        entry[0:4] = true_boxes[t, 0:4]
        entry[4] = 1.
        entry[5 + int(true_boxes[t, 4])] = 1.
    return y_true[0] if num_scales == 1 else tuple(y_true)


def preprocess_true_boxes_device(true_boxes, input_shape, anchors, num_classes, num_scales, device=None):
    """The batched twin of ``preprocess_true_boxes`` on the device (the HIP kernels behind ``yr_encode_labels``).

    true_boxes [B,T,5]: the host function's rows for B images, T <= 256, as a NumPy array (copied to ``device``, default the
    current CUDA device: a few KB) or a float32 CUDA tensor (``device`` is then its own).  Returns float32 device tensors
    [B,gh,gw,3,5+num_classes], one per scale (a single tensor for num_scales == 1, else a tuple): byte for byte the host
    function's arrays stacked over the batch.  Rows it could not write are not written: a row with a non-finite value is
    removed from the list first (the others are encoded as if it were absent); a row with a class or cell out of range keeps its
    place in the list - and so its part in the reference's pairing of anchors and rows - and only its own write is dropped.
    ``runtime.encode_labels(..., skipped=)`` counts both kinds per image."""
    import torch
    from .. import runtime as rt
    if not isinstance(true_boxes, torch.Tensor):
        true_boxes = np.asarray(true_boxes) if isinstance(true_boxes, np.ndarray) else np.asarray(true_boxes, np.float32)
        if true_boxes.dtype != np.float32:
            raise ValueError('preprocess_true_boxes_device: a %s array, float32 rows expected' % true_boxes.dtype)
        host = torch.from_numpy(np.ascontiguousarray(true_boxes))
        rt.label_args(host, input_shape, anchors, num_classes, num_scales)     # (raises before anything is copied)
        true_boxes = host.to(torch.device('cuda', torch.cuda.current_device()) if device is None else device)
    elif device is not None and (torch.device(device).type != true_boxes.device.type
                                 or torch.device(device).index not in (None, true_boxes.device.index)):
        raise ValueError('preprocess_true_boxes_device: true_boxes is on %s, device=%s' % (true_boxes.device, device))
    y_true = rt.encode_labels(true_boxes, input_shape, anchors, num_classes, num_scales)
    return y_true[0] if num_scales == 1 else y_true


def _augment_params(min_scale, max_scale, jitter, min_gamma, max_gamma, blur, hue, sat, val, cont, noise, zoom_in):
    """The reference's keyword arguments -> the parameters of ``runtime.augment_geometry``; raises for the steps that are not built."""
    if val > 0:
        raise NotImplementedError('get_random_data_device(val=%r): random_brightness is not built' % (val,))
    if noise > 0:
        raise NotImplementedError('get_random_data_device(noise=%r): the additive noise is not built' % (noise,))
    if blur:
        raise NotImplementedError('get_random_data_device(blur=True): random_blur is not built')
    if zoom_in:
        raise NotImplementedError('get_random_data_device(zoom_in=True): the zoom-in branch is not built')
    return dict(jitter=jitter, min_scale=min_scale, max_scale=max_scale, hue=hue, sat=sat, min_gamma=min_gamma, max_gamma=max_gamma, cont=cont)


def _check_jpeg_bounds(min_jpeg_quality, max_jpeg_quality):
    """tf.image.random_jpeg_quality's own argument check."""
    if min_jpeg_quality < 0 or max_jpeg_quality < 0 or min_jpeg_quality > 100 or max_jpeg_quality > 100:
        raise ValueError('jpeg encoding range must be between 0 and 100.')
    if min_jpeg_quality >= max_jpeg_quality:
        raise ValueError('`min_jpeg_quality` must be less than `max_jpeg_quality`.')


def draw_jpeg_quality(u, min_jpeg_quality, max_jpeg_quality):
    """One image's quality from a uniform ``u`` in [0, 1) (float32): TensorFlow draws an int32 uniformly in [min, max); here, in
    double, min + int(u * (max - min)), kept below max; libjpeg reads quality 0 as 1."""
    lo, hi = int(min_jpeg_quality), int(max_jpeg_quality)
    return max(min(lo + int(float(np.float32(u)) * (hi - lo)), hi - 1), 1)


def random_jpeg_quality_device(images, min_jpeg_quality, max_jpeg_quality, draws=None, seed=None):
    """``tf.image.random_jpeg_quality`` (utils.py:228-230) for a batch on the device, IN PLACE: images float32 CUDA [B,H,W,3] with H
    and W multiples of 16, each encoded as a JPEG (4:2:0) at a quality drawn uniformly from [min_jpeg_quality, max_jpeg_quality) and
    decoded again - the HIP kernels behind ``yr_jpeg_roundtrip_batch``, bit for bit libjpeg's integer arithmetic, no bitstream.
    ``draws``: float32 [B] uniforms in [0, 1), one per image; None draws them from ``np.random.default_rng(seed)``.  ValueError
    unless 0 <= min_jpeg_quality < max_jpeg_quality <= 100, as TensorFlow raises.  Returns (images, quality int32 [B] as drawn)."""
    from .. import runtime as rt
    _check_jpeg_bounds(min_jpeg_quality, max_jpeg_quality)
    b = int(images.shape[0])
    if draws is None:
        draws = np.random.default_rng(seed).random(b, dtype=np.float32)
    draws = np.asarray(draws, np.float32).reshape(-1)
    if draws.shape[0] != b:
        raise ValueError('random_jpeg_quality_device: %d draws for %d images' % (draws.shape[0], b))
    quality = np.array([draw_jpeg_quality(u, min_jpeg_quality, max_jpeg_quality) for u in draws], np.int32)
    return rt.jpeg_roundtrip_batch(images, quality), quality


def get_random_data_device(images, boxes, counts, input_shape, draws=None, seed=None, min_scale=0.25, max_scale=2, jitter=0.3,
                           min_gamma=0.8, max_gamma=2, blur=False, flip=True, hue=.5, sat=.5, val=0., cont=.1, noise=0, max_boxes=20,
                           min_jpeg_quality=80, max_jpeg_quality=100, zoom_in=False, device=None, stager=None, apply_jpeg=False,
                           jpeg_draws=None):
    """The batch-level mirror of ``get_random_data(train=True)`` (utils.py:120-237, then :258-293) on the device: the HIP kernels
    behind ``yr_augment_batch`` and, with ``apply_jpeg=True``, ``yr_jpeg_roundtrip_batch``.

    images: a list of B decoded uint8 arrays [h,w,3] of any sizes; boxes: float32 [B,max_in,5] rows (xmin, ymin, xmax, ymax, label)
    in source pixels (NumPy or a CUDA tensor); counts: int32 [B], the rows of each image that are boxes.  ``draws``: float32 [B,10]
    uniforms in [0, 1), per image in the reference's order j1, j2, scale, dx, dy, flip, hue, sat, gamma, contrast; None draws them
    from ``np.random.default_rng(seed)``.  Returns (images float32 [B,H,W,3], boxes_out [B,max_boxes,5], kept int32 [B]) on the device.

    ``jitter``, ``min_scale``, ``max_scale``, ``min_gamma``, ``max_gamma``, ``flip``, ``hue``, ``sat`` and ``cont`` are honoured, each
    step switched off by the reference's own condition.  ``val``, ``noise``, ``blur`` and ``zoom_in`` raise NotImplementedError when
    switched on.

    ``apply_jpeg``: ``random_jpeg_quality`` (:228-230), the last image step, which the reference applies by default with the bounds
    80 / 100.  ``apply_jpeg=True`` IS THE REFERENCE'S DEFAULT BEHAVIOUR; the default here is False, which keeps the bytes this
    function returned before the step was built, and then ``min_jpeg_quality`` / ``max_jpeg_quality`` are accepted and unused.  With
    ``apply_jpeg=True`` the step runs iff ``min_jpeg_quality < max_jpeg_quality`` (the reference's condition; bounds outside 0..100
    raise ValueError as TensorFlow does) and needs both sides of ``input_shape`` to be multiples of 16.  ``jpeg_draws``: float32 [B]
    uniforms in [0, 1), one per image; None draws them from a second generator, ``np.random.default_rng((seed, 1))``, so the ten
    draws above do not depend on this switch.  The draws are NumPy's, not TensorFlow's generator: the distribution is the
    reference's, the stream is not."""
    import torch
    from .. import runtime as rt
    params = _augment_params(min_scale, max_scale, jitter, min_gamma, max_gamma, blur, hue, sat, val, cont, noise, zoom_in)
    jpeg = bool(apply_jpeg) and min_jpeg_quality < max_jpeg_quality
    if jpeg:
        _check_jpeg_bounds(min_jpeg_quality, max_jpeg_quality)
        if int(input_shape[0]) % 16 or int(input_shape[1]) % 16:
            raise ValueError('get_random_data_device(apply_jpeg=True): input_shape must be multiples of 16, not %s' % (tuple(input_shape),))
    b = len(images)
    if draws is None:
        draws = np.random.default_rng(seed).random((b, 10), dtype=np.float32)
    if jpeg and jpeg_draws is None:
        jpeg_draws = np.random.default_rng((seed, 1) if seed is not None else None).random(b, dtype=np.float32)
    dev = torch.device(device if device is not None else (boxes.device if isinstance(boxes, torch.Tensor) else 'cuda:0'))
    table = rt.augment_geometry([np.shape(im)[:2] for im in images], input_shape, draws, flip=flip, **params)
    stager = rt.RaggedStager(dev) if stager is None else stager
    packed, table = stager.upload_table(images, table)
    if not isinstance(boxes, torch.Tensor):
        boxes = torch.from_numpy(np.array(boxes, dtype=np.float32)).to(dev)
    if not isinstance(counts, torch.Tensor):
        counts = torch.from_numpy(np.array(counts, dtype=np.int32)).to(dev)
    x, boxes_out, kept = rt.augment_batch(packed, table, input_shape, boxes=boxes, box_count=counts, max_boxes=max_boxes)
    if jpeg:
        random_jpeg_quality_device(x, min_jpeg_quality, max_jpeg_quality, draws=jpeg_draws)
    return x, boxes_out, kept
