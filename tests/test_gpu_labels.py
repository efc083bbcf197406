"""yr_encode_labels (yoloret_amd/csrc/labels.hip) against the host function yoloret_amd.yolo3.utils.preprocess_true_boxes applied
image by image.  Every comparison is on raw bytes (uint32 views): no tolerance, no excluded element.  Every C-ABI call goes
through tests/fence.run with the label tensors and `skipped` as written tensors and the boxes as the read one; the written tensors
are pre-filled with NaN (skipped: a sentinel), so an element the zero-fill missed shows up.

Shapes are the smallest at which the encoder can go wrong: T = 1 (one lane), T = 20 (part of a wave), T = 256 (all four waves, the
prefix over waves), grids of 1x2 cells (collisions) up to 52x52, tensors whose byte count is no multiple of 16 (C = 20 at odd
cell counts: the fill's tail), a non-square input, and batch 64 at 416 (the size the entry is for)."""
import numpy as np
import pytest
import torch

from tests import fence
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

SENTINEL = -99


def _rt():
    from yoloret_amd import runtime as rt
    return rt


def host_labels(boxes, hw, c, num_scales):
    """the yardstick: the host function image by image, stacked -> [num_scales] arrays [B,gh,gw,3,5+C]"""
    from yoloret_amd.yolo3.utils import preprocess_true_boxes
    per_image = [preprocess_true_boxes(t, hw, ANCHORS, c, num_scales) for t in boxes]
    if num_scales == 1:
        per_image = [(p,) for p in per_image]
    return [np.stack([p[s] for p in per_image]) for s in range(num_scales)]


def device_labels(dev, boxes, hw, c, num_scales):
    """NumPy in, NumPy out, through the C entry between the guards of tests/fence.py -> ([num_scales] arrays, skipped [B])"""
    rt = _rt()
    b, t = boxes.shape[:2]
    tb = torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(dev)
    ys = [torch.full(shp, float('nan'), dtype=torch.float32, device=dev) for shp in rt.label_shapes(b, hw, c, num_scales)]
    skipped = torch.full((b,), SENTINEL, dtype=torch.int32, device=dev)
    an = np.ascontiguousarray(ANCHORS, np.float32)

    def call(moved):
        p = [rt._ptr(moved(y)) for y in ys] + [None] * (3 - num_scales)
        with torch.cuda.device(dev):
            rt.check(rt.lib().yr_encode_labels(rt._ptr(moved(tb)), b, t, hw[0], hw[1], an.ctypes.data, c, num_scales, p[0], p[1], p[2],
                                               rt._ptr(moved(skipped)), rt.stream_ptr(dev)))
    fence.run(call, writes=ys + [skipped], reads=[tb], batch=b)
    torch.cuda.synchronize()
    return [y.cpu().numpy() for y in ys], skipped.cpu().numpy()


def same_bytes(got, want, what):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.float32 and w.dtype == np.float32, (what, s, g.shape, w.shape)
        d = g.view(np.uint32) != w.view(np.uint32)
        assert not d.any(), '%s scale %d: %d of %d words differ, the first at %s: device %r, host %r' % (
            what, s, int(d.sum()), d.size, tuple(np.argwhere(d)[0]), g[tuple(np.argwhere(d)[0])], w[tuple(np.argwhere(d)[0])])


def objects(y):
    return int((y[..., 4] != 0).sum())


def random_boxes(seed, b, t, hw, c, full=False):
    """integer pixels inside the input, width >= 1 (height >= 0), sizes spread over the anchors' range, integer classes, a random
    number of zero padding rows last (none with `full`)"""
    rs = np.random.RandomState(seed)
    h, w = hw
    out = np.zeros((b, t, 5), np.float32)
    for i in range(b):
        n = t if full else rs.randint(1, t + 1)
        bw = np.clip(np.round(np.exp(rs.uniform(0, np.log(w), n))), 1, w).astype(np.int64)
        bh = np.clip(np.round(np.exp(rs.uniform(0, np.log(h), n))), 0, h).astype(np.int64) * (rs.rand(n) > .05)
        x0 = (rs.rand(n) * (w - bw + 1)).astype(np.int64)
        y0 = (rs.rand(n) * (h - bh)).astype(np.int64)      # y0 <= h - 1: the centre row stays inside
        out[i, :n] = np.stack([x0, y0, x0 + bw, y0 + bh, rs.randint(0, c, n)], -1)
    assert (out[..., 2] <= w).all() and (out[..., 3] <= h).all() and (out[..., :2] >= 0).all()
    return out


def check_parity(dev, boxes, hw, c, num_scales, what, every_scale=True):
    want = host_labels(boxes, hw, c, num_scales)
    counts = [objects(y) for y in want]
    print('%s: objects per scale %s' % (what, counts))
    if every_scale:
        assert all(counts), '%s: a scale without an object (%s) - choose another seed' % (what, counts)
    else:
        assert sum(counts) > 0
    got, skipped = device_labels(dev, boxes, hw, c, num_scales)
    same_bytes(got, want, what)
    assert skipped.tolist() == [0] * boxes.shape[0]
    return want


# ----------------------------------------------------------------------------- known answers
def test_known_answer_one_box(dev):
    """(414,414,415,415,3) at 416: centre floor(829 / 2) = 414, size 1 x 1.  The IoU of a centred 1 x 1 box with a centred anchor that
    contains it is 1 / (the anchor's area): largest for anchor 0 (10 x 13) -> scale 2 (stride 8, grid 52), slot 0; cell
    floor(414 / 416 * 52) = floor(51.75) = 51 on both axes."""
    got, skipped = device_labels(dev, np.array([[[414, 414, 415, 415, 3]]], np.float32), (416, 416), 20, 3)
    want = [np.zeros((1, g, g, 3, 25), np.float32) for g in (13, 26, 52)]
    want[2][0, 51, 51, 0, :5] = (np.float32(414.0 / 416.0), np.float32(414.0 / 416.0), np.float32(1.0 / 416.0), np.float32(1.0 / 416.0), 1)
    want[2][0, 51, 51, 0, 5 + 3] = 1
    same_bytes(got, want, 'one box')
    assert skipped.tolist() == [0] and [objects(y) for y in got] == [0, 0, 1]


def test_known_answer_all_zero(dev):
    got, skipped = device_labels(dev, np.zeros((1, 1, 5), np.float32), (416, 416), 20, 3)
    for y in got:
        assert not y.view(np.uint32).any()
    assert skipped.tolist() == [0]


# ----------------------------------------------------------------------------- random parity
@pytest.mark.parametrize('b,t,seed', [(1, 1, 0), (1, 20, 4), (3, 1, 97), (3, 20, 0)])
def test_parity_96(dev, b, t, seed):
    """(one box cannot land on three scales: with B * T = 1 the CPU-side condition is 'an object', not 'an object at every scale')"""
    check_parity(dev, random_boxes(seed, b, t, (96, 96), 20, full=(t == 1)), (96, 96), 20, 3, '96 B%d T%d' % (b, t), every_scale=b * t > 1)


def test_parity_416_batch_64(dev):
    check_parity(dev, random_boxes(0, 64, 20, (416, 416), 20), (416, 416), 20, 3, '416 B64')


def test_parity_416_80_classes(dev):
    check_parity(dev, random_boxes(1, 4, 20, (416, 416), 80), (416, 416), 80, 3, '416 C80')


def test_parity_non_square_one_class(dev):
    check_parity(dev, random_boxes(2, 3, 20, (320, 416), 1), (320, 416), 1, 3, '320x416 C1')


@pytest.mark.parametrize('num_scales', [1, 2, 3])
def test_parity_scale_subsets(dev, num_scales):
    """with fewer than 3 scales the small anchors meet stride 32 and the boxes of the other anchors land nowhere"""
    boxes = random_boxes(4, 2, 20, (96, 96), 20)
    want = check_parity(dev, boxes, (96, 96), 20, num_scales, '96 scales %d' % num_scales)
    assert want[0].shape[1:3] == (3, 3)
    if num_scales < 3:
        assert sum(objects(y) for y in want) < sum(objects(y) for y in host_labels(boxes, (96, 96), 20, 3))


def test_parity_256_rows(dev):
    check_parity(dev, random_boxes(6, 2, 256, (96, 96), 20, full=True), (96, 96), 20, 3, '96 T256')


# ----------------------------------------------------------------------------- collisions
def test_collisions_last_writer_wins_and_class_bits_accumulate(dev):
    """grids 1x2 / 2x4 / 4x8 and 64 rows per image: most rows share their (cell, slot) with others"""
    hw, c = (32, 64), 5
    boxes = random_boxes(7, 2, 64, hw, c, full=True)
    # where each row lands (every row is valid, so rank == row): the host function on that row alone
    worst = 0
    for img in boxes:
        hits = {}
        for row in img:
            ys = host_labels(row[None, None], hw, c, 3)
            (s,) = [i for i in range(3) if objects(ys[i])]
            where = (s,) + tuple(np.argwhere(ys[s][0, ..., 4] != 0)[0])
            hits.setdefault(where, []).append(int(row[4]))
        worst = max(worst, max(len(v) for v in hits.values() if len(set(v)) >= 2))
    assert worst >= 3, 'no (cell, slot) hit by >= 3 rows of >= 2 classes'
    want = check_parity(dev, boxes, hw, c, 3, 'collisions', every_scale=False)      # (boxes of 32 x 64 pixels reach no large anchor)
    assert max(int(y[..., 5:].sum(-1).max()) for y in want) >= 2       # an entry with two class bits


# ----------------------------------------------------------------------------- the index quirk
def test_index_quirk_invalid_rows_anywhere(dev):
    """The r-th VALID row supplies the anchor, row r of the unfiltered rows the coordinates: with invalid rows (zero width, or
    x_max < x_min) in front of valid ones the two differ.  All rows lie inside the input, so the host function writes inside its
    grids whichever row it takes the coordinates from."""
    g = [[10, 20, 70, 80, 3], [40, 8, 64, 60, 7], [50, 50, 62, 70, 0], [2, 30, 90, 66, 11], [60, 60, 76, 90, 19], [5, 5, 15, 18, 1]]
    z, zw, neg = [0, 0, 0, 0, 0], [30, 40, 30, 70, 4], [80, 10, 20, 50, 9]       # padding, zero width, x_max < x_min
    images = [[zw] + g + [z],                              # an invalid row first
              g[:3] + [neg] + g[3:] + [z],                 # one in the middle
              g[:2] + [zw, neg, z] + g[2:5] ,              # a run
              [z, zw, neg, zw, z, neg, z, z],              # all invalid: nothing is written
              [neg, zw] + g[:1] + [z] + g[1:4] + [neg]]    # invalid rows at both ends
    boxes = np.array(images, np.float32)
    want = host_labels(boxes, (96, 96), 20, 3)
    plain = host_labels(np.array([g + [z, z]] * 5, np.float32), (96, 96), 20, 3)
    assert any((w[i].view(np.uint32) != p[i].view(np.uint32)).any() for w, p in zip(want, plain) for i in (0, 1, 2, 4)), 'the quirk does not show'
    assert sum(objects(w[3:4]) for w in want) == 0
    got, skipped = device_labels(dev, boxes, (96, 96), 20, 3)
    same_bytes(got, want, 'index quirk')
    assert skipped.tolist() == [0] * 5


# ----------------------------------------------------------------------------- rows the host function does not write
def test_skipped_rows(dev):
    """Known answers: each bad row sits among good rows; the result must be what the host function gives for the good rows alone, in
    the same relative order, padded with zeros last, and `skipped` the number of bad rows of the image.  (The good rows are all
    valid, so every bad row comes to its turn.)"""
    hw, c, t = (96, 96), 20, 12
    nan, inf = float('nan'), float('inf')
    good = random_boxes(8, 16, 8, hw, c, full=True)
    bad = [[[10, 10, 30, 30, c]],                       # class = C
           [[10, 10, 30, 30, -1]],                      # class = -1
           [[94, 10, 98, 30, 1]],                       # centre at x = in_w
           [[10, 94, 30, 98, 1]],                       # centre at y = in_h
           [[-40, 10, 10, 30, 1]],                      # centre at x = -15
           [[nan, 10, 30, 30, 1]], [[10, nan, 30, 30, 1]], [[10, 10, nan, 30, 1]], [[10, 10, 30, nan, 1]], [[10, 10, 30, 30, nan]],
           [[inf, 10, 30, 30, 1]], [[10, 10, inf, 30, 1]], [[10, 10, 30, inf, 1]], [[10, 10, 30, 30, inf]], [[10, -inf, 30, 30, 1]],
           [[10, 10, 30, 30, c + .5], [nan, nan, nan, nan, nan], [10, 10, 30, 30, -1.5], [1e30, 1e30, 3e38, 3e38, 0]]]
    boxes = np.zeros((len(bad), t, 5), np.float32)
    alone = np.zeros_like(boxes)
    for i, rows in enumerate(bad):
        at = sorted(set(np.random.RandomState(i).randint(0, 9, len(rows)).tolist()))      # where the bad rows go
        at += [8] * (len(rows) - len(at))
        merged = list(good[i])
        for p, r in zip(reversed(at), reversed(rows)):
            merged.insert(p, np.array(r, np.float32))
        boxes[i, :len(merged)] = np.array(merged, np.float32)
        alone[i, :8] = good[i]
    assert not np.isfinite(boxes).all()
    want = host_labels(alone, hw, c, 3)
    got, skipped = device_labels(dev, boxes, hw, c, 3)
    same_bytes(got, want, 'skipped rows')
    assert skipped.tolist() == [len(rows) for rows in bad]


def test_skipped_rows_of_both_kinds_side_by_side(dev):
    """A non-finite row and a row dropped at its turn are two rows of the count, also when the lane that holds the first plays the
    second as a rank: the non-finite row directly in front of a class- or cell-skipped row, and the pair at rows 0 and 1."""
    hw, c, t = (96, 96), 20, 10
    nan, inf = float('nan'), float('inf')
    good = random_boxes(12, 4, 6, hw, c, full=True)
    bad_class, bad_cell, low_class = [10, 10, 30, 30, c], [94, 10, 98, 30, 1], [10, 10, 30, 30, -1]
    layouts = [[[nan, 10, 30, 30, 1], bad_class, 0, 1, 2, 3, 4, 5],                              # rows 0 and 1
               [[10, 10, 30, inf, 1], bad_cell, 0, 1, 2, 3, 4, 5],
               [0, 1, 2, [10, 10, 30, 30, nan], low_class, 3, 4, 5],                             # in the middle
               [[nan] * 5, [inf, 10, 30, 30, 1], bad_class, bad_cell, 0, 1, 2, 3, 4, 5]]        # two and two
    boxes = np.zeros((4, t, 5), np.float32)
    alone = np.zeros_like(boxes)
    for i, rows in enumerate(layouts):
        boxes[i, :len(rows)] = np.array([good[i, r] if isinstance(r, int) else r for r in rows], np.float32)
        alone[i, :6] = good[i]
    want = host_labels(alone, hw, c, 3)
    got, skipped = device_labels(dev, boxes, hw, c, 3)
    same_bytes(got, want, 'both kinds')
    assert skipped.tolist() == [2, 2, 2, 4]


def test_no_classes_no_class_bit_to_write(dev):
    """num_classes = 0 is accepted and an entry is then 5 floats: there is no class bit, the host function raises IndexError for every
    row it comes to, so every such row is skipped - also a class in (-1, 0), which truncates to 0.  The rows aim at the LAST entry
    of the last tensor (33 x 23 pixels: anchor 2 = slot 2 of stride 8; centre (88, 88) of 96 = cell (11, 11)), where a class bit
    would be written past the end, and at the first."""
    hw = (96, 96)
    rows = [[72, 77, 105, 100, -0.5], [72, 77, 105, 100, 0], [72, 77, 105, 100, -0.0], [0, 0, 5, 6, -0.9], [0, 0, 33, 23, 0.5]]
    boxes = np.array([rows, rows[::-1]], np.float32)
    from yoloret_amd.yolo3.utils import preprocess_true_boxes
    probe = preprocess_true_boxes(np.array([[72, 77, 105, 100, 0]], np.float32), hw, ANCHORS, 1, 3)[2]     # where it lands with one class
    assert probe[11, 11, 2, 4] == 1 and objects(probe) == 1
    with pytest.raises(IndexError):
        preprocess_true_boxes(boxes[0], hw, ANCHORS, 0, 3)
    got, skipped = device_labels(dev, boxes, hw, 0, 3)
    assert [g.shape for g in got] == [(2, 3, 3, 3, 5), (2, 6, 6, 3, 5), (2, 12, 12, 3, 5)]
    for g in got:
        assert not g.view(np.uint32).any()
    assert skipped.tolist() == [5, 5]


def test_fractional_class_is_truncated_not_skipped(dev):
    """class 2.7 is written as class 2 (int() truncates toward zero), -0.5 as class 0: the host function does the same"""
    boxes = random_boxes(9, 1, 8, (96, 96), 20, full=True)
    boxes[0, 3, 4] = 2.7
    boxes[0, 5, 4] = -0.5
    want = check_parity(dev, boxes, (96, 96), 20, 3, 'class 2.7', every_scale=False)
    ref = boxes.copy()
    ref[0, 3, 4], ref[0, 5, 4] = 2, 0
    same_bytes(want, host_labels(ref, (96, 96), 20, 3), 'class 2.7 on the host')


# ----------------------------------------------------------------------------- reproducibility
def test_same_bytes_across_calls_streams_and_out_tensors(dev):
    rt = _rt()
    boxes = random_boxes(10, 8, 20, (416, 416), 20)
    tb = torch.from_numpy(boxes).to(dev)
    sk = [torch.full((8,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(4)]
    first = rt.encode_labels(tb, (416, 416), ANCHORS, 20, 3, skipped=sk[0])
    again = rt.encode_labels(tb, (416, 416), ANCHORS, 20, 3, skipped=sk[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        third = rt.encode_labels(tb, (416, 416), ANCHORS, 20, 3, skipped=sk[2])
    side.synchronize()
    out = [torch.randn(y.shape, device=dev) for y in first]
    ptrs = [o.data_ptr() for o in out]
    fourth = rt.encode_labels(tb, (416, 416), ANCHORS, 20, 3, out=out, skipped=sk[3])
    torch.cuda.synchronize()
    assert [o.data_ptr() for o in fourth] == ptrs and isinstance(first, tuple) and len(first) == 3
    want = host_labels(boxes, (416, 416), 20, 3)
    for res in (first, again, third, fourth):
        same_bytes([y.cpu().numpy() for y in res], want, 'reproducibility')
    assert all(s.tolist() == [0] * 8 for s in sk)


# ----------------------------------------------------------------------------- through the public surface
def test_loss_from_boxes_equals_loss_of_host_labels(dev):
    """size and model of tests/test_gpu_loss.py::test_loss_of_model_logits"""
    from oracle import model as om, params
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3 import model as m
    from yoloret_amd.yolo3.utils import preprocess_true_boxes_device
    hw, b, c = (96, 96), 2, 20
    net = m.yolov3_body(L.Input(shape=[hw[0], hw[1], 3]), 'mobilenetv2x75', 3, num_classes=c)
    P = params.ParamStore(1234)
    x = params.synthetic_images(b, hw[0], hw[1])
    om.yolov3_body(P, x, 'mobilenetv2x75', 3, c)      # (draws the synthetic weights)
    net.set_weights(P.values)
    ys = net(torch.from_numpy(x).to(dev))
    boxes = np.array([[[10, 20, 70, 80, 3], [40, 8, 64, 60, 7], [50, 50, 62, 70, 0], [0, 0, 0, 0, 0]],
                      [[2, 30, 90, 66, 11], [60, 60, 76, 90, 19], [5, 5, 15, 18, 1], [70, 10, 92, 34, 5]]], np.float32)
    y_trues = host_labels(boxes, hw, c, 3)
    assert sum(objects(y) for y in y_trues) == 7
    total0, terms0 = m.yolo_loss(ys, [torch.from_numpy(y).to(dev) for y in y_trues], ANCHORS, 3)
    total1, terms1 = m.yolo_loss_from_boxes(ys, boxes, ANCHORS, c, 3)
    total2, terms2 = m.yolo_loss_from_boxes(ys, torch.from_numpy(boxes).to(dev), ANCHORS, c, 3)
    torch.cuda.synchronize()
    t0 = terms0.cpu().numpy()
    assert t0.shape == (3, 5) and np.isfinite(t0).all() and t0[:, 0].min() > 0
    for total, terms in ((total1, terms1), (total2, terms2)):
        assert np.array_equal(terms.cpu().numpy().view(np.uint32), t0.view(np.uint32))
        assert total.dim() == 0 and np.float32(total.item()).view(np.uint32) == np.float32(total0.item()).view(np.uint32)
    from_numpy = preprocess_true_boxes_device(boxes, hw, ANCHORS, c, 3, device=dev)
    from_tensor = preprocess_true_boxes_device(torch.from_numpy(boxes).to(dev), hw, ANCHORS, c, 3)
    assert isinstance(from_numpy, tuple) and isinstance(from_tensor, tuple) and len(from_numpy) == 3
    same_bytes([y.cpu().numpy() for y in from_numpy], y_trues, 'NumPy boxes')
    same_bytes([y.cpu().numpy() for y in from_tensor], y_trues, 'device boxes')
    one = preprocess_true_boxes_device(boxes, hw, ANCHORS, c, 1, device=dev)       # one scale: a tensor, as the host function
    assert isinstance(one, torch.Tensor)
    same_bytes([one.cpu().numpy()], host_labels(boxes, hw, c, 1), 'one scale')


# ----------------------------------------------------------------------------- error paths
def test_error_paths_leave_the_outputs_untouched(dev):
    rt = _rt()
    tb = torch.from_numpy(random_boxes(11, 2, 4, (96, 96), 20)).to(dev)
    ys = [torch.full(shp, float('nan'), dtype=torch.float32, device=dev) for shp in rt.label_shapes(2, (96, 96), 20, 3)]
    skipped = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)
    an = np.ascontiguousarray(ANCHORS, np.float32)
    ok = dict(boxes=rt._ptr(tb), batch=2, t=4, in_h=96, in_w=96, anchors=an.ctypes.data, c=20, s=3, y1=rt._ptr(ys[0]), y2=rt._ptr(ys[1]),
              y3=rt._ptr(ys[2]))
    cases = [('null', dict(boxes=None)), ('null', dict(anchors=None)), ('output 1', dict(y1=None)), ('output 3', dict(y3=None)),
             ('batch', dict(batch=0)), ('batch', dict(batch=-1)), ('max_boxes', dict(t=0)), ('max_boxes', dict(t=257)),
             ('num_scales', dict(s=0)), ('num_scales', dict(s=4)), ('num_classes', dict(c=-1)),
             ('multiples of 32', dict(in_h=100)), ('multiples of 32', dict(in_w=100)), ('multiples of 32', dict(in_h=0)),
             ('multiples of 32', dict(in_w=-32)), ('2\\^31', dict(c=5 * 10 ** 6))]
    for word, change in cases:
        a = dict(ok, **change)
        with torch.cuda.device(dev), pytest.raises(rt.YoloretHipError, match=word):
            rt.check(rt.lib().yr_encode_labels(a['boxes'], a['batch'], a['t'], a['in_h'], a['in_w'], a['anchors'], a['c'], a['s'], a['y1'], a['y2'],
                                               a['y3'], rt._ptr(skipped), rt.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(y).all()) for y in ys) and skipped.tolist() == [SENTINEL] * 2
    # the wrapper's own checks of tensors that live on the device
    with pytest.raises(ValueError, match='out tensors'):
        rt.encode_labels(tb, (96, 96), ANCHORS, 20, 3, out=ys[:2])
    with pytest.raises(ValueError, match='out tensors'):
        rt.encode_labels(tb, (96, 96), ANCHORS, 20, 3, out=[ys[0], ys[1], ys[2][:, :11]])
    with pytest.raises(ValueError, match='skipped'):
        rt.encode_labels(tb, (96, 96), ANCHORS, 20, 3, skipped=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match='contiguous'):
        rt.encode_labels(tb[:, ::2], (96, 96), ANCHORS, 20, 3)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(y).all()) for y in ys)
