"""yr_voc_match (yoloret_amd/csrc/vocmatch.hip) against tests/map_ref.py: known answers and random cases, every call through the C
entry with all six buffers between the guards of tests/fence.py (both alignments), outputs pre-filled with a sentinel.  Every
comparison is exact: no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from tests import fence, map_ref as R
from tests.test_map import _scenario

pytestmark = pytest.mark.gpu

SENTINEL = -99


def _rt():
    from yoloret_amd import runtime as rt
    return rt


def _entry(dev, det, det_count, gt, gt_count, num_classes, iou, flags, npos, batch=None, rows=None, max_gt=None, moved=lambda t: t,
           null_flags=False):
    """the raw return code of yr_voc_match"""
    rt = _rt()
    p = lambda t: rt._ptr(moved(t)) if t is not None else None
    with torch.cuda.device(dev):
        return rt.lib().yr_voc_match(p(det), p(det_count), det.shape[0] if batch is None else batch, det.shape[1] if rows is None else rows,
                                     num_classes, p(gt), p(gt_count), (gt.shape[1] if gt is not None else 0) if max_gt is None else max_gt,
                                     float(iou), None if null_flags else p(flags), p(npos), rt.stream_ptr(dev))


def match(dev, det, det_count, gt, gt_count, num_classes, iou=.5):
    """NumPy in, NumPy out; gt=None: max_gt = 0 with a null pointer."""
    rt = _rt()
    d, dc, gc = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (det, det_count, gt_count))
    g = torch.from_numpy(np.ascontiguousarray(gt)).to(dev) if gt is not None else None
    flags = torch.full(det.shape[:2], SENTINEL, dtype=torch.int32, device=dev)
    npos = torch.full((det.shape[0], num_classes), SENTINEL, dtype=torch.int32, device=dev)

    def call(moved):
        rt.check(_entry(dev, d, dc, g, gc, num_classes, iou, flags, npos, moved=moved))
    fence.run(call, writes=[flags, npos], reads=[d, dc, g, gc], batch=det.shape[0])
    return flags.cpu().numpy(), npos.cpu().numpy()


def one_image(dets, boxes, num_classes, iou=.5, dev=None, rows=None):
    """dets: (left, top, right, bottom, score, class) rows, boxes: (xmin, ymin, xmax, ymax, label) rows -> flags of the rows, npos"""
    det, dc = R.make_det([[(t, l, b, r, s, c) for l, t, r, b, s, c in dets]], rows or max(len(dets), 1))
    gt, gc = R.make_gt([boxes])
    flags, npos = match(dev, det, dc, gt, gc, num_classes, iou)
    want = R.reference_flags(det, dc, gt, gc, num_classes, iou)
    assert np.array_equal(flags, want[0]) and np.array_equal(npos, want[1])
    return flags[0, :len(dets)].tolist(), npos[0].tolist()


# ----------------------------------------------------------------------------- known answers
def test_hand_example(dev):
    pred, true_res = _scenario()
    rows = [[(p[4], p[3], p[6], p[5], p[2], p[1]) for p in pred if p[0] == b] for b in range(2)]
    det, dc = R.make_det(rows, 6)
    gt, gc = R.make_gt([true_res[b] for b in range(2)])
    flags, npos = match(dev, det, dc, gt, gc, 4)
    assert flags.tolist() == [[1, 0, -1, -1, -1, -1], [1, 0, 0, -1, -1, -1]]       # 1, 1, 0, 0, 0 in the order of _scenario
    assert npos.tolist() == [[1, 0, 0, 0], [2, 1, 0, 0]]


def test_iou_of_exactly_one_half_is_no_match(dev):
    box = [(0, 0, 9, 9, 0)]
    assert one_image([(0, 0, 9, 19, .9, 0)], box, 1, dev=dev)[0] == [0]         # 10x10 inside 10x20: 100 / 200
    assert one_image([(0, 0, 9, 19, .9, 0)], box, 1, iou=.4999, dev=dev)[0] == [1]
    assert one_image([(0, 0, 9, 9, .9, 0)], box, 1, iou=.9999, dev=dev)[0] == [1]   # the identical box: IoU exactly 1


def test_higher_score_claims_first_in_both_row_orders(dev):
    box = [(0, 0, 9, 9, 0)]
    exact, shifted = (0, 0, 9, 9, .3, 0), (1, 0, 10, 9, .9, 0)
    assert one_image([exact, shifted], box, 1, dev=dev)[0] == [0, 1]
    assert one_image([shifted, exact], box, 1, dev=dev)[0] == [1, 0]


def test_equal_scores_lower_row_wins(dev):
    box = [(0, 0, 9, 9, 0)]
    exact, shifted = (0, 0, 9, 9, .5, 0), (1, 0, 10, 9, .5, 0)
    assert one_image([exact, shifted], box, 1, dev=dev)[0] == [1, 0]
    assert one_image([shifted, exact], box, 1, dev=dev)[0] == [1, 0]
    # -0.0 and +0.0 are one score value: row order decides
    assert one_image([(0, 0, 9, 9, -0.0, 0), (1, 0, 10, 9, 0.0, 0)], box, 1, dev=dev)[0] == [1, 0]
    assert one_image([(0, 0, 9, 9, 0.0, 0), (1, 0, 10, 9, -0.0, 0)], box, 1, dev=dev)[0] == [1, 0]
    # negative scores order like any other value
    assert one_image([(0, 0, 9, 9, -.5, 0), (1, 0, 10, 9, -.25, 0)], box, 1, dev=dev)[0] == [0, 1]


def test_duplicate_ground_truth_is_not_best_unclaimed(dev):
    """two identical boxes, two identical detections: the second detection's argmax is index 0 again, which is taken"""
    boxes = [(20, 30, 60, 90, 0), (20, 30, 60, 90, 0)]
    assert one_image([(20, 30, 60, 90, .9, 0), (20, 30, 60, 90, .8, 0)], boxes, 1, dev=dev) == ([1, 0], [2])


def test_argmax_tie_across_a_chunk_goes_to_the_lowest_index(dev):
    """ground-truth rows 3 and 100 (two 64-row chunks) overlap the first detection equally: it must take row 3, so the detection
    that fits row 100 alone is still a true positive and the one that fits row 3 alone is not"""
    boxes = [(1000 + 40 * i, 1000, 1000 + 40 * i + 20, 1020, i % 2) for i in range(104)]      # far away, both classes
    boxes[3] = (98, 100, 138, 160, 0)         # the centre box shifted 2 px left
    boxes[100] = (102, 100, 142, 160, 0)      # ... and 2 px right
    dets = [(100, 100, 140, 160, .9, 0), (102, 100, 142, 160, .8, 0), (98, 100, 138, 160, .7, 0)]
    ov = R._iou(np.asarray(boxes, np.float64)[:, :4], (100., 100., 140., 160.))
    assert ov[3] == ov[100] == ov.max() and ov[3] > .5
    assert one_image(dets, boxes, 2, dev=dev)[0] == [1, 1, 0]


@pytest.mark.parametrize('box,det', [((10.25, 20.5, 70.75, 90.125, 0), (12, 22, 71, 88)),
                                     ((3.0625, 4.9375, 40.5, 33.3125, 0), (1, 2, 38, 35)),
                                     ((100.1, 50.7, 180.3, 121.9, 0), (95, 55, 170, 130))])
def test_threshold_on_the_last_bit(dev, box, det):
    """float64 IoU in the host's operation order: iou_thr = ov is no match (strict), one ulp below is one"""
    ov = float(R._iou(np.asarray([box], np.float32).astype(np.float64)[:, :4], tuple(float(v) for v in det))[0])
    assert .3 < ov < 1
    assert one_image([det + (.9, 0)], [box], 1, iou=ov, dev=dev)[0] == [0]
    assert one_image([det + (.9, 0)], [box], 1, iou=float(np.nextafter(ov, 0)), dev=dev)[0] == [1]


def test_empty_combinations(dev):
    dets = [(0, 0, 9, 9, .9, 0), (0, 0, 9, 9, .8, 1)]
    boxes = [(0, 0, 9, 9, 0), (0, 0, 9, 9, 1), (5, 5, 9, 9, 1)]
    assert one_image([], boxes, 2, dev=dev, rows=3) == ([], [1, 2])                     # det_count = 0
    assert one_image(dets, [], 2, dev=dev) == ([0, 0], [0, 0])                          # gt_count = 0
    assert one_image([], [], 2, dev=dev, rows=2) == ([], [0, 0])                        # both
    det, dc = R.make_det([[(0, 0, 9, 9, .9, 0)], []], 2)
    flags, npos = match(dev, det, dc, None, np.zeros(2, np.int32), 3)                   # max_gt = 0, null gt
    assert flags.tolist() == [[0, -1], [-1, -1]] and npos.tolist() == [[0, 0, 0], [0, 0, 0]]


def test_rows_with_a_class_out_of_range_and_labels_out_of_range(dev):
    dets = [(0, 0, 9, 9, .9, -1), (0, 0, 9, 9, .8, 2), (0, 0, 9, 9, .7, 1), (0, 0, 9, 9, .6, 1)]
    boxes = [(0, 0, 9, 9, -1), (0, 0, 9, 9, 2), (0, 0, 9, 9, 1.5), (0, 0, 9, 9, 1), (0, 0, 9, 9, .5)]
    assert one_image(dets, boxes, 2, dev=dev) == ([-1, -1, 1, 0], [0, 1])


# ----------------------------------------------------------------------------- random cases
@functools.lru_cache(maxsize=None)
def _case(case):
    return R.random_case(*case)


@functools.lru_cache(maxsize=None)
def _want(case, iou):
    return R.reference_flags(*_case(case), case[1], iou)


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: 'B%d-C%d-m%d-g%d' % c[:4])
@pytest.mark.parametrize('iou', R.IOUS)
def test_random_cases(dev, case, iou):
    from yoloret_amd.yolo3 import map as M
    det, dc, gt, gc = _case(case)
    flags, npos = match(dev, det, dc, gt, gc, case[1], iou)
    want_flags, want_npos = _want(case, iou)
    assert np.array_equal(npos, want_npos)
    assert np.array_equal(flags, want_flags), np.argwhere(flags != want_flags)[:10]
    ev = M.DeviceEvaluator(case[1], iou)
    half = case[0] // 2          # two batches: images count in the order added
    for lo, hi in ((0, half), (half, case[0])):
        ev.add(torch.from_numpy(det[lo:hi]).to(dev), torch.from_numpy(dc[lo:hi]).to(dev), [gt[b, :gc[b]] for b in range(lo, hi)])
    pred, true_res = R.to_host_inputs(det, dc, gt, gc)
    want = M.evaluate_detections(pred, true_res, case[1], iou)
    got = ev.result()
    assert set(got) == set(want) and all(got[c] == want[c] and type(got[c]) is type(want[c]) for c in want), (got, want)


def test_same_bytes_twice_and_whatever_lies_beyond_the_counts(dev):
    case = R.CASES[1]
    det, dc, gt, gc = (a.copy() for a in _case(case))
    first = match(dev, det, dc, gt, gc, case[1])
    again = match(dev, det, dc, gt, gc, case[1])
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    rng = np.random.RandomState(9)
    for b in range(case[0]):          # other garbage: class words in range, huge coordinates, labels in range, infinities
        n, g = int(dc[b]), int(gc[b])
        det[b, n:] = rng.randint(-2 ** 31, 2 ** 31 - 1, det[b, n:].shape, dtype=np.int64).astype(np.int32)
        det[b, n:, 5] = rng.randint(0, case[1], det[b, n:, 5].shape)
        gt[b, g:] = np.where(rng.rand(*gt[b, g:].shape) < .5, np.inf, 1.0).astype(np.float32)
    assert any(int(dc[b]) < det.shape[1] for b in range(case[0])) and any(int(gc[b]) < gt.shape[1] for b in range(case[0]))
    other = match(dev, det, dc, gt, gc, case[1])
    assert first[0].tobytes() == other[0].tobytes() and first[1].tobytes() == other[1].tobytes()


def test_bad_arguments_launch_nothing(dev):
    rt = _rt()
    flags = torch.full((1, rt.VOC_MAX_ROWS + 1), SENTINEL, dtype=torch.int32, device=dev)
    npos = torch.full((1, 2), SENTINEL, dtype=torch.int32, device=dev)
    det = torch.zeros((1, rt.VOC_MAX_ROWS + 1, 6), dtype=torch.int32, device=dev)
    gt = torch.zeros((1, rt.VOC_MAX_GT + 1, 5), dtype=torch.float32, device=dev)
    cnt = torch.ones((1,), dtype=torch.int32, device=dev)
    for kwargs in (dict(rows=rt.VOC_MAX_ROWS + 1, max_gt=1), dict(rows=1, max_gt=rt.VOC_MAX_GT + 1), dict(rows=1, max_gt=1, batch=0),
                   dict(rows=1, max_gt=1, null_flags=True)):
        rc = _entry(dev, det, cnt, gt, cnt, 2, .5, flags, npos, **kwargs)
        msg = rt.lib().yr_last_error().decode()
        assert rc != 0 and 'voc_match' in msg, (kwargs, rc, msg)
        with pytest.raises(rt.YoloretHipError, match='voc_match'):
            rt.check(rc)
    torch.cuda.synchronize()
    assert bool((flags == SENTINEL).all()) and bool((npos == SENTINEL).all())
    # the binding refuses what it can see, with the shapes in the message
    with pytest.raises(ValueError, match=r'\(1, %d, 6\)' % (rt.VOC_MAX_ROWS + 1)):
        rt.voc_match(det, cnt, gt[:, :1].contiguous(), cnt, 2)
    with pytest.raises(ValueError, match=r'\(1, %d, 5\)' % (rt.VOC_MAX_GT + 1)):
        rt.voc_match(det[:, :4].contiguous(), cnt, gt, cnt, 2)
    with pytest.raises(ValueError):
        rt.voc_match(det[:, :4].contiguous().cpu(), cnt, gt[:, :1].contiguous(), cnt, 2)


def test_at_the_limits(dev):
    """rows = YR_VOC_MAX_ROWS and max_gt = YR_VOC_MAX_GT, one image: the rows of a 150-row random case (the other 3946 carry a class
    out of range, inside det_count) lie scattered over the whole image"""
    rt = _rt()
    num_classes = 3
    sdet, sdc, sgt, sgc = R.random_case(1, num_classes, 50, rt.VOC_MAX_GT, False, 7)
    rng = np.random.RandomState(7)
    det = np.zeros((1, rt.VOC_MAX_ROWS, 6), np.int32)
    det[0, :, 0:2] = rng.randint(0, 300, (rt.VOC_MAX_ROWS, 2))
    det[0, :, 2:4] = det[0, :, 0:2] + rng.randint(0, 90, (rt.VOC_MAX_ROWS, 2))
    det[0, :, 4] = (rng.randint(1, 9, rt.VOC_MAX_ROWS) / 8.0).astype(np.float32).view(np.int32)
    det[0, :, 5] = np.where(rng.rand(rt.VOC_MAX_ROWS) < .5, -1, num_classes)
    at = np.sort(rng.choice(rt.VOC_MAX_ROWS, int(sdc[0]), replace=False))
    at[-1] = rt.VOC_MAX_ROWS - 1
    det[0, at] = sdet[0, :sdc[0]]
    dc = np.array([rt.VOC_MAX_ROWS], np.int32)
    assert sgc[0] == rt.VOC_MAX_GT and sdc[0] == 150
    want_flags, want_npos = R.reference_flags(det, dc, sgt, sgc, num_classes, .5)
    in_range = int(((sdet[0, :150, 5] >= 0) & (sdet[0, :150, 5] < num_classes)).sum())
    assert (want_flags == 1).sum() >= 5 and (want_flags >= 0).sum() == in_range >= 100
    flags, npos = match(dev, det, dc, sgt, sgc, num_classes, .5)
    assert np.array_equal(npos, want_npos) and np.array_equal(flags, want_flags)
