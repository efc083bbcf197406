"""Host side of the device mAP evaluation (yoloret_amd/yolo3/map.py: pack_ground_truth, aps_from_flags, MAPCallback(on_device=...))
and the reference the GPU tests compare the matcher with (tests/map_ref.py).  Every comparison is exact: no tolerance."""
import os
import re

import numpy as np
import pytest

from tests import map_ref as R
from tests.test_map import _scenario
from yoloret_amd.yolo3 import map as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scenario_as_records(num_classes=4):
    pred, true_res = _scenario()
    rows = [[(p[4], p[3], p[6], p[5], p[2], p[1]) for p in pred if p[0] == b] for b in range(2)]
    det, det_count = R.make_det(rows, 6)
    gt, gt_count = R.make_gt([true_res[b] for b in range(2)])
    return det, det_count, gt, gt_count, pred, true_res


def aps_through_flags(det, det_count, gt, gt_count, num_classes, iou):
    flags, npos = R.reference_flags(det, det_count, gt, gt_count, num_classes, iou)
    valid = flags >= 0
    return M.aps_from_flags(det[:, :, 4].view(np.float32)[valid], det[:, :, 5][valid], flags[valid], npos.sum(axis=0), num_classes)


def same_aps(a, b):
    return set(a) == set(b) and all(a[c] == b[c] and type(a[c]) is type(b[c]) for c in a)


def test_hand_example_flags_and_aps():
    det, det_count, gt, gt_count, pred, true_res = scenario_as_records()
    flags, npos = R.reference_flags(det, det_count, gt, gt_count, 4, .5)
    assert flags[0].tolist() == [1, 0, -1, -1, -1, -1] and flags[1].tolist() == [1, 0, 0, -1, -1, -1]     # rows 1, 1, 0, 0, 0 of _scenario
    assert npos.tolist() == [[1, 0, 0, 0], [2, 1, 0, 0]]
    want = M.evaluate_detections(pred, true_res, 4, .5)
    got = aps_through_flags(det, det_count, gt, gt_count, 4, .5)
    assert same_aps(got, want), (got, want)
    assert got[1] == 0 and isinstance(got[1], int) and got[0] == pytest.approx(2.0 / 3.0)


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: 'B%d-C%d-m%d-g%d-s%d' % (c[0], c[1], c[2], c[3], c[5]))
@pytest.mark.parametrize('iou', R.IOUS)
def test_random_cases_are_worth_running_and_agree_with_the_host_evaluator(case, iou):
    batch, num_classes, max_boxes, max_gt = case[:4]
    det, det_count, gt, gt_count = R.random_case(*case)
    assert det.shape == (batch, num_classes * max_boxes, 6) and gt.shape == (batch, max_gt, 5)
    assert (det[0, det_count[0]:] == R.FILLER_DET).all() and np.isnan(gt[1, gt_count[1]:]).all()
    stats = R.case_statistics(det, det_count, gt, gt_count, num_classes, iou)
    need = R.required_statistics(batch, num_classes, max_gt)
    print(case, iou, stats)
    assert all(stats[k] >= need[k] for k in need), (stats, need)
    pred, true_res = R.to_host_inputs(det, det_count, gt, gt_count)
    assert same_aps(aps_through_flags(det, det_count, gt, gt_count, num_classes, iou), M.evaluate_detections(pred, true_res, num_classes, iou))


def test_row_order_does_not_change_the_reference_aps():
    """flags follow their rows under a permutation that keeps the order of equal scores inside a class"""
    det, det_count, gt, gt_count = R.random_case(*R.CASES[1])
    flags, _ = R.reference_flags(det, det_count, gt, gt_count, 3, .5)
    n = int(det_count[0])
    perm = np.argsort(det[0, :n, 5], kind='stable')          # class-major, otherwise the same order
    det2 = det.copy()
    det2[0, :n] = det[0, :n][perm]
    flags2, _ = R.reference_flags(det2, det_count, gt, gt_count, 3, .5)
    assert np.array_equal(flags2[0, :n], flags[0, :n][perm]) and np.array_equal(flags2[1:], flags[1:])


def test_pack_ground_truth_shapes():
    import torch
    a = np.array([[1, 2, 3, 4, 0], [5, 6, 7, 8, 1]], np.float32)
    gt, cnt = M.pack_ground_truth([a, np.zeros((0, 5), np.float32), a[:1]], 'cpu')
    assert gt.dtype == torch.float32 and cnt.dtype == torch.int32 and tuple(gt.shape) == (3, 2, 5) and cnt.tolist() == [2, 0, 1]
    assert np.array_equal(gt[0].numpy(), a) and np.array_equal(gt[2, 0].numpy(), a[0])
    gt, cnt = M.pack_ground_truth([np.zeros((0, 5), np.float32)] * 2, 'cpu')          # no box at all: G = 1
    assert tuple(gt.shape) == (2, 1, 5) and cnt.tolist() == [0, 0]
    M.pack_ground_truth([np.zeros((M.VOC_MAX_GT, 5), np.float32)], 'cpu')
    with pytest.raises(ValueError, match='%d' % (M.VOC_MAX_GT + 1)):
        M.pack_ground_truth([a, np.zeros((M.VOC_MAX_GT + 1, 5), np.float32)], 'cpu')


def _label_files(tmp_path):
    pred, true_res = _scenario()
    for i in range(2):
        (tmp_path / ('im%d.jpg' % i)).write_bytes(b'image-%d' % i)
    with open(tmp_path / 'test.txt', 'w') as f:
        for i in range(2):
            f.write('im%d.jpg ' % i + ' '.join(str(int(v)) for v in true_res[i].ravel()) + '\n')
    return pred, true_res


class FakeModel:   # the stand-in of tests/test_map.py: no call_packed
    def __init__(self, pred):
        self.pred = pred

    def __call__(self, inputs):
        i = int(inputs[0].decode().split('-')[1])
        rows = [r for r in self.pred if r[0] == i]
        boxes = np.array([[r[4], r[3], r[6], r[5]] for r in rows], np.float32).reshape(-1, 4)
        return boxes, np.array([r[2] for r in rows], np.float32), np.array([r[1] for r in rows], np.int32)


def test_callback_on_device_needs_call_packed_and_the_host_path_is_unchanged(tmp_path):
    pred, true_res = _label_files(tmp_path)
    names = ['a', 'b', 'c', 'd']
    cb = M.MAPCallback(str(tmp_path / '*.txt'), (416, 416), names, root=str(tmp_path), on_device=True, batch_size=2)
    cb.set_model(FakeModel(pred))
    with pytest.raises(TypeError, match='call_packed'):
        cb.calculate_aps()
    want = M.evaluate_detections(pred, true_res, 4, .5)
    for kwargs in ({}, {'on_device': False}):
        cb = M.MAPCallback(str(tmp_path / '*.txt'), (416, 416), names, root=str(tmp_path), **kwargs)
        assert cb.on_device is False
        cb.set_model(FakeModel(pred))
        assert same_aps(cb.calculate_aps(), want) and cb.seconds_per_image >= 0


def test_entry_is_declared_and_exported():
    from yoloret_amd import build, runtime as rt
    header = open(os.path.join(ROOT, 'include', 'yoloret_hip.h')).read()
    assert 'yr_voc_match' in rt.EXPORTS and 'vocmatch.hip' in build.SOURCES
    assert re.search(r'\bint\s+yr_voc_match\s*\(', header)
    assert int(re.search(r'#define YR_VOC_MAX_ROWS\s+(\d+)', header).group(1)) == rt.VOC_MAX_ROWS
    assert int(re.search(r'#define YR_VOC_MAX_GT\s+(\d+)', header).group(1)) == rt.VOC_MAX_GT == M.VOC_MAX_GT
