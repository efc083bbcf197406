"""Host side of the loss forward (no GPU): the hand-derived answers that pin tests/loss_ref.py, the label encoder
``preprocess_true_boxes``, and the public surface (BOX_LOSS, YoloLoss, the C-ABI entry)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import loss_ref
from tests.util import ANCHORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = float(np.log(2.0))
C = 20


def _zero_case(batch):
    return np.zeros((batch, 13, 13, 3, 5 + C), np.float32), np.zeros((batch, 13, 13, 3, 5 + C), np.float32)


def _one_box(y_true, image):
    y_true[image, 6, 6, 0, :5] = (6.5 / 13, 6.5 / 13, 116 / 416, 90 / 416, 1)
    y_true[image, 6, 6, 0, 5 + 3] = 1


def _ref(y_true, logits, dtype=np.float64):
    return loss_ref.yolo_loss(y_true, logits, loss_ref.scale_anchors(ANCHORS, 0), 32, .5, dtype)


# ----------------------------------------------------------------------------- known answers (scale 0, input 416, all logits 0)
@pytest.mark.parametrize('dtype,rel', [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_known_answer_no_labelled_box(dtype, rel):
    logits, y_true = _zero_case(1)
    r = _ref(y_true, logits, dtype)
    assert r['giou'] == 0 and r['cls'] == 0
    assert r['conf'] == pytest.approx(507 * LN2, rel=rel) and abs(r['conf'] - 351.425621) < 1e-4
    assert r['ignore_sum'] == 507            # the maximum over no box is below every threshold
    assert r['loss'] == pytest.approx(507 * LN2, rel=rel)


@pytest.mark.parametrize('dtype,rel', [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_known_answer_one_box_and_its_neighbours(dtype, rel):
    logits, y_true = _zero_case(1)
    _one_box(y_true, 0)
    r = _ref(y_true, logits, dtype)
    best = r['best_iou'][0]
    assert best[6, 6, 0] == pytest.approx(1.0, abs=1e-6)
    side = 84 * 90 / (2 * 116 * 90 - 84 * 90)          # the horizontal neighbours overlap 84 of 116 pixels
    assert best[6, 5, 0] == pytest.approx(side, abs=1e-6) and best[6, 7, 0] == pytest.approx(side, abs=1e-6) and side >= .5
    assert best[5, 6, 0] == pytest.approx(0.4754, abs=1e-4) and best[7, 6, 0] == pytest.approx(0.4754, abs=1e-4)
    assert r['ignore_sum'] == 504
    assert r['conf'] == pytest.approx(505 * LN2, rel=rel) and abs(r['conf'] - 350.039326) < 1e-4
    assert r['cls'] == pytest.approx(20 * LN2, rel=rel) and abs(r['cls'] - 13.862944) < 1e-5
    assert abs(r['giou']) <= 1e-6


@pytest.mark.parametrize('dtype,rel', [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_known_answer_batch_wide_gather(dtype, rel):
    """The box of image 1 also removes the three cells of image 0 from the confidence term (model.py:643)."""
    logits, y_true = _zero_case(2)
    _one_box(y_true, 1)
    r = _ref(y_true, logits, dtype)
    assert r['ignore_sum'] == 1008
    assert r['conf'] == pytest.approx(1009 * LN2 / 2, rel=rel) and abs(r['conf'] - 349.692753) < 1e-4
    assert r['cls'] == pytest.approx(10 * LN2, rel=rel)
    assert np.array_equal(r['best_iou'][0], r['best_iou'][1])


def _giou_impls():
    from yoloret_amd.yolo3.utils import do_giou_calculate
    return [loss_ref.giou, do_giou_calculate]


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_known_answer_giou(which, dtype):
    f = _giou_impls()[which]
    sq = lambda y, x: np.array([y, x, y + 1, x + 1], dtype)
    assert f(sq(0, 0), sq(0, 1), mode='iou') == 0 and f(sq(0, 0), sq(0, 1)) == 0          # side by side
    assert f(sq(0, 0), sq(0, 2), mode='iou') == 0
    assert f(sq(0, 0), sq(0, 2)) == pytest.approx(-1 / 3, rel=1e-6)                      # a unit apart
    assert f(sq(0, 0), sq(0, 0)) == 1
    z = np.zeros(4, dtype)
    assert f(z, z, mode='iou') == 0 and f(z, z) == 0                                     # divide_no_nan
    assert f(sq(0, 0), sq(0, 2)).dtype == dtype
    # broadcasting: [2,1,4] against [3,4]
    a = np.stack([sq(0, 0), sq(0, 1)])[:, None, :]
    b = np.stack([sq(0, 0), sq(0, 1), sq(0, 2)])
    assert np.allclose(f(a, b, mode='iou'), [[1, 0, 0], [0, 1, 0]])


def test_reference_head_for_the_loss():
    rs = np.random.RandomState(0)
    feats = rs.randn(2, 2, 3, 3, 7)
    an = loss_ref.scale_anchors(ANCHORS, 1)
    grid, xy, wh, conf = loss_ref.yolo_head(feats, an, (64, 96))
    assert grid.shape == (2, 3, 1, 2) and all(tuple(grid[j, i, 0]) == (i, j) for j in range(2) for i in range(3))
    sig = lambda v: 1 / (1 + np.exp(-v))
    assert xy[1, 1, 2, 0, 0] == pytest.approx((sig(feats[1, 1, 2, 0, 0]) + 2) / 3)
    assert xy[1, 1, 2, 0, 1] == pytest.approx((sig(feats[1, 1, 2, 0, 1]) + 1) / 2)
    assert wh[0, 0, 1, 2, 0] == pytest.approx(np.exp(feats[0, 0, 1, 2, 2]) * an[2, 0] / 96)
    assert wh[0, 0, 1, 2, 1] == pytest.approx(np.exp(feats[0, 0, 1, 2, 3]) * an[2, 1] / 64)
    assert conf.shape == (2, 2, 3, 3, 1)


# ----------------------------------------------------------------------------- the parity recipe meets the GPU tests' condition
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_recipe_keeps_clear_of_the_threshold(seed):
    case = loss_ref.random_case(seed, 3, (416, 416), C, ANCHORS)
    for s, (logits, y_true) in case.items():
        r = loss_ref.yolo_loss(y_true, logits, loss_ref.scale_anchors(ANCHORS, s), loss_ref.GRID_STEPS[s])
        assert loss_ref.threshold_margin(r) > 1e-5
        ignored = r['best_iou'].size - r['ignore_sum']
        assert ignored >= 5, 'the ignore branch is not exercised (scale %d: %d)' % (s, ignored)


# ----------------------------------------------------------------------------- preprocess_true_boxes
def _pre(boxes, num_scales=3, hw=(416, 416)):
    from yoloret_amd.yolo3.utils import preprocess_true_boxes
    return preprocess_true_boxes(np.asarray(boxes, np.float32).reshape(-1, 5), hw, ANCHORS, C, num_scales)


def _box(cx, cy, w, h, cls):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cls]


def test_preprocess_places_a_box_by_its_best_anchor():
    y = _pre([_box(208, 208, 116, 90, 3)])
    assert [a.shape for a in y] == [(13, 13, 3, 25), (26, 26, 3, 25), (52, 52, 3, 25)] and all(a.dtype == np.float32 for a in y)
    row = y[0][6, 6, 0]
    assert np.allclose(row[:5], [208 / 416, 208 / 416, 116 / 416, 90 / 416, 1], atol=1e-7)
    assert row[5 + 3] == 1 and row[5:].sum() == 1
    assert np.count_nonzero(y[0]) == 6 and not y[1].any() and not y[2].any()
    # 30x61 is anchor 3: scale 1, slot 0; 10x13 is anchor 0: scale 2, slot 0
    y = _pre([_box(100, 300, 30, 61, 0), _box(11, 401, 10, 13, 19)])
    assert not y[0].any()
    assert y[1][300 // 16, 100 // 16, 0, 4] == 1 and y[1][300 // 16, 100 // 16, 0, 5] == 1 and np.count_nonzero(y[1][..., 4]) == 1
    assert y[2][401 // 8, 11 // 8, 0, 4] == 1 and y[2][401 // 8, 11 // 8, 0, 5 + 19] == 1 and np.count_nonzero(y[2][..., 4]) == 1


def test_preprocess_quirks_of_the_reference():
    # zero-width padding rows (trailing, as the reference pads) are skipped
    y = _pre([_box(208, 208, 116, 90, 3), [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
    assert sum(np.count_nonzero(a[..., 4]) for a in y) == 1
    # two boxes in one cell and slot: the later box stays, the class bits of both remain
    y = _pre([_box(200, 200, 116, 90, 3), _box(210, 210, 120, 92, 7)])
    row = y[0][6, 6, 0]
    assert np.allclose(row[:4], [210 / 416, 210 / 416, 120 / 416, 92 / 416], atol=1e-7) and np.count_nonzero(y[0][..., 4]) == 1
    assert row[5 + 3] == 1 and row[5 + 7] == 1
    # centres come from a floor division: (101 + 204) // 2 = 152, not 152.5
    y = _pre([[101, 100, 204, 190, 1]])
    assert y[0][145 // 32, 152 // 32, 0, 0] == np.float32(152 / 416) and y[0][145 // 32, 152 // 32, 0, 2] == np.float32(103 / 416)
    # num_scales = 1 returns one array, and only the anchors of that scale are placed
    y = _pre([_box(208, 208, 116, 90, 3), _box(11, 401, 10, 13, 19)], num_scales=1)
    assert isinstance(y, np.ndarray) and y.shape == (13, 13, 3, 25) and np.count_nonzero(y[..., 4]) == 1
    # a non-square input: x scales with the width, y with the height
    y = _pre([_box(80, 40, 116, 90, 2)], hw=(64, 96))
    assert y[0].shape == (2, 3, 3, 25) and y[0][1, 2, 0, 4] == 1
    assert np.allclose(y[0][1, 2, 0, :4], [80 / 96, 40 / 64, 116 / 96, 90 / 64], atol=1e-7)


def test_preprocessed_labels_feed_the_loss():
    y = _pre([_box(208, 208, 116, 90, 3)])
    logits = np.zeros((1, 13, 13, 3, 25), np.float32)
    r = _ref(y[0][None], logits)
    assert r['ignore_sum'] == 504 and r['cls'] == pytest.approx(20 * LN2, rel=1e-12)


# ----------------------------------------------------------------------------- public surface
def test_box_loss_enum_and_mse_branch():
    from yoloret_amd.yolo3.enums import BOX_LOSS
    from yoloret_amd.yolo3.model import YoloLoss
    assert BOX_LOSS.MSE.value == 0 and BOX_LOSS.GIOU.value == 1
    with pytest.raises(NotImplementedError):
        YoloLoss(0, ANCHORS, 3, box_loss=BOX_LOSS.MSE)
    layer = YoloLoss(1, ANCHORS, 3)
    assert layer.grid_step == 16 and layer.ignore_thresh == .5 and layer.print_loss is True and layer.box_loss == BOX_LOSS.GIOU
    assert np.array_equal(layer.anchor, np.asarray(ANCHORS, np.float32).reshape(-1, 2)[3:6])
    assert np.array_equal(YoloLoss(0, ANCHORS, 1).anchor, np.asarray(ANCHORS, np.float32).reshape(-1, 2)[0:3])
    assert YoloLoss(0, ANCHORS, 1).grid_step == 32


def test_c_abi_declares_and_exports_the_loss():
    from yoloret_amd import build, runtime as rt
    header = open(os.path.join(ROOT, 'include', 'yoloret_hip.h')).read()
    assert re.search(r'\bint\s+yr_yolo_loss\s*\(', header) and re.search(r'\bsize_t\s+yr_yolo_loss_workspace_bytes\s*\(', header)
    assert 'added under ABI 9' in header
    L = ctypes.CDLL(build.build())
    assert hasattr(L, 'yr_yolo_loss') and hasattr(L, 'yr_yolo_loss_workspace_bytes')
    assert 'yr_yolo_loss' in rt.EXPORTS and 'yr_yolo_loss_workspace_bytes' in rt.EXPORTS and 'loss.hip' in build.SOURCES
    f = L.yr_yolo_loss_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
    total = 64 * 52 * 52 * 3
    assert f(64, 52, 52, 3) >= total * 16 + (total + 255) // 256 * 32      # the box list + one row per workgroup
    assert f(0, 52, 52, 3) == 0 and f(1, 13, 13, 0) == 0
    # argument errors are reported before anything is launched (no device is needed to reach them)
    g = L.yr_yolo_loss
    g.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                                           ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.yr_last_error.restype = ctypes.c_char_p
    an = (ctypes.c_float * 6)(*[1.0] * 6)
    fake = ctypes.c_void_p(4096)
    assert g(None, fake, 1, 13, 13, 3, 20, an, 416, 416, .5, fake, 1 << 20, fake, None) == -1 and b'null' in L.yr_last_error()
    assert g(fake, fake, 1, 13, 13, 0, 20, an, 416, 416, .5, fake, 1 << 20, fake, None) == -1 and b'num_anchors' in L.yr_last_error()
    assert g(fake, fake, 1, 13, 13, 3, 20, an, 416, 416, .5, fake, 64, fake, None) == -1 and b'workspace' in L.yr_last_error()
