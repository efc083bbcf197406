"""The label encoder's surface without a GPU (yoloret_amd/csrc/labels.hip behind yr_encode_labels): what is declared, exported
and built, and every argument error that is reported before the device is touched - by the Python wrappers (ValueError) and by
the C entry (YR_ERR_ARG = -1 with a message; nothing is launched, so fake pointers do).  tests/test_gpu_labels.py holds the
parity tests."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.util import ANCHORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_declares_exports_and_builds_the_encoder():
    from yoloret_amd import build, runtime as rt
    header = open(os.path.join(ROOT, 'include', 'yoloret_hip.h')).read()
    assert re.search(r'\bint\s+yr_encode_labels\s*\(', header)
    assert re.search(r'^#define\s+YR_ENC_MAX_BOXES\s+256\b', header, re.M) and rt.ENC_MAX_BOXES == 256
    assert 'yr_encode_labels' in rt.EXPORTS and 'labels.hip' in build.SOURCES
    assert rt.ABI_VERSION == 9 and re.search(r'^#define\s+YR_ABI_VERSION\s+9\b', header, re.M)
    assert hasattr(ctypes.CDLL(build.build()), 'yr_encode_labels')


def test_label_shapes():
    from yoloret_amd import runtime as rt
    assert rt.label_shapes(64, (416, 416), 20, 3) == [(64, 13, 13, 3, 25), (64, 26, 26, 3, 25), (64, 52, 52, 3, 25)]
    assert rt.label_shapes(2, (320, 416), 1, 2) == [(2, 10, 13, 3, 6), (2, 20, 26, 3, 6)]


BAD = [  # (what, true_boxes, input shape, num_scales, a word of the message)
    ('wrong rank', np.zeros((4, 5), np.float32), (96, 96), 3, 'shape'),
    ('wrong last dimension', np.zeros((1, 4, 4), np.float32), (96, 96), 3, 'shape'),
    ('float64', np.zeros((1, 4, 5), np.float64), (96, 96), 3, 'float32'),
    ('T = 0', np.zeros((1, 0, 5), np.float32), (96, 96), 3, 'rows per image'),
    ('T = 257', np.zeros((1, 257, 5), np.float32), (96, 96), 3, 'rows per image'),
    ('num_scales 0', np.zeros((1, 4, 5), np.float32), (96, 96), 0, 'num_scales'),
    ('num_scales 4', np.zeros((1, 4, 5), np.float32), (96, 96), 4, 'num_scales'),
    ('input shape 100', np.zeros((1, 4, 5), np.float32), (100, 100), 3, 'multiples of 32'),
    ('input width 100', np.zeros((1, 4, 5), np.float32), (96, 100), 3, 'multiples of 32'),
    ('CPU tensor', np.zeros((1, 4, 5), np.float32), (96, 96), 3, 'CUDA'),
]


@pytest.mark.parametrize('what,boxes,hw,num_scales,word', BAD, ids=[b[0] for b in BAD])
def test_wrappers_raise_before_the_library_is_touched(what, boxes, hw, num_scales, word, monkeypatch):
    from yoloret_amd import runtime as rt
    from yoloret_amd.yolo3.utils import preprocess_true_boxes_device

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(rt, 'lib', no_library)
    with pytest.raises(ValueError, match=word):
        rt.encode_labels(torch.from_numpy(boxes), hw, ANCHORS, 20, num_scales)
    with pytest.raises(ValueError, match=word):      # a CPU tensor is not copied anywhere: the same errors
        preprocess_true_boxes_device(torch.from_numpy(boxes), hw, ANCHORS, 20, num_scales)
    if what != 'CPU tensor':                         # (a NumPy array would be copied to the device: its checks come first)
        with pytest.raises(ValueError, match=word):
            preprocess_true_boxes_device(boxes, hw, ANCHORS, 20, num_scales)


def test_wrapper_rejects_other_bad_arguments():
    from yoloret_amd import runtime as rt
    t = torch.zeros((1, 4, 5))
    with pytest.raises(ValueError, match='num_classes'):
        rt.encode_labels(t, (96, 96), ANCHORS, -1, 3)
    with pytest.raises(ValueError, match='anchors'):
        rt.encode_labels(t, (96, 96), ANCHORS[:3], 20, 3)
    with pytest.raises(ValueError, match='2\\^31'):
        rt.encode_labels(t, (96, 96), ANCHORS, 5 * 10 ** 6, 3)      # 12 * 12 * 3 * 5e6 elements at stride 8
    with pytest.raises(ValueError, match='float32'):
        rt.encode_labels(np.zeros((1, 4, 5), np.float32), (96, 96), ANCHORS, 20, 3)     # not a tensor


def test_c_entry_reports_argument_errors_before_any_launch():
    from yoloret_amd import build
    L = ctypes.CDLL(build.build())
    L.yr_last_error.restype = ctypes.c_char_p
    g = L.yr_encode_labels
    g.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    an = (ctypes.c_float * 18)(*ANCHORS.reshape(-1).tolist())
    f = ctypes.c_void_p(4096)

    def err(boxes=f, batch=1, t=4, in_h=96, in_w=96, anchors=an, c=20, s=3, y1=f, y2=f, y3=f):
        assert g(boxes, batch, t, in_h, in_w, anchors, c, s, y1, y2, y3, None, None) == -1
        return L.yr_last_error()
    assert b'null' in err(boxes=None) and b'null' in err(anchors=None)
    assert b'output 2' in err(y2=None) and b'output 1' in err(s=1, y1=None, y2=None, y3=None)
    assert b'batch' in err(batch=0) and b'batch' in err(batch=-3)
    assert b'max_boxes' in err(t=0) and b'max_boxes' in err(t=257)
    assert b'num_scales' in err(s=0) and b'num_scales' in err(s=4)
    assert b'num_classes' in err(c=-1)
    for hw in ((100, 96), (96, 100), (0, 96), (96, -32), (16, 16)):
        assert b'multiples of 32' in err(in_h=hw[0], in_w=hw[1])
    assert b'2^31' in err(c=5 * 10 ** 6)                      # 12 * 12 * 3 * (5 + 5e6) > 2^31 at stride 8
    assert b'2^31' in err(batch=1 << 20, in_h=416, in_w=416)   # the element count does not wrap in 32 bits either
