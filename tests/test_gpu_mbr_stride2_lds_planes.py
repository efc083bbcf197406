"""The stride-2 split-form instantiations of YR_OP_MBR (csrc/mbr.hip) on the smallest maps that reach every edge of the walk: the
ones that read their projection planes from LDS and keep the finishing wave's partial sums in registers (three waves per SIMD), and
their neighbours of the same launcher.  Against the oracle composition at the bar of test_mbr_split_form; bitwise independent of the
row segments and of the batch."""
import numpy as np
import pytest
import torch

from tests import fence
from tests.test_gpu_mbr import _reference, make_block
from tests.util import assert_close, from_dev, to_dev

pytestmark = pytest.mark.gpu

BLOCKS = [
    # (cin, cexp, cout, nw)
    (16, 96, 24, 2),      # MobileNetV2 x0.75 block_1, two waves per strip: all eight plane fragments of a wave in LDS
    (16, 96, 24, 3),      # ... three waves per strip: two tiles a wave, planes in registers
    (24, 144, 24, 3),     # block_3
    (24, 144, 48, 3),     # block_6: three cout tiles, planes in registers (the LDS of four workgroups would not fit a CU)
    (24, 144, 32, 3),     # MobileNetV2 x1.4 block_1
]
SHAPES = [
    # (h, w, segs)
    (16, 16, 0),      # even size, TF SAME pad 0/1, one strip pair
    (31, 45, 3),      # odd size, pad 1/1; ragged last strip (23 output columns); an odd segment whose last row pair stores its even row only
    (27, 27, 2),      # odd size, two segments
    (30, 44, 0),      # ragged strips, even size
]
SCALES = {'plain': (1.0, 1.0), 'wide': (100.0, 0.01)}     # per image of the batch of 2


def _case(block, h, w, segs, nw=None):
    cin, cexp, cout, bnw = block
    return (h, w, cin, cexp, cout, 2, False, bnw if nw is None else nw, segs)


def _seed(block, h, w):
    return 1000 * (block[0] + block[2]) + 50 * h + w      # (not the waves, not the segments: the same data for every geometry)


def _with_input(rt, op, keep, x, dev, cin):
    """Points the op at input x; returns the tensors the launch reads."""
    xd = to_dev(x, dev)
    op.src[0] = rt.make_src(xd, c=cin)
    return keep[:-1] + [xd]


_refs = {}


def _ref(block, h, w, scale, params):
    """The oracle composition for (shape of the block, map, input scaling), computed once and not written to afterwards."""
    key = (block[:3], h, w, scale)
    if key not in _refs:
        x = params[0] * np.array(SCALES[scale], np.float32).reshape(2, 1, 1, 1)
        r = _reference(x, *params[1:])
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def _run(dev, block, h, w, segs, scale='plain', nw=None):
    from yoloret_amd import runtime as rt
    op, out, params, keep = make_block(_case(block, h, w, segs, nw), dev, seed=_seed(block, h, w), split=True)
    x = params[0] * np.array(SCALES[scale], np.float32).reshape(2, 1, 1, 1)
    reads = _with_input(rt, op, keep, x, dev, block[0])
    fence.run_op(op, 2, writes=[out], reads=reads)
    torch.cuda.synchronize()
    return from_dev(out), params


@pytest.mark.parametrize('scale', list(SCALES))
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d-s%d' % s for s in SHAPES])
@pytest.mark.parametrize('block', BLOCKS, ids=['%d-%d-%d-nw%d' % b for b in BLOCKS])
def test_against_the_oracle(dev, block, shape, scale):
    """5e-5 of the oracle composition (the bar of test_mbr_split_form), also with image 0 scaled by 100 and image 1 by 0.01.  Both
    wave counts of block_1 run on the same data and are held to the same bar (their partial sums are grouped by wave: not equal)."""
    h, w, segs = shape
    got, params = _run(dev, block, h, w, segs, scale)
    err = assert_close(got, _ref(block, h, w, scale, params), 5e-5, 'mbr split, stride 2 %s %s %s' % (block, shape, scale))
    print('max scaled error %.3e' % err)


@pytest.mark.parametrize('shape', SHAPES[1:3], ids=['%dx%d' % s[:2] for s in SHAPES[1:3]])
@pytest.mark.parametrize('block', BLOCKS, ids=['%d-%d-%d-nw%d' % b for b in BLOCKS])
def test_row_segments_do_not_change_a_bit(dev, block, shape):
    """One segment per strip (the library's choice on maps this small), two and three: the same bytes."""
    h, w, _ = shape
    outs = [_run(dev, block, h, w, segs)[0] for segs in (0, 2, 3)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize('block', BLOCKS, ids=['%d-%d-%d-nw%d' % b for b in BLOCKS])
def test_batch_does_not_change_a_bit(dev, block):
    """Image i of a batch of 3 equals the same image run alone, bit for bit."""
    from yoloret_amd import runtime as rt
    h, w, segs = SHAPES[1]
    case = _case(block, h, w, segs)
    op, out, params, keep = make_block(case, dev, b=3, seed=7, split=True)
    fence.run_op(op, 3, writes=[out], reads=keep)
    torch.cuda.synchronize()
    full = from_dev(out).copy()
    for i in range(3):
        op1, out1, _, keep1 = make_block(case, dev, b=3, seed=7, split=True)      # (same seed and batch: the same weights; it runs one image)
        reads = _with_input(rt, op1, keep1, params[0][i:i + 1], dev, block[0])
        fence.run_op(op1, 1, writes=[out1], reads=reads)
        torch.cuda.synchronize()
        assert np.array_equal(from_dev(out1)[0], full[i]), 'image %d' % i
