"""The fence of tests/fence.py fails when it should: run on CPU tensors, with Python functions that play the kernel by writing through
NumPy views at the (relocated) pointers of the op - a clean writer, and one writer per kind of error the fence exists to catch."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import fence
from yoloret_amd import runtime as rt

B, H, W, C, LD = 3, 5, 4, 6, 8       # `out` rows are LD wide, the kernel may write [0, C)
IMG = H * W * LD                     # elements of one image


def _f32(ptr, n, off=0):
    """float32 view of n elements at ptr + off elements (what a kernel sees of its pointer)"""
    buf = (ctypes.c_float * n).from_address(ptr + 4 * off)
    return np.frombuffer(buf, np.float32)


def _setup(residual=False):
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, H, W, LD), generator=g)
    out = torch.full((B, H, W, LD), float('nan'))
    op = rt.new_op(rt.OP_POINTWISE)
    op.h, op.w, op.cin, op.cout, op.nsrc = H, W, C, C, 1
    op.src[0] = rt.make_src(x, c=C)
    op.out, op.out_ld = out.data_ptr(), LD
    if residual:
        op.res, op.res_ld = x.data_ptr(), LD
    return op, x, out


def clean(op, batch):
    """out[..., :C] = 2 * src[..., :C]"""
    s = _f32(op.src[0].ptr, batch * IMG).reshape(-1, LD)
    o = _f32(op.out, batch * IMG).reshape(-1, LD)
    o[:, :C] = 2 * s[:, :C]


def _then(extra):
    def launch(op, batch):
        clean(op, batch)
        extra(op, batch)
    return launch


def _pointers(op):
    return [op.out, op.res, op.gate, op.src[0].ptr]


def test_clean_writer_passes_and_result_comes_back():
    op, x, out = _setup()
    before = _pointers(op)
    seen = []

    def launch(op, batch):
        seen.append((op.out, op.src[0].ptr))
        clean(op, batch)
    fence.run_op(op, B, writes=[out], reads=[x], cols=C, launch=launch)
    assert _pointers(op) == before
    assert [p % 256 for p, _ in seen] == [0, 16] and [p % 256 for _, p in seen] == [0, 16]     # variants A and B
    assert all(p not in before for pair in seen for p in pair)
    assert torch.equal(out[..., :C], 2 * x[..., :C]) and torch.isnan(out[..., C:]).all()


def test_guard_is_at_least_one_image_and_64_kib():
    small = torch.zeros((B, 2, 2, 4))
    big = torch.zeros((2, 100, 100, 8))
    assert fence.guard_bytes(small, B) == 64 << 10
    assert fence.guard_bytes(big, 2) == 100 * 100 * 8 * 4 and fence.guard_bytes(big, 2) % 256 == 0
    assert fence.guard_bytes(torch.zeros((2, 9, 9, 1001)), 2) % 256 == 0
    assert fence.guard_bytes(torch.zeros(3, dtype=torch.int32)) == 64 << 10


BAD_WRITERS = [
    # (name, what the kernel does after the clean pass, words the failure must carry)
    ('one element past the end', lambda op, b: _f32(op.out, 1, b * IMG).fill(0.0),
     [r'written tensor writes\[0\] \(out\)', 'guard after', r'bytes \+%d \.\. \+%d ' % (4 * B * IMG, 4 * B * IMG + 3)]),
    ('one element before the start', lambda op, b: _f32(op.out, 1, -1).fill(np.nan),
     [r'written tensor writes\[0\] \(out\)', 'guard before', r'bytes -4 \.\. -1 ']),
    ('one whole image past the end', lambda op, b: _f32(op.out, IMG, b * IMG).fill(1.0),
     [r'written tensor writes\[0\] \(out\)', 'guard after', r'bytes \+%d \.\. \+%d ' % (4 * B * IMG, 4 * (B + 1) * IMG - 1)]),
    ('a write into the cols gap', lambda op, b: _f32(op.out, 1, 2 * LD + C).fill(1.2345),
     [r'written tensor writes\[0\] \(out\)', 'columns >= %d' % C, r'bytes \+%d \.\. \+%d ' % (4 * (2 * LD + C), 4 * (2 * LD + C) + 3)]),
    ('a result that depends on a byte of a source guard',
     lambda op, b: _f32(op.out, 1, 0).__setitem__(0, float(_f32(op.src[0].ptr, 1, b * IMG).view(np.uint8)[0])),
     [r'written tensor writes\[0\] \(out\)', 'variant A .* and variant B .* differ', r'bytes \+[0-3] \.\. \+3 ']),      # 255.0 against 123.0
    ('a write into a read tensor\'s guard', lambda op, b: _f32(op.src[0].ptr, 1, b * IMG).fill(0.0),
     [r'read tensor reads\[0\] \(src\[0\]\)', 'guard after', r'bytes \+%d \.\. \+%d ' % (4 * B * IMG, 4 * B * IMG + 3)]),
]


@pytest.mark.parametrize('name,extra,words', BAD_WRITERS, ids=[b[0] for b in BAD_WRITERS])
def test_bad_writer_is_caught(name, extra, words):
    op, x, out = _setup()
    before = _pointers(op)
    with pytest.raises(fence.FenceError) as e:
        fence.run_op(op, B, writes=[out], reads=[x], cols=C, launch=_then(extra))
    for wd in words:
        assert re.search(wd, str(e.value)), (wd, str(e.value))
    assert _pointers(op) == before
    assert torch.isnan(out).all()          # a failed launch hands nothing back


def test_a_constant_store_shows_in_a_written_guard():
    """The guards of written tensors are random bytes: a stray store of the byte 0x00, 0xFF or 0x7B cannot hide in them."""
    for byte in (0x00, 0xFF, 0x7B):
        op, x, out = _setup()

        def stray(op, b, byte=byte):
            _f32(op.out, 64, b * IMG).view(np.uint8)[:] = byte
        with pytest.raises(fence.FenceError, match='guard after'):
            fence.run_op(op, B, writes=[out], reads=[x], launch=_then(stray))


def test_aliased_fields_move_together():
    """An MBR residual is the block's input: op.res == op.src[0].ptr before, during and after."""
    op, x, out = _setup(residual=True)
    seen = []

    def launch(op, batch):
        seen.append((op.res, op.src[0].ptr, op.out))
        clean(op, batch)
    fence.run_op(op, B, writes=[out], reads=[x], launch=launch)
    assert len(seen) == 2 and all(r == s and r != x.data_ptr() and o != r for r, s, o in seen)
    assert op.res == op.src[0].ptr == x.data_ptr()


def test_a_pointer_inside_a_tensor_keeps_its_offset():
    op, x, out = _setup()
    op.gate = out.data_ptr() + 4 * IMG          # a second pointer into the same output (image 1)
    seen = []

    def launch(op, batch):
        seen.append(op.gate - op.out)
        clean(op, batch)
    fence.run_op(op, B, writes=[out], reads=[x], launch=launch)
    assert seen == [4 * IMG, 4 * IMG] and op.gate == out.data_ptr() + 4 * IMG


def test_pointers_are_restored_when_the_launch_raises():
    op, x, out = _setup(residual=True)
    before = _pointers(op)

    def launch(op, batch):
        assert op.out != before[0]
        raise rt.YoloretHipError('refused')
    with pytest.raises(rt.YoloretHipError, match='refused'):
        fence.run_op(op, B, writes=[out], reads=[x], launch=launch)
    assert _pointers(op) == before


def test_a_tensor_behind_no_pointer_is_an_error_of_the_test():
    op, x, out = _setup()
    with pytest.raises(ValueError, match='not behind any pointer'):
        fence.run_op(op, B, writes=[out], reads=[x, torch.zeros(4)], launch=clean)


def test_written_interiors_restart_from_the_pre_launch_bytes():
    """An accumulating kernel (+= into its output) gives the same bytes in both variants only if B starts where A started."""
    op, x, out = _setup()
    out.fill_(1.0)

    def launch(op, batch):
        _f32(op.out, batch * IMG)[:] += 1.0
    fence.run_op(op, B, writes=[out], reads=[x], launch=launch)
    assert (out == 2.0).all()


def test_run_with_plain_pointers():
    """fence.run, the form for the entries that take plain pointers: a second written tensor with its own cols."""
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    a = torch.zeros((3, 4))
    n = torch.zeros(1, dtype=torch.int32)

    def call(moved):
        _f32(moved(a).data_ptr(), 12)[:] = _f32(moved(x).data_ptr(), 12) + 1
        np.frombuffer((ctypes.c_int32 * 1).from_address(moved(n).data_ptr()), np.int32)[0] = 7
    fence.run(call, writes=[a, n], reads=[x], batch=3)
    assert torch.equal(a, x + 1) and int(n) == 7

    def bad(moved):
        call(moved)
        np.frombuffer((ctypes.c_int32 * 1).from_address(moved(n).data_ptr() + 4), np.int32)[0] = 7
    with pytest.raises(fence.FenceError, match=r'writes\[1\]: guard after'):
        fence.run(bad, writes=[a, n], reads=[x], batch=3)


def test_scratch_is_guarded_but_not_compared():
    """A workspace may hold different bytes after each launch (here: the pointer it was given); its guards are checked all the same."""
    x = torch.arange(8, dtype=torch.float32)
    a = torch.zeros(8)
    ws = torch.full((64,), 0xFF, dtype=torch.uint8)

    def call(moved, over=0):
        w = np.frombuffer((ctypes.c_uint8 * (64 + over)).from_address(moved(ws).data_ptr()), np.uint8)
        w[:] = moved(ws).data_ptr() % 251
        _f32(moved(a).data_ptr(), 8)[:] = _f32(moved(x).data_ptr(), 8) * 2
    fence.run(call, writes=[a], reads=[x], scratch=[ws])
    assert torch.equal(a, 2 * x) and (ws == 0xFF).all()
    with pytest.raises(fence.FenceError, match='variant A .* and variant B .* differ'):
        fence.run(call, writes=[a, ws], reads=[x])
    with pytest.raises(fence.FenceError, match=r'written tensor writes\[1\]: guard after the tensor: bytes \+64 \.\. \+64 '):
        fence.run(lambda moved: call(moved, over=1), writes=[a], reads=[x], scratch=[ws])
