"""The parts of the loss kernels (yoloret_amd/csrc/loss.hip: yr_yolo_loss, yr_yolo_loss_grad) that tests/test_gpu_loss.py and
tests/test_gpu_lossgrad.py never run, against tests/lossgrad_ref.py (torch-CPU float64, valid at ties of Maximum / Minimum) and
tests/loss_ref.py:
  * the tie rules of the GIoU gradient: all 13 x 13 interval relations of a label to its prediction and zero-size labels, built
    from dyadic numbers so that a tie is a tie in float32, in float64 and on the device; hand-derived answers for five cells;
  * the threshold comparison on its last bit (an IoU of exactly 0.5);
  * lists of labelled boxes of more than one LDS chunk (256): two chunks, three, exactly one (256) and one past it (257);
  * the second phase of the gradient kernel at rows of 5, 256, 257 and 305 floats, totals of 3 and exactly 256 predictions,
    A = 1, 2, 4, 5, 8 anchor slots, and object flags of 0.5.
tests/test_lossgrad_edges_host.py asserts, without a GPU, what these cases depend on.

Bars, those of the sibling files.  Gradient, per channel group (box 0-3, confidence 4, class 5..):
    max |device - ref64| / max |ref64|  <=  4 x (the same quantity of the reference run in float32) + 4 * 2^-24;
structurally zero elements must be exactly 0.  Forward: relative error of each sum <= 4 x (the float32 reference's) + 4 * 2^-24
(the GIoU term on max(|ref|, 1)), ignore_sum equal.  The cases of random numbers assert first that no kink lies within 1e-5
(lossgrad_ref.margins_of); the dyadic cases sit ON the kinks and assert no margin.  Every direct call of a C entry runs between
the guards of tests/fence.py with dfeats / out5 pre-filled with NaN.  Every case prints its figures before it asserts (-s).

Measured on an MI355X.  Largest device error as a fraction of its bar over the cases of this file: gradient box 0.28 (total
256), confidence 0.18 (row of 305), class 0.14 (total 256); forward loss 0.11, GIoU 0.36 (row of 305), confidence 0.09, class
0.09.  The hand-derived cells come out as (0.25, -0, -0.25, 0.5), (-0.33333334, -0, -0.33333334, 0.3333333) and (0.25599998,
0.25599998, -0.384, -0.384); both threshold answers are exact.

What the file catches, tried once each on a scratch copy of the kernel:
  * one `>=` of loss_giou_grad made `>` (`pb.x >= tb.x`, the intersection's y_min): test_tie_grid fails, and so does the older
    tests/test_gpu_lossgrad.py::test_known_answer_one_box_and_its_neighbours - with prediction == label that comparison moves
    the box gradient off 0 (to 0.5 in channel 3), so this particular `>=` was already guarded; test_tie_grid misses its bar by
    0.75 against 5.8e-7.
  * the bound of the partial chunk dropped (`m = LOSS_T` for every chunk): NOT caught by the multi-chunk cases, and it cannot be
    by any deterministic test.  Past the first chunk the entries beyond the bound are boxes of the previous, full chunk of the
    same list, which the running maximum already holds: best_iou, ignore_sum and every gradient are unchanged at 257, 332-342
    and 663 boxes, and those cases stayed green.  Only a first chunk of fewer than 256 boxes reads LDS nobody wrote; what that
    holds is arbitrary.  In the run it made 34 tests fail, old and new alike (mostly as a difference between the fence's two variants), but no test
    here is built on it.  What the multi-chunk cases do pin: the barrier before a chunk is overwritten, boxes of every chunk
    reaching the maximum (forward and gradient against the reference), and reproducibility when arrival order decides the chunk."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fence, loss_ref, lossgrad_ref

pytestmark = pytest.mark.gpu

ULPS4 = 4 * 2.0 ** -24


def _rt():
    from yoloret_amd import runtime
    return runtime


def _fenced(dev, logits, y_true, anchors, input_hw, ignore_thresh=.5, grad=True):
    """yr_yolo_loss_grad (or yr_yolo_loss) through tests/fence.run with explicit anchors [A,2] and input size
    -> (out5 [5], dfeats or None) as arrays."""
    rt = _rt()
    f, y = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev)
    b, gh, gw, a, ch = f.shape
    an = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(-1, 2))
    assert an.shape[0] == a
    need = rt.yolo_loss_workspace_bytes(b, gh, gw, a)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    out5 = torch.full((5,), float('nan'), dtype=torch.float32, device=dev)
    dfeats = torch.full(f.shape, float('nan'), dtype=torch.float32, device=dev) if grad else None

    def call(moved):
        p = lambda t: rt._ptr(moved(t))
        head = (p(f), p(y), b, gh, gw, a, ch - 5, an.ctypes.data_as(ctypes.c_void_p), int(input_hw[0]), int(input_hw[1]),
                float(ignore_thresh), p(ws), need)
        if grad:
            rt.check(rt.lib().yr_yolo_loss_grad(*head, None, p(out5), p(dfeats), rt.stream_ptr(dev)))
        else:
            rt.check(rt.lib().yr_yolo_loss(*head, p(out5), rt.stream_ptr(dev)))
    with torch.cuda.device(dev):
        fence.run(call, writes=[dfeats, out5] if grad else [out5], reads=[f, y], scratch=[ws], batch=b)
    torch.cuda.synchronize()
    return out5.cpu().numpy(), dfeats.cpu().numpy() if grad else None


def _input_hw(case):
    _, logits, _, _, step = case
    return logits.shape[1] * step, logits.shape[2] * step


def _check_grad(got, case, ignore_thresh=.5, assert_margins=True):
    """got: the device's dfeats.  Prints every figure, then asserts the bar and the exact zeros -> the float64 reference's res."""
    what, logits, y_true, an, step = case
    print('%s: %d listed boxes, %d predictions, rows of %d floats' % (what, int((y_true[..., 4] != 0).sum()), y_true[..., 4].size, y_true.shape[-1]))
    if assert_margins:
        m = lossgrad_ref.margins_of(logits, y_true, an, step, ignore_thresh)
        print('%s: margins threshold %.3e, coordinates %.3e, intersection sides %.3e' % ((what,) + m))
        assert min(m) > 1e-5, '%s: a kink lies within 1e-5 (%r) - choose another case' % (what, m)
    r64, g64 = lossgrad_ref.loss_and_grad(y_true, logits, an, step, ignore_thresh, np.float64)
    _, g32 = lossgrad_ref.loss_and_grad(y_true, logits, an, step, ignore_thresh, np.float32)
    assert got.shape == g64.shape and got.dtype == np.float32 and np.isfinite(got).all(), '%s: shape / dtype / a NaN survived' % what
    dev_err, ref_err = lossgrad_ref.group_errors(got, g64), lossgrad_ref.group_errors(g32, g64)
    bad = []
    for name in dev_err:
        bar = 4 * ref_err[name] + ULPS4
        print('%s %-5s device %.3e  (float32 reference %.3e, bar %.3e, device / bar %.3f)' % (what, name, dev_err[name], ref_err[name], bar, dev_err[name] / bar))
        if not dev_err[name] <= bar:
            bad.append('%s: %.3e > %.3e' % (name, dev_err[name], bar))
    om = y_true[..., 4]
    assert np.all(got[om == 0][:, :4] == 0) and np.all(got[om == 0][:, 5:] == 0), '%s: box / class gradient in a cell without an object' % what
    assert np.all(got[(om == 0) & (r64['ignore_mask'] == 0)][:, 4] == 0), '%s: confidence gradient in an ignored cell' % what
    assert not bad, '%s: %s' % (what, '; '.join(bad))
    return r64


def _check_forward(got, case, ignore_thresh=.5, assert_margin=True):
    """got: the device's five words.  The rule of tests/test_gpu_loss.py with explicit anchors."""
    what, logits, y_true, an, step = case
    r64 = loss_ref.yolo_loss(y_true, logits, an, step, ignore_thresh, np.float64)
    r32 = loss_ref.yolo_loss(y_true, logits, an, step, ignore_thresh, np.float32)
    if assert_margin:
        margin = loss_ref.threshold_margin(r64, ignore_thresh)
        print('%s: min |best_iou - thresh| = %.3e' % (what, margin))
        assert margin > 1e-5, '%s: a best IoU lies within 1e-5 of the threshold - choose another seed' % what
    t64, t32 = loss_ref.terms(r64), loss_ref.terms(r32)
    bad = []
    for i, name in enumerate(('loss', 'giou', 'conf', 'class')):
        scale = max(abs(t64[i]), 1.0) if name == 'giou' else abs(t64[i])
        if scale == 0:
            assert got[i] == 0, '%s %s: %r, the reference is exactly 0' % (what, name, got[i])
            continue
        err, err32 = abs(float(got[i]) - t64[i]) / scale, abs(t32[i] - t64[i]) / scale
        bar = 4 * err32 + ULPS4
        print('%s forward %-5s device %.9g  float64 %.12g  rel err %.3e  (float32 reference %.3e, bar %.3e, device / bar %.3f)'
              % (what, name, got[i], t64[i], err, err32, bar, err / bar))
        if not err <= bar:
            bad.append('%s: %.3e > %.3e' % (name, err, bar))
    print('%s ignore_sum device %d reference %d' % (what, got[4], t64[4]))
    assert got[4] == t64[4], '%s: ignore_sum %r, reference %r' % (what, got[4], t64[4])
    assert not bad, '%s: %s' % (what, '; '.join(bad))


def _grad_forward_and_bits(dev, case, ignore_thresh=.5, margins=True):
    """The three checks of a case: gradient against float64, forward against loss_ref, out5 of the gradient call == the forward's
    bits -> (out5, dfeats, the float64 reference's res)."""
    _, logits, y_true, an, _ = case
    out5, g = _fenced(dev, logits, y_true, an, _input_hw(case), ignore_thresh)
    fwd, _ = _fenced(dev, logits, y_true, an, _input_hw(case), ignore_thresh, grad=False)
    r64 = _check_grad(g, case, ignore_thresh, margins)
    _check_forward(fwd, case, ignore_thresh, margins)
    assert np.array_equal(out5.view(np.uint32), fwd.view(np.uint32)), '%s: out5 %r differs from yr_yolo_loss %r' % (case[0], out5, fwd)
    return out5, g, r64


# ----------------------------------------------------------------------------- ties
def _check_known_answers(g, which):
    """The hand-derived cells (lossgrad_ref.KNOWN_TIE_ANSWERS) to 1e-6 relative; a component whose answer is 0 to 1e-6 of the
    gradients' scale in this layout, which is 1 (the non-zero answers are 0.25 .. 0.5)."""
    n = 0
    for (name, _, _, _, _), (j, i), want in lossgrad_ref.known_tie_answers():
        if name != which:
            continue
        row = g[0, j, i, 0]
        print('%s cell (%d, %d): device %r, derived %r' % (name, j, i, row, want))
        assert np.all(np.abs(row[:4] - want) <= 1e-6 * np.where(want == 0, 1.0, np.abs(want))), (name, j, i, row, want)
        assert row[4] == -0.5 and row[5] == -0.5
        n += 1
    return n


def test_tie_grid(dev):
    """169 object cells, one per pair of interval relations (y, x): every comparison of loss_giou_grad at its tie, on either
    side of it, and under every state of the `> 0` gates."""
    case = lossgrad_ref.tie_grid_case()
    out5, g, r64 = _grad_forward_and_bits(dev, case, margins=False)
    assert _check_known_answers(g, 'tie grid') == 3
    obj = case[2][..., 4] != 0
    assert np.all(g[obj][:, 4:] == -0.5)                              # sigmoid(0) - 1, exact
    assert out5[4] == r64['ignore_sum']


def test_zero_size_labels(dev):
    """Labels without width, height or either: area 0, an intersection of 0 that passes no gradient, ties of the enclosing box
    where the label sits on an edge of the prediction."""
    case = lossgrad_ref.zero_size_case()
    out5, g, r64 = _grad_forward_and_bits(dev, case, margins=False)
    assert _check_known_answers(g, 'zero-size labels') == 2
    assert out5[4] == r64['ignore_sum']


def test_threshold_on_the_last_bit(dev):
    """best_iou == 0.5 exactly: with ignore_thresh 0.5 the strict `<` is false - P leaves the confidence term, gradient exactly
    0 -; with the next float32 above 0.5 it is true: P is background, gradient sigmoid(0) = 0.5, and one more cell is counted."""
    case = lossgrad_ref.threshold_case()
    _, logits, y_true, an, _ = case
    P, Q = lossgrad_ref.THRESHOLD_P, lossgrad_ref.THRESHOLD_Q
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    want = {}
    for thresh, g_p, count in ((.5, 0.0, 255.0), (above, 0.5, 256.0)):
        out5, g = _fenced(dev, logits, y_true, an, _input_hw(case), thresh)
        fwd, _ = _fenced(dev, logits, y_true, an, _input_hw(case), thresh, grad=False)
        print('threshold %.9g: confidence gradient of P %r, ignore_sum %r' % (thresh, g[0, P[0], P[1], 0, 4], out5[4]))
        assert g[0, P[0], P[1], 0, 4] == g_p and out5[4] == count
        conf = g[..., 4].copy()
        assert conf[0, Q[0], Q[1], 0] == -0.5
        conf[0, P[0], P[1], 0] = conf[0, Q[0], Q[1], 0] = 0.5
        assert np.all(conf == 0.5)
        assert np.array_equal(out5.view(np.uint32), fwd.view(np.uint32))
        want[thresh] = (g, out5)
    r64 = _check_grad(want[.5][0], case, .5, assert_margins=False)            # the float64 reference confirms the first
    assert r64['ignore_sum'] == 255 and want[.5][1][4] == r64['ignore_sum']


# ----------------------------------------------------------------------------- more than one chunk of labelled boxes
@pytest.mark.parametrize('name', list(lossgrad_ref.CHUNK_RECIPES))
def test_chunks_of_labelled_boxes(dev, name):
    """The second and third iteration of the chunk loop of loss_main_kernel (forward and gradient instantiation): the barrier
    before a chunk is overwritten, the partial last chunk, the maximum carried across chunks."""
    _grad_forward_and_bits(dev, lossgrad_ref.chunk_case(name))


def test_bit_reproducible_across_chunks(dev):
    """tests/test_gpu_lossgrad.py::test_bit_reproducible_across_calls_streams_and_workspaces with 663 boxes: the list is in arrival
    order, which here decides the chunk a box lands in."""
    rt = _rt()
    case = lossgrad_ref.chunk_case('chunks B=4 seed 0')
    _, logits, y_true, an, _ = case
    hw = _input_hw(case)
    f, y = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev)
    first = rt.yolo_loss_grad(f, y, an, hw, .5)
    again = rt.yolo_loss_grad(f, y, an, hw, .5)
    need = rt.yolo_loss_workspace_bytes(*f.shape[:4])
    results = []
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    for pattern in (0xFF, 0x7B, 'random'):      # NaN bits (and a box count of 2^32 - 1), large finite values, random bytes
        ws = torch.empty((need + 64,), dtype=torch.uint8, device=dev)
        if pattern == 'random':
            ws.random_(0, 256)
        else:
            ws.fill_(pattern)
        out = torch.full(f.shape, float('nan'), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            results.append(rt.yolo_loss_grad(f, y, an, hw, .5, workspace=ws, out=out))
        side.synchronize()
    forward = rt.yolo_loss(f, y, an, hw, .5)
    torch.cuda.synchronize()
    bits = lambda r: (r[0].cpu().numpy().view(np.uint32), r[1].cpu().numpy().view(np.uint32))
    t0, g0 = bits(first)
    assert np.isfinite(first[1].cpu().numpy()).all()
    assert np.array_equal(t0, forward.cpu().numpy().view(np.uint32))
    for r in [again] + results:
        t, g = bits(r)
        assert np.array_equal(t, t0) and np.array_equal(g, g0)


# ----------------------------------------------------------------------------- row and slot edges of the gradient's second phase
@pytest.mark.parametrize('name', list(lossgrad_ref.EDGE_RECIPES))
def test_row_and_slot_edges(dev, name):
    """(row, channel) stepped by dq = 256 / row, dr = 256 - dq * row: dr = 0 (a row of 256), dq = 0 (rows wider than the
    workgroup), no class group (rows of 5), fewer elements than lanes, exactly 256 predictions; gid % A as the slot for A != 3."""
    _grad_forward_and_bits(dev, lossgrad_ref.edge_case(name))
