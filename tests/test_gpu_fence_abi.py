"""The entries that work in caller-owned buffers (post-processing, letterbox, YoloLoss), called through the C ABI with every buffer
between the guards of tests/fence.py: an entry writes its outputs and nothing else, nothing around a source reaches a result, and
16-byte-aligned pointers (4-byte-aligned for the int32 / dword buffers) do.  Shapes and oracle assertions are those of the tests
of each entry (tests/test_gpu_postprocess.py, test_gpu_yolo.py::test_letterbox_bit_exact, test_gpu_loss.py).

Also the positive control of the fence on the device: a byte written just past an interior is reported."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cpost, preprocess
from oracle import postprocess as pp
from tests import fence, loss_ref
from tests.util import ANCHORS
from tests.test_gpu_postprocess import _logits, _random_boxes

pytestmark = pytest.mark.gpu


def _rt():
    from yoloret_amd import runtime as rt
    return rt


def _nan(shape, dev):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=dev)


def _ints(shape, dev, v=-77):
    return torch.full(shape, v, dtype=torch.int32, device=dev)


def _anchors_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ----------------------------------------------------------------------------- the positive control
def test_fence_reports_a_byte_past_the_interior(dev):
    """After a clean launch, a torch indexed write to the first guard byte past an interior (inside the backing allocation: nothing
    outside an allocation is touched) must be reported, with the tensor and the side."""
    rt = _rt()
    x = torch.randn((2, 4, 4, 8), device=dev)
    out = _nan((2, 4, 4, 8), dev)
    wt = torch.eye(8, device=dev)
    op = rt.new_op(rt.OP_POINTWISE)
    op.h, op.w, op.cin, op.cout, op.nsrc = 4, 4, 8, 8, 1
    op.src[0] = rt.make_src(x, c=8)
    op.wgt = wt.data_ptr()
    op.out, op.out_ld = out.data_ptr(), 8
    fence.run_op(op, 2, writes=[out], reads=[x, wt])
    torch.cuda.synchronize()
    assert torch.allclose(out, x, rtol=1e-5, atol=1e-6)
    out.fill_(float('nan'))

    def call(moved):
        o = moved(out)
        assert o.data_ptr() % 256 in (0, 16)
        op.out, op.src[0].ptr, op.wgt = o.data_ptr(), moved(x).data_ptr(), moved(wt).data_ptr()
        rt.run_op(op, 2)
        flat = torch.empty(0, dtype=torch.uint8, device=dev).set_(o.untyped_storage())       # the whole backing allocation
        at = o.data_ptr() - flat.data_ptr() + o.numel() * 4      # the first byte behind the interior, inside the backing
        assert 0 < at < flat.numel()
        flat[at] = flat[at] ^ 0x5A
    with pytest.raises(fence.FenceError, match=r'written tensor writes\[0\]: guard after the tensor: bytes \+1024 \.\. \+1024 '):
        fence.run(call, writes=[out], reads=[x, wt], batch=2)
    assert torch.isnan(out).all()


# ----------------------------------------------------------------------------- decode / yolo_head / correct_boxes / nms / pack
def _decode(dev, yd, ihw, c, hw, zd=None):
    rt = _rt()
    b = yd[0].shape[0]
    an = np.ascontiguousarray(ANCHORS, np.float32)
    n = rt.num_boxes(hw[0], hw[1]) * (2 if zd else 1)
    boxes, scores = _nan((b, n, 4), dev), _nan((b, c, n), dev)

    def call(moved):
        p = lambda t: rt._ptr(moved(t))
        if zd:
            rt.check(rt.lib().yr_decode_zoom(p(yd[0]), p(yd[1]), p(yd[2]), p(zd[0]), p(zd[1]), p(zd[2]), rt.ZOOM_MUL, rt.ZOOM_ADD, b, hw[0], hw[1],
                                             3, c, 3, _anchors_ptr(an), p(ihw), p(boxes), p(scores), rt.stream_ptr(dev)))
        else:
            rt.check(rt.lib().yr_decode(p(yd[0]), p(yd[1]), p(yd[2]), b, hw[0], hw[1], 3, c, 3, _anchors_ptr(an), p(ihw), p(boxes), p(scores),
                                        rt.stream_ptr(dev)))
    fence.run(call, writes=[boxes, scores], reads=list(yd) + list(zd or []) + [ihw], batch=b)
    torch.cuda.synchronize()
    return boxes, scores


@pytest.mark.parametrize('hw,c,image_shapes', [((416, 416), 20, [(416, 416), (375, 500), (500, 375)]), ((320, 320), 20, [(240, 320)]),
                                               ((64, 96), 80, [(100, 333), (64, 96)])])
def test_decode(dev, hw, c, image_shapes):
    rt = _rt()
    rng = np.random.default_rng(11)
    b = len(image_shapes)
    ys = _logits(rng, b, hw, c)
    ys[0][0, 0, 0, 0, :] = [30.0, -30.0, 9.0, -9.0, 100.0] + [0.0] * c
    yd = [torch.from_numpy(y).to(dev) for y in ys]
    ihw = rt.image_hw_tensor(np.array(image_shapes), b, dev)
    boxes, scores = [t.cpu().numpy() for t in _decode(dev, yd, ihw, c, hw)]
    for i in range(b):
        rb, rs = cpost.decode_image([y[i] for y in ys], ANCHORS, c, image_shapes[i])
        assert np.array_equal(boxes[i], rb), 'boxes differ from the C oracle (image %d)' % i
        assert np.array_equal(scores[i], rs), 'scores differ from the C oracle (image %d)' % i


@pytest.mark.parametrize('hw,c,image_shapes', [((416, 416), 20, [(375, 500), (416, 416)]), ((64, 96), 7, [(100, 333)])])
def test_decode_zoom(dev, hw, c, image_shapes):
    rt = _rt()
    rng = np.random.default_rng(23)
    b = len(image_shapes)
    ys, zs = _logits(rng, b, hw, c), _logits(rng, b, hw, c)
    yd = [torch.from_numpy(y).to(dev) for y in ys]
    zd = [torch.from_numpy(z).to(dev) for z in zs]
    ihw = rt.image_hw_tensor(np.array(image_shapes), b, dev)
    boxes, scores = [t.cpu().numpy() for t in _decode(dev, yd, ihw, c, hw, zd)]
    for i in range(b):
        rb, rs = cpost.decode_image([y[i] for y in ys], ANCHORS, c, image_shapes[i], zoom_outputs=[z[i] for z in zs])
        assert np.array_equal(boxes[i], rb) and np.array_equal(scores[i], rs)


@pytest.mark.parametrize('with_scores', [True, False])
def test_yolo_head_and_correct_boxes(dev, with_scores):
    rt = _rt()
    rng = np.random.default_rng(5)
    b, g, a, c, hw = 2, 13, 3, 20, (416, 416)
    feats = (rng.standard_normal((b, g, g, a, c + 5)) * 2).astype(np.float32)
    fd = torch.from_numpy(feats).to(dev)
    anchors = np.ascontiguousarray(ANCHORS[[6, 7, 8]], np.float32)
    xy, wh, conf, probs = _nan((b, g, g, a, 2), dev), _nan((b, g, g, a, 2), dev), _nan((b, g, g, a, 1), dev), _nan((b, g, g, a, c), dev)
    sc = _nan((b, g, g, a, c), dev) if with_scores else None

    def head(moved):
        p = lambda t: rt._ptr(moved(t)) if t is not None else None
        rt.check(rt.lib().yr_yolo_head(p(fd), b, g, g, a, c, _anchors_ptr(anchors), hw[0], hw[1], p(xy), p(wh), p(conf), p(probs), p(sc),
                                       rt.stream_ptr(dev)))
    fence.run(head, writes=[xy, wh, conf, probs] + ([sc] if with_scores else []), reads=[fd], batch=b)
    ihw = rt.image_hw_tensor((375, 500), b, dev)
    boxes = _nan((b, g, g, a, 4), dev)

    def correct(moved):
        p = lambda t: rt._ptr(moved(t))
        rt.check(rt.lib().yr_correct_boxes(p(xy), p(wh), b, g * g * a, hw[0], hw[1], p(ihw), p(boxes), rt.stream_ptr(dev)))
    fence.run(correct, writes=[boxes], reads=[xy, wh, ihw], batch=b)
    torch.cuda.synchronize()
    for i in range(b):
        rxy, rwh, rconf, rprobs = pp.yolo_head(feats[i], anchors, hw)
        assert np.allclose(xy[i].cpu().numpy(), rxy, rtol=2e-6, atol=1e-7)
        assert np.allclose(wh[i].cpu().numpy(), rwh, rtol=2e-6, atol=1e-7)
        assert np.allclose(conf[i].cpu().numpy(), rconf, rtol=2e-6, atol=1e-7)
        assert np.allclose(probs[i].cpu().numpy(), rprobs, rtol=2e-6, atol=1e-7)
        if with_scores:
            assert np.allclose(sc[i].cpu().numpy(), rconf * rprobs, rtol=3e-6, atol=1e-7)
        rb = pp.yolo_correct_boxes(rxy, rwh, hw, (375, 500))
        assert np.allclose(boxes[i].cpu().numpy(), rb, rtol=3e-6, atol=3e-4)


def _nms(dev, boxes, scores, max_boxes, score_thr, iou_thr):
    rt = _rt()
    b, c, n = scores.shape
    idx, cnt = _ints((b, c, max_boxes), dev), _ints((b, c), dev)

    def call(moved):
        p = lambda t: rt._ptr(moved(t))
        rt.check(rt.lib().yr_nms(p(boxes), p(scores), b, n, c, max_boxes, score_thr, iou_thr, p(idx), p(cnt), rt.stream_ptr(dev)))
    fence.run(call, writes=[idx, cnt], reads=[boxes, scores], batch=b)
    torch.cuda.synchronize()
    return idx, cnt


@pytest.mark.parametrize('n,c,score_thr,ties', [(10647, 20, 0.2, False), (3000, 7, 0.3, True), (100, 3, 0.99, False), (257, 2, 0.1, True),
                                                (25200, 3, 0.2, True)])
def test_nms(dev, n, c, score_thr, ties):
    rng = np.random.default_rng(n + c)
    b = 2
    boxes = np.stack([_random_boxes(rng, n) for _ in range(b)])
    scores = rng.random((b, c, n), dtype=np.float32)
    if ties:
        scores = np.round(scores * 8) / 8
    scores = scores.astype(np.float32)
    idx, cnt = _nms(dev, torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), 20, score_thr, 0.5)
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    for i in range(b):
        for k in range(c):
            ref = cpost.nms(boxes[i], scores[i, k], 20, 0.5, score_thr)
            assert cnt[i, k] == len(ref)
            assert np.array_equal(idx[i, k, :len(ref)], ref), (i, k)
            assert (idx[i, k, len(ref):] == -1).all()


def test_nms_with_more_candidates_than_the_first_pass_list(dev):
    """... through both launches of the entry (the histogram cut, then the full-capacity pass: kind 'duplicates' of
    tests/test_gpu_postprocess.py)."""
    rng = np.random.default_rng(3)
    n, c, b = 10647, 3, 2
    scores = (0.2 + 0.8 * rng.random((b, c, n))).astype(np.float32)
    proto = _random_boxes(rng, 7, degenerate=False)
    boxes = np.stack([proto[rng.integers(0, 7, n)] for _ in range(b)])
    idx, cnt = _nms(dev, torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), 20, 0.2, 0.5)
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    for i in range(b):
        for k in range(c):
            ref = cpost.nms(boxes[i], scores[i, k], 20, 0.5, 0.2)
            assert cnt[i, k] == len(ref) and np.array_equal(idx[i, k, :len(ref)], ref) and (idx[i, k, len(ref):] == -1).all()


def test_pack_detections(dev):
    rt = _rt()
    rng = np.random.default_rng(21)
    b, c, hw, mx = 3, 20, (416, 416), 20
    ys = _logits(rng, b, hw, c, scale=2.5)
    shapes = [(416, 416), (375, 500), (300, 300)]
    yd = [torch.from_numpy(y).to(dev) for y in ys]
    ihw = rt.image_hw_tensor(np.array(shapes), b, dev)
    boxes, scores = _decode(dev, yd, ihw, c, hw)
    idx, cnt = _nms(dev, boxes, scores, mx, 0.2, 0.5)
    n = scores.shape[2]
    det, dcnt = _ints((b, c * mx, 6), dev), _ints((b,), dev)

    def call(moved):
        p = lambda t: rt._ptr(moved(t))
        rt.check(rt.lib().yr_pack_detections(p(boxes), p(scores), p(idx), p(cnt), b, n, c, mx, p(det), p(dcnt), rt.stream_ptr(dev)))
    fence.run(call, writes=[det, dcnt], reads=[boxes, scores, idx, cnt], batch=b)
    torch.cuda.synchronize()
    det, dcnt = det.cpu().numpy(), dcnt.cpu().numpy()
    for i in range(b):
        rb, rs, rc, _ = cpost.yolo_eval([y[i] for y in ys], ANCHORS, 3, c, shapes[i], 20, 0.2, 0.5)
        k = dcnt[i]
        assert k == len(rs)
        assert np.array_equal(det[i, :k, 0:4], rb)
        assert np.array_equal(det[i, :k, 4].view(np.float32), rs)
        assert np.array_equal(det[i, :k, 5], rc)
        assert (det[i, k:, 5] == -1).all() and (det[i, k:, :5] == 0).all()


# ----------------------------------------------------------------------------- letterbox
@pytest.mark.parametrize('batched', [False, True])
@pytest.mark.parametrize('ihw,size', [((375, 500), (416, 416)), ((500, 375), (416, 416)), ((64, 64), (96, 96)),
                                      ((1080, 1920), (320, 320)), ((33, 17), (64, 96))])
def test_letterbox(dev, ihw, size, batched):
    """yr_letterbox (one image) and yr_letterbox_batch (three equally sized images): the uint8 source's bytes are a multiple of
    neither 4 nor 16 at the odd sizes."""
    rt = _rt()
    rng = np.random.default_rng(ihw[0])
    b = 3 if batched else 1
    imgs = rng.integers(0, 256, (b, ihw[0], ihw[1], 3), dtype=np.uint8)
    src = torch.from_numpy(imgs).to(dev)
    dst = _nan((b, size[0], size[1], 3), dev)

    def call(moved):
        s, d = rt._ptr(moved(src)), rt._ptr(moved(dst))
        if batched:
            rt.check(rt.lib().yr_letterbox_batch(s, b, ihw[0], ihw[1], d, size[0], size[1], rt.stream_ptr(dev)))
        else:
            rt.check(rt.lib().yr_letterbox(s, ihw[0], ihw[1], d, size[0], size[1], rt.stream_ptr(dev)))
    fence.run(call, writes=[dst], reads=[src], batch=b)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    for i in range(b):
        ref, _ = preprocess.letterbox_image(imgs[i], size)
        assert np.array_equal(out[i], ref), 'image %d' % i


# ----------------------------------------------------------------------------- YoloLoss
@pytest.mark.parametrize('pattern', [0xFF, 0x7B, 'random'])
def test_yolo_loss_stays_inside_its_workspace(dev, pattern):
    """yr_yolo_loss with a workspace of exactly yr_yolo_loss_workspace_bytes, poisoned (NaN bits and a box count of 2^32 - 1, large
    finite values, random bytes): nothing around the workspace, the five words or the two sources is touched or used, the five
    words are those of the plain call bit for bit, and they meet the reference at the bar of tests/test_gpu_loss.py."""
    from tests.test_gpu_loss import _check_against_reference
    rt = _rt()
    logits, y_true = loss_ref.random_case(1, 8, (416, 416), 20, ANCHORS, scales=(2,))[2]
    f, y = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev)
    an = np.ascontiguousarray(loss_ref.scale_anchors(ANCHORS, 2), np.float32)
    b, gh, gw, a, ch = f.shape
    plain = rt.yolo_loss(f, y, an, (416, 416), .5)
    need = rt.yolo_loss_workspace_bytes(b, gh, gw, a)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    if pattern == 'random':
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        ws.random_(0, 256, generator=g)
    else:
        ws.fill_(pattern)
    out5 = _nan((5,), dev)

    def call(moved):
        p = lambda t: rt._ptr(moved(t))
        rt.check(rt.lib().yr_yolo_loss(p(f), p(y), b, gh, gw, a, ch - 5, _anchors_ptr(an), 416, 416, .5, p(ws), need, p(out5), rt.stream_ptr(dev)))
    fence.run(call, writes=[out5], reads=[f, y], scratch=[ws], batch=b)     # (the list of boxes in the workspace is in arrival order)
    torch.cuda.synchronize()
    got = out5.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), plain.cpu().numpy().view(np.uint32))
    _check_against_reference(got, logits, y_true, 2, 'fenced, workspace %r' % (pattern,))
