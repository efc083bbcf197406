"""random_jpeg_quality on the device (yoloret_amd/csrc/jpeg.hip behind yr_jpeg_roundtrip_batch) against tests/jpeg_ref.py and the
committed Pillow goldens, bit for bit, and get_random_data_device / AugmentedDataset with apply_jpeg=True end to end.  Every call of
the C entry runs between the guards of tests/fence.py at both alignments: the images are a written tensor, the workspace
(pre-filled with 0xFF) a scratch tensor, the qualities a read tensor.

Inputs: tests/jpeg_cases.py.  16x16 is a single MCU (every upsampling edge rule at once); 16x48 and 48x16 have left / middle / right
and top / middle / bottom MCUs; 48x80 has an MCU with all eight neighbours and is not square."""
import os

import numpy as np
import pytest
import torch

from tests import fence, jpeg_cases as jc, jpeg_ref as jr
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

F = np.float32
GPU_CONTENTS = ('noise', 'primaries', 'black', 'white', 'demo', 'step_a')
_cache = {}


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _golden():
    if 'golden' not in _cache:
        with np.load(os.path.join(jc.GOLDEN, 'jpeg_cases.npz')) as z:
            _cache['golden'] = {k: z[k] for k in z.files}
    return _cache['golden']


def _input(content, shape):
    """float32 [H,W,3]: the uint8 contents as u * (1 / 255)f (step a gives u back), or the image of step-a boundary values."""
    return jc.step_a_image(shape) if content == 'step_a' else jc.image(content, shape).astype(F) * F(1.0 / 255)


def _want(content, shape, q):
    """The restatement's round trip, computed once per case and left unchanged."""
    key = (content, shape, q)
    if key not in _cache:
        out = jr.roundtrip(_input(content, shape), q)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _roundtrip(dev, x, quality, ws_fill=0xFF, rc=0, ws_bytes=None):
    """One fenced call of yr_jpeg_roundtrip_batch on a copy of x [B,H,W,3] -> the images after the call (a device tensor)."""
    from yoloret_amd import runtime as rt
    L = rt.lib()
    img = torch.from_numpy(np.ascontiguousarray(x, F)).to(dev)
    b, h, w = (int(n) for n in img.shape[:3])
    q = torch.from_numpy(np.asarray(quality, np.int32)).to(dev)
    n = rt.jpeg_workspace_bytes(img.shape[0], img.shape[1:3]) if ws_bytes is None else ws_bytes
    ws = torch.full((n,), ws_fill, dtype=torch.uint8, device=dev)

    def call(moved):
        got = L.yr_jpeg_roundtrip_batch(rt._ptr(moved(img)), rt._ptr(moved(q)), b, h, w, rt._ptr(moved(ws)), ws.numel(), rt.stream_ptr(dev))
        assert got == rc, (got, L.yr_last_error())
    fence.run(call, writes=[img], reads=[q], batch=b, scratch=[ws])
    torch.cuda.synchronize()
    return img


@pytest.mark.parametrize('shape', jc.GOLDEN_SHAPES, ids=['%dx%d' % s for s in jc.GOLDEN_SHAPES])
def test_roundtrip_bit_exact(dev, shape):
    """Every content at one shape in ONE batch, once per quality group: the restatement and, where committed, Pillow's own bytes."""
    g = _golden()
    x = np.stack([_input(c, shape) for c in GPU_CONTENTS])
    for qs in ((1, 50, 99, 100, 87, 93), (80, 37, 100, 1, 50, 99)):      # one quality per image, every image at several
        got = _roundtrip(dev, x, qs).cpu().numpy()
        for i, (c, q) in enumerate(zip(GPU_CONTENTS, qs)):
            want = _want(c, shape, q)
            assert np.array_equal(_bits(got[i]), _bits(want)), '%s %s quality %d: %d elements differ, max %g' % (
                c, shape, q, (_bits(got[i]) != _bits(want)).sum(), np.abs(got[i] - want).max())
            key = 'out/%s/%dx%d/q%d' % ((c,) + shape + (q,))
            if key in g:
                assert np.array_equal(_bits(got[i]), _bits(g[key].astype(F) * F(1.0 / 255))), 'Pillow golden %s' % key
    assert not np.array_equal(got[0], x[0])      # (the round trip is not the identity)


def test_every_committed_golden(dev):
    """The committed Pillow outputs directly: per shape one batch of every (content, quality) pair of the golden file."""
    g = _golden()
    for shape in jc.GOLDEN_SHAPES:
        pairs = [(c, q) for c, s in jc.GOLDEN_CASES if s == shape for q in jc.GOLDEN_QUALITIES]
        x = np.stack([g['in/%s/%dx%d' % ((c,) + shape)].astype(F) * F(1.0 / 255) for c, _ in pairs])
        got = _roundtrip(dev, x, [q for _, q in pairs]).cpu().numpy()
        for i, (c, q) in enumerate(pairs):
            want = g['out/%s/%dx%d/q%d' % ((c,) + shape + (q,))].astype(F) * F(1.0 / 255)
            assert np.array_equal(_bits(got[i]), _bits(want)), '%s %s quality %d: %d elements differ' % (c, shape, q, (_bits(got[i]) != _bits(want)).sum())


def test_batch_of_four_qualities_and_independence(dev):
    shape, qs = (48, 80), [1, 50, 99, 100]
    x = np.stack([_input('noise', shape)] * 4)
    one = _roundtrip(dev, x, qs)
    for i, q in enumerate(qs):
        assert np.array_equal(_bits(one[i]), _bits(_want('noise', shape, q))), 'quality %d' % q
    two = _roundtrip(dev, x, qs)                        # the same call twice
    other = _roundtrip(dev, x, qs, ws_fill=0x00)        # whatever the workspace held
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)) and torch.equal(one.view(torch.int32), other.view(torch.int32))
    mixed = np.stack([_input(c, shape) for c in ('primaries', 'noise', 'step_a', 'white')])
    batch = _roundtrip(dev, mixed, qs)
    for i in range(4):                                  # image b alone == slice b of the batch
        alone = _roundtrip(dev, mixed[i:i + 1], qs[i:i + 1])
        assert torch.equal(alone[0].view(torch.int32), batch[i].view(torch.int32)), 'image %d alone' % i
    # qualities outside 1..100 are clamped on the device
    clamped = _roundtrip(dev, x, [0, -7, 101, 1 << 30])
    assert torch.equal(clamped[0].view(torch.int32), one[0].view(torch.int32)) and torch.equal(clamped[1].view(torch.int32), one[0].view(torch.int32))
    assert torch.equal(clamped[2].view(torch.int32), one[3].view(torch.int32)) and torch.equal(clamped[3].view(torch.int32), one[3].view(torch.int32))


def test_refusals_write_nothing(dev):
    from yoloret_amd import runtime as rt
    L = rt.lib()
    x = np.full((2, 24, 16, 3), np.nan, F)
    need = rt.jpeg_workspace_bytes(2, (32, 16))
    got = _roundtrip(dev, x, [50, 50], rc=-1, ws_bytes=need)      # H = 24: not whole MCUs
    assert b'multiples of 16' in L.yr_last_error() and torch.isnan(got).all()
    x = np.full((2, 32, 16, 3), np.nan, F)
    got = _roundtrip(dev, x, [50, 50], rc=-1, ws_bytes=need - 16)      # a short workspace
    assert b'workspace' in L.yr_last_error() and torch.isnan(got).all()
    img = torch.zeros((1, 16, 16, 3), dtype=torch.float32, device=dev)
    q = torch.full((1,), 50, dtype=torch.int32, device=dev)
    ws = torch.empty(rt.jpeg_workspace_bytes(1, (16, 16)), dtype=torch.uint8, device=dev)
    p, s = rt._ptr, rt.stream_ptr(dev)
    assert L.yr_jpeg_roundtrip_batch(None, p(q), 1, 16, 16, p(ws), ws.numel(), s) == -1 and b'null' in L.yr_last_error()
    assert L.yr_jpeg_roundtrip_batch(p(img), None, 1, 16, 16, p(ws), ws.numel(), s) == -1
    assert L.yr_jpeg_roundtrip_batch(p(img), p(q), 1, 16, 16, None, ws.numel(), s) == -1
    assert L.yr_jpeg_roundtrip_batch(p(img), p(q), 8, 16384, 16384, p(ws), 1 << 40, s) == -1 and b'2^31' in L.yr_last_error()
    assert rt.jpeg_workspace_bytes(3, (48, 80)) == 3 * 48 * 80 * 3 // 2
    # the Python entry: CPU tensors, shapes, qualities
    with pytest.raises(ValueError, match='CUDA'):
        rt.jpeg_roundtrip_batch(torch.zeros(1, 16, 16, 3), [50])
    with pytest.raises(ValueError, match='multiples of 16'):
        rt.jpeg_roundtrip_batch(torch.zeros((1, 24, 16, 3), device=dev), [50])
    with pytest.raises(ValueError, match='quality'):
        rt.jpeg_roundtrip_batch(img, [50, 60])
    with pytest.raises(ValueError, match='quality'):
        rt.jpeg_roundtrip_batch(img, torch.tensor([50], dtype=torch.int32))      # a CPU tensor
    out = rt.jpeg_roundtrip_batch(img, np.array([50]))
    assert out is img


def test_random_jpeg_quality_device(dev):
    from yoloret_amd.yolo3.utils import random_jpeg_quality_device
    shape = (32, 32)
    x = np.stack([_input(c, shape) for c in ('noise', 'demo', 'primaries')])
    draws = np.array([0.0, 0.5, 1 - 2.0 ** -24], F)
    img = torch.from_numpy(x.copy()).to(dev)
    out, quality = random_jpeg_quality_device(img, 80, 100, draws=draws)
    torch.cuda.synchronize()
    assert out is img and quality.dtype == np.int32 and quality.tolist() == [80, 90, 99]
    for i, q in enumerate(quality):
        assert np.array_equal(_bits(out[i]), _bits(jr.roundtrip(x[i], int(q))))
    a, qa = random_jpeg_quality_device(torch.from_numpy(x.copy()).to(dev), 0, 100, seed=9)
    b, qb = random_jpeg_quality_device(torch.from_numpy(x.copy()).to(dev), 0, 100, seed=9)
    want = [jr.draw_quality(u, 0, 100) for u in np.random.default_rng(9).random(3, dtype=F)]
    assert qa.tolist() == qb.tolist() == want and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ----------------------------------------------------------------------------- the training data path with the step switched on
HW, C, S = (96, 96), 20, 3


def _demos():
    from PIL import Image
    paths = [os.path.join(jc.GOLDEN, n) for n in jc.DEMOS]
    return paths, [np.array(Image.open(p).convert('RGB'), dtype=np.uint8) for p in paths]


def _rows(im, k):
    ih, iw = im.shape[:2]
    return [[int(.1 * iw), int(.2 * ih), int(.6 * iw), int(.9 * ih), 3 + k], [int(.5 * iw), int(.1 * ih), int(.95 * iw), int(.5 * ih), 11]]


def test_get_random_data_device_apply_jpeg(dev):
    from yoloret_amd.yolo3.utils import get_random_data_device
    _, images = _demos()
    boxes = np.array([_rows(im, k) for k, im in enumerate(images)], F)
    counts = np.array([2, 2], np.int32)
    draws = np.random.default_rng(21).random((2, 10), dtype=F)
    jd = np.array([0.26, 0.93], F)
    off = get_random_data_device(images, boxes, counts, HW, draws=draws, device=dev)
    on = get_random_data_device(images, boxes, counts, HW, draws=draws, device=dev, apply_jpeg=True, jpeg_draws=jd)
    same = get_random_data_device(images, boxes, counts, HW, draws=draws, device=dev, apply_jpeg=True, jpeg_draws=jd, min_jpeg_quality=90, max_jpeg_quality=90)
    torch.cuda.synchronize()
    base = off[0].cpu().numpy()
    for i, u in enumerate(jd):
        q = jr.draw_quality(u, 80, 100)
        assert q == (85, 98)[i]
        assert np.array_equal(_bits(on[0][i]), _bits(jr.roundtrip(base[i], q))), 'image %d' % i
    assert not np.array_equal(_bits(on[0]), _bits(base))
    assert np.array_equal(_bits(on[1]), _bits(off[1])) and on[2].cpu().tolist() == off[2].cpu().tolist()      # boxes and kept
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(same, off))      # min == max: the step is off
    # without jpeg_draws the uniforms are those of default_rng((seed, 1)); the ten draws stay those of default_rng(seed)
    s_on = get_random_data_device(images, boxes, counts, HW, seed=6, device=dev, apply_jpeg=True)
    s_off = get_random_data_device(images, boxes, counts, HW, seed=6, device=dev)
    torch.cuda.synchronize()
    qs = [jr.draw_quality(u, 80, 100) for u in np.random.default_rng((6, 1)).random(2, dtype=F)]
    for i in range(2):
        assert np.array_equal(_bits(s_on[0][i]), _bits(jr.roundtrip(s_off[0][i].cpu().numpy(), qs[i])))


def test_augmented_dataset_apply_jpeg(dev, tmp_path):
    from PIL import Image
    from yoloret_amd.yolo3.data import AugmentedDataset
    paths, images = _demos()
    png = tmp_path / 'third.png'
    third = np.random.RandomState(11).randint(0, 256, size=(61, 45, 3)).astype(np.uint8)
    Image.fromarray(third).save(str(png))
    paths, images = paths + [str(png)], images + [third]
    labels = tmp_path / 'train_3.txt'
    labels.write_text('\n'.join(p + ' ' + ' '.join('%d %d %d %d %d' % tuple(r) for r in _rows(im, k)) for k, (p, im) in enumerate(zip(paths, images))) + '\n')

    def run(**kw):
        ds = AugmentedDataset(str(labels), 3, ANCHORS, C, HW, S, seed=3, device=dev, **kw)
        it, num = ds.build()
        assert num == 3
        out = []
        for _ in range(2):
            for x, y_true in it:
                torch.cuda.synchronize()
                out.append((x.cpu().numpy(), [y.cpu().numpy() for y in y_true], ds.last_draws.copy(),
                            None if ds.last_quality is None else ds.last_quality.copy()))
        return out
    on, again, off = run(apply_jpeg=True), run(apply_jpeg=True), run()
    assert len(on) == len(off) == 2 and on[0][0].shape == (3, 96, 96, 3)
    second = np.random.default_rng((3, 1))
    for a, b, o in zip(on, again, off):
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[3], b[3])      # the same seed: the same bytes
        assert np.array_equal(a[2], o[2]) and o[3] is None                                  # the ten draws do not depend on the switch
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a[1], o[1]))          # nor does y_true
        want_q = [jr.draw_quality(u, 80, 100) for u in second.random(3, dtype=F)]
        assert a[3].tolist() == want_q
        for i in range(3):      # the restatement chain: the apply_jpeg=False image through the round trip at the drawn quality
            assert np.array_equal(_bits(a[0][i]), _bits(jr.roundtrip(o[0][i], want_q[i]))), 'image %d' % i
    assert not np.array_equal(on[0][3], on[1][3])      # a further pass draws new qualities
