"""The training data transform on the device (yoloret_amd/csrc/augment.hip behind yr_augment_batch) against tests/augment_ref.py,
and yolo3.data.AugmentedDataset end to end.  Every call of the C entry runs between the guards of tests/fence.py: dst, boxes_out,
kept and the workspace are written tensors; the packed source, the table, the boxes and the counts are read tensors.

Inputs: tests/augment_cases.py - five sources (5x7, 9x4 greys, 13x13 primaries, 20x3, 61x45), canvases 8x12, 36x52 and 52x36, one
row of draws per image.  Geometry, flip, hue and saturation are compared on raw bytes; gamma and contrast against the float64
evaluation of the same float32 pre-gamma tensor, within max(4 E_ref, 4 * 2^-24), E_ref being the float32 restatement's own largest
deviation from float64 on the same inputs."""
import os

import numpy as np
import pytest
import torch

from tests import augment_cases as ac, augment_ref as ar, fence
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SENTINEL = -77
ALL = ar.HUE | ar.SAT | ar.GAMMA | ar.CONTRAST
_cache = {}


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _expected(size, stages, dtype=F):
    """The restatement's images of the five sources, computed once per (canvas, stages, dtype) and left unchanged."""
    key = ('exp', size, stages, np.dtype(dtype).name)
    if key not in _cache:
        out = [ar.image(im, size, g, stages, dtype) for im, g in zip(ac.images(), ac.geometries(size, stages))]
        for o in out:
            o.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _pack(images, draws, size, stages, dev, fill=0xA5):
    """-> (table, packed source on the device): the staging a caller does, byte by byte; the padding between images must not matter."""
    from yoloret_amd import runtime as rt
    table = rt.augment_geometry([im.shape[:2] for im in images], size, draws, stages=stages)
    buf = np.full(table.packed_bytes, fill, np.uint8)
    for im, off in zip(images, table.host['src_off']):
        buf[off:off + im.size] = im.reshape(-1)
    table.upload(dev)
    return table, torch.from_numpy(buf).to(dev)


def _augment(dev, table, src, size, boxes=None, counts=None, max_boxes=20):
    """One fenced call of yr_augment_batch -> (dst, boxes_out, kept, workspace as float32); the outputs start as NaN / SENTINEL."""
    from yoloret_amd import runtime as rt
    L = rt.lib()
    b, (h, w) = table.batch, size
    dst = torch.full((b, h, w, 3), float('nan'), dtype=torch.float32, device=dev)
    ws = torch.full((rt.augment_workspace_bytes(b, size) // 4,), float('nan'), dtype=torch.float32, device=dev)
    boxes_out = kept = None
    max_in = 0
    if boxes is not None:
        max_in = boxes.shape[1]
        boxes_out = torch.full((b, max_boxes, 5), float('nan'), dtype=torch.float32, device=dev)
        kept = torch.full((b,), SENTINEL, dtype=torch.int32, device=dev)

    def call(moved):
        p = lambda t: rt._ptr(moved(t)) if t is not None else None
        rt.check(L.yr_augment_batch(p(src), p(table.device), b, table.stages, p(dst), h, w, p(boxes), p(counts), max_in, p(boxes_out), p(kept),
                                    max_boxes, p(ws), ws.numel() * 4, rt.stream_ptr(dev)))
    fence.run(call, writes=[dst, boxes_out, kept, ws], reads=[src, table.device, boxes, counts], batch=b)
    torch.cuda.synchronize()
    return dst, boxes_out, kept, ws


def test_the_draws_reach_every_branch_before_the_gpu_is_touched():
    kinds, flips, clamps = ac.coverage()
    assert kinds == {'pad', 'crop_x', 'crop_y', 'crop_xy'} and flips == {0, 1} and clamps == {0, 1}


@pytest.mark.parametrize('stages', [0, ar.HUE | ar.SAT], ids=['geometry-flip-clip', 'hue-saturation'])
@pytest.mark.parametrize('size', ac.CANVASES, ids=['8x12', '36x52', '52x36'])
def test_images_bit_exact(dev, size, stages):
    images, want = ac.images(), _expected(size, stages)
    if stages:      # the restatement itself takes the range == 0 and the tie branches on these sources
        pre = [ar.canvas(im, size, g) for im, g in zip(images, ac.geometries(size, stages))]
        assert any(((p.max(axis=2) == p.min(axis=2)) & (p.max(axis=2) > 0)).any() for p in pre), 'no grey pixel'
        assert any((p[..., 0] == p[..., 1]).any() and (p[..., 0] > p[..., 2]).any() for p in pre[2:3]), 'no tie r == g'
        assert (pre[2].max(axis=2) == 1).any() and (pre[2].min(axis=2) == 0).any()
    table, src = _pack(images, ac.DRAWS, size, stages, dev)
    dst, _, _, _ = _augment(dev, table, src, size)
    got = dst.cpu().numpy()
    for i in range(len(images)):
        assert np.array_equal(_bits(got[i]), _bits(want[i])), 'image %d %s on %s: %d elements differ, max %g' % (
            i, ac.SOURCES[i], size, (_bits(got[i]) != _bits(want[i])).sum(), np.abs(got[i] - want[i]).max())


@pytest.mark.parametrize('size', ac.CANVASES, ids=['8x12', '36x52', '52x36'])
def test_boxes_bit_exact(dev, size):
    images = ac.images()
    boxes, counts = ac.boxes(size)
    geo = ac.geometries(size, 0)
    want, want_kept, seen = [], [], {'flip_across_clip': 0, 'dropped_after_crop': 0, 'cap': 0, 'count0': 0}
    for i, g in enumerate(geo):
        out, kept, info = ar.map_boxes(boxes[i, :counts[i]], g, size)
        want.append(out)
        want_kept.append(kept)
        raw, n = info['raw'], counts[i]
        if n and g['flip']:      # before the flip xmin was inside [0, 1); after it xmax lies beyond W - 1 and is clipped
            seen['flip_across_clip'] += int(((raw[:, 2] > size[1] - 1) & (raw[:, 2] <= size[1]) & info['keep']).sum())
        if n and ar.window_kind(g, size) == 'crop_xy':
            seen['dropped_after_crop'] += int(((raw[:, 2] - raw[:, 0] > 1) & (raw[:, 3] - raw[:, 1] > 1) & ~(info['w'] > 1)).sum())
        seen['cap'] += int(info['passed'] > 20)
        seen['count0'] += int(n == 0)
    print('canvas %s: kept %s, reference branches %s' % (size, want_kept, seen))
    assert all(v >= 1 for v in seen.values()), seen
    table, src = _pack(images, ac.DRAWS, size, 0, dev)
    b, c = torch.from_numpy(np.array(boxes)).to(dev), torch.from_numpy(counts).to(dev)
    dst, boxes_out, kept, _ = _augment(dev, table, src, size, b, c)
    assert kept.cpu().tolist() == want_kept
    got = boxes_out.cpu().numpy()
    for i in range(len(images)):
        assert np.array_equal(_bits(got[i]), _bits(want[i])), 'boxes of image %d: %s != %s' % (i, got[i, :3], want[i][:3])
    ref = _expected(size, 0)
    img = dst.cpu().numpy()
    assert all(np.array_equal(_bits(img[i]), _bits(ref[i])) for i in range(len(images)))      # the image part is the same with boxes


@pytest.mark.parametrize('size', ac.CANVASES, ids=['8x12', '36x52', '52x36'])
def test_all_stages_against_float64(dev, size):
    """Measured on an MI355X (profiles/r11_augment_probe.txt repeats them):
        canvas   E_ref (float32 restatement vs float64)   device vs float64   bound max(4 E_ref, 4 * 2^-24)
        8x12     1.197e-07                                 6.999e-08           4.789e-07
        36x52    1.336e-07                                 1.273e-07           5.344e-07
        52x36    1.331e-07                                 1.166e-07           5.322e-07
    and the per-image channel means, rebuilt from the workspace's slots, within 1.6e-08 of float64 on every canvas.
    The margin covers a device powf that differs from NumPy's by an ulp or two, feeding a contrast factor of up to 1.1, and a
    different summation order of the mean."""
    images = ac.images()
    geo = ac.geometries(size, ALL)
    want64, want32 = _expected(size, ALL, np.float64), _expected(size, ALL)
    e_ref = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(want32, want64))
    bound = max(4 * e_ref, 4 * 2.0 ** -24)
    table, src = _pack(images, ac.DRAWS, size, ALL, dev)
    b, c = torch.from_numpy(np.array(ac.boxes(size)[0])).to(dev), torch.from_numpy(ac.boxes(size)[1]).to(dev)
    dst, boxes_out, kept, ws = _augment(dev, table, src, size, b, c)
    got = dst.cpu().numpy()
    err = max(float(np.abs(got[i].astype(np.float64) - want64[i]).max()) for i in range(len(images)))
    print('canvas %s: E_ref %.3e, device vs float64 %.3e, bound %.3e' % (size, e_ref, err, bound))
    assert err <= bound
    assert (got >= 0).all() and (got <= 1).all()
    # the channel means: the workspace keeps one slot of three sums per workgroup
    blocks = (size[0] * size[1] // 4 + 255) // 256
    slots = ws.cpu().numpy()[:len(images) * blocks * 3].reshape(len(images), blocks, 3).astype(np.float64)
    worst = 0.0
    for i, (im, g) in enumerate(zip(images, geo)):
        mean64 = ar.gamma_contrast(ar.pre_gamma(im, size, g, ALL), g, ALL, np.float64)[1]
        worst = max(worst, float(np.abs(slots[i].sum(axis=0) / (size[0] * size[1]) - mean64).max()))
    print('canvas %s: channel means vs float64 %.3e' % (size, worst))
    assert worst <= bound
    # the boxes do not depend on the colour stages
    zero = [ar.map_boxes(ac.boxes(size)[0][i, :ac.boxes(size)[1][i]], g, size) for i, g in enumerate(geo)]
    assert kept.cpu().tolist() == [z[1] for z in zero]
    assert all(np.array_equal(_bits(boxes_out[i]), _bits(zero[i][0])) for i in range(len(images)))


@pytest.mark.parametrize('stages', [ALL, ar.HUE | ar.GAMMA | ar.NOFLIP], ids=['all', 'no-contrast-no-flip'])
def test_same_call_twice_and_batch_of_one(dev, stages):
    size = (36, 52)
    images = ac.images()
    boxes, counts = ac.boxes(size)
    table, src = _pack(images, ac.DRAWS, size, stages, dev)
    b, c = torch.from_numpy(np.array(boxes)).to(dev), torch.from_numpy(counts).to(dev)
    one = _augment(dev, table, src, size, b, c)
    two = _augment(dev, table, src, size, b, c)
    for x, y in zip(one[:3], two[:3]):
        assert np.array_equal(_bits(x), _bits(y))
    if not stages & ar.CONTRAST:
        assert torch.isnan(one[3]).all()      # launch 2 carries only the boxes: the workspace is not touched
        assert not table.host['flip'].any()
    for i, im in enumerate(images):      # per-image sums do not leak across images
        t1, s1 = _pack([im], ac.DRAWS[i:i + 1], size, stages, dev, fill=0x3C)
        d1, b1, k1, _ = _augment(dev, t1, s1, size, b[i:i + 1].contiguous(), c[i:i + 1].contiguous())
        assert np.array_equal(_bits(d1[0]), _bits(one[0][i])), 'image %d alone' % i
        assert np.array_equal(_bits(b1[0]), _bits(one[1][i])) and k1.cpu().tolist() == one[2][i:i + 1].cpu().tolist()


def test_wrapper_stager_and_argument_errors(dev):
    from yoloret_amd import runtime as rt
    from yoloret_amd.yolo3.utils import get_random_data_device
    size = (36, 52)
    images = ac.images()
    boxes, counts = ac.boxes(size)
    table, src = _pack(images, ac.DRAWS, size, ALL, dev)
    b, c = torch.from_numpy(np.array(boxes)).to(dev), torch.from_numpy(counts).to(dev)
    want = _augment(dev, table, src, size, b, c)
    stager = rt.RaggedStager(dev)
    packed, staged = stager.upload_table(images, rt.augment_geometry(ac.SOURCES, size, ac.DRAWS))
    assert stager._host.is_pinned() and packed.data_ptr() % 16 == 0 and staged.device.data_ptr() % 16 == 0 and staged.stages == ALL
    wx, wb, wk = rt.augment_batch(packed, staged, size, boxes=b, box_count=c)
    gx, gb, gk = get_random_data_device(images, boxes, counts, size, draws=ac.DRAWS, device=dev)
    torch.cuda.synchronize()
    for got in ((wx, wb, wk), (gx, gb, gk)):
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got, want[:3]))
    only = rt.augment_batch(packed, staged, size)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(only), _bits(want[0]))
    # flip=False is honoured: the canvas of a flipped image, mirrored back, with the other stages off
    fx, _, _ = get_random_data_device(images, boxes, counts, size, draws=ac.DRAWS, device=dev, flip=False, hue=0, sat=0, min_gamma=1, max_gamma=1, cont=0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(fx[0]), _bits(_expected(size, 0)[0][:, ::-1])) and ac.geometries(size, 0)[0]['flip'] == 1
    with pytest.raises(ValueError, match='not computed for these'):
        stager.upload_table(images[:2], staged)
    with pytest.raises(ValueError, match='uploaded AugmentTable'):
        rt.augment_batch(packed, rt.augment_geometry(ac.SOURCES, size, ac.DRAWS), size)
    with pytest.raises(ValueError, match='computed for'):
        rt.augment_batch(packed, staged, (52, 36))
    # at the C entry: H * W no multiple of 4, a workspace that is too small; the outputs are left alone
    L = rt.lib()
    dst = torch.full((5, 36, 52, 3), float('nan'), dtype=torch.float32, device=dev)
    p, s = rt._ptr, rt.stream_ptr(dev)
    assert L.yr_augment_batch(p(packed), p(staged.device), 5, ALL, p(dst), 7, 9, None, None, 0, None, None, 20, None, 0, s) == -1
    assert b'multiple of 4' in L.yr_last_error()
    ws = torch.empty(16, dtype=torch.uint8, device=dev)
    assert L.yr_augment_batch(p(packed), p(staged.device), 5, ALL, p(dst), 36, 52, None, None, 0, None, None, 20, p(ws), 16, s) == -1
    assert b'workspace' in L.yr_last_error()
    assert L.yr_augment_batch(p(packed), p(staged.device), 5, 0, p(dst), 36, 52, p(b), None, 40, None, None, 20, None, 0, s) == -1
    assert b'without' in L.yr_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()


# ----------------------------------------------------------------------------- AugmentedDataset end to end
HW, C, S = (96, 96), 20, 3


def _dataset_setup(tmp):
    from PIL import Image
    png = tmp / 'third.png'
    Image.fromarray(np.random.RandomState(11).randint(0, 256, size=(61, 45, 3)).astype(np.uint8)).save(str(png))
    paths = [os.path.join(GOLDEN, 'demo_2011_001694.jpg'), os.path.join(GOLDEN, 'demo_2011_002558.jpg'), str(png)]
    decoded = {p: np.array(Image.open(p).convert('RGB'), dtype=np.uint8) for p in paths}
    lines = []
    for k, p in enumerate(paths):
        ih, iw = decoded[p].shape[:2]
        bb = [[int(.1 * iw), int(.2 * ih), int(.6 * iw), int(.9 * ih), 3 + k], [int(.5 * iw), int(.1 * ih), int(.95 * iw), int(.5 * ih), 11],
              [int(.3 * iw), int(.3 * ih), int(.3 * iw) + 2, int(.8 * ih), 5]]
        lines.append(p + ' ' + ' '.join('%d %d %d %d %d' % tuple(r) for r in bb))
    labels = tmp / 'train_3.txt'
    labels.write_text('\n'.join(lines) + '\n')
    return str(labels), decoded


def test_augmented_dataset_end_to_end(dev, tmp_path):
    from yoloret_amd.yolo3.data import AugmentedDataset
    from yoloret_amd.yolo3.utils import preprocess_true_boxes
    labels, decoded = _dataset_setup(tmp_path)

    def run(seed, passes):
        ds = AugmentedDataset(labels, 2, ANCHORS, C, HW, S, seed=seed, device=dev)
        it, num = ds.build()
        assert num == 3
        out = []
        for _ in range(passes):
            for x, y_true in it:
                torch.cuda.synchronize()
                out.append((x.cpu().numpy(), [y.cpu().numpy() for y in y_true], ds.last_boxes[0].cpu().numpy(), ds.last_boxes[1].cpu().tolist(),
                            ds.last_draws.copy()))
        return out
    first, again = run(3, 3), run(3, 3)
    assert [b[0].shape[0] for b in first] == [2, 1] * 3
    for a, b in zip(first, again):      # the same seed: the same bytes
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a[1], b[1]))
        assert np.array_equal(a[4], b[4])
    # the passes differ in order or, where a permutation repeats, in the draws
    assert not all(np.array_equal(first[0][4], first[k][4]) for k in (2, 4))
    # decode -> restatement -> host preprocess_true_boxes, with the records and draws AugmentedDataset plans (host side, same seed)
    ds = AugmentedDataset(labels, 2, ANCHORS, C, HW, S, seed=3, device=dev)
    it, _ = ds.build()
    orders = []
    at = 0
    labelled = 0
    for _ in range(3):
        plan = ds.epoch_plan(it.files, it.rng)
        orders.append([int(bb[0, 4]) for recs, _ in plan for _, bb in recs])
        for recs, draws in plan:
            x, y_true, boxes_out, kept, got_draws = first[at]
            at += 1
            assert np.array_equal(draws, got_draws)
            for i, (path, bb) in enumerate(recs):
                im = decoded[path]
                g = ar.geometry(im.shape[0], im.shape[1], HW, draws[i], ALL)
                want64 = ar.image(im, HW, g, ALL, np.float64)
                want32 = ar.image(im, HW, g, ALL)
                bound = max(4 * float(np.abs(want32.astype(np.float64) - want64).max()), 4 * 2.0 ** -24)
                assert float(np.abs(x[i].astype(np.float64) - want64).max()) <= bound, path
                rows, n, _ = ar.map_boxes(bb, g, HW)
                assert kept[i] == n and np.array_equal(_bits(boxes_out[i]), _bits(rows))
                want_y = preprocess_true_boxes(rows, HW, ANCHORS, C, S)
                for s in range(S):
                    assert np.array_equal(_bits(y_true[s][i]), _bits(want_y[s])), 'y_true scale %d of %s' % (s, path)
                    labelled += int((want_y[s][..., 4] != 0).sum())
    assert at == 6 and labelled >= 3
    assert len({tuple(o) for o in orders}) >= 2, orders      # two passes give different orders
