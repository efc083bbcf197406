"""The ragged batched ingest on the device (yoloret_amd/csrc/ingest.hip behind yr_ingest_batch) against the existing letterbox,
the oracle and tests/valdata_ref.py.  Every call of the C entry runs between the guards of tests/fence.py: dst, boxes_out and
kept are written tensors, pre-filled with NaN / a sentinel; the packed source, the table, the boxes and the counts are read
tensors.  All comparisons are on raw bytes.

Shapes: outputs 96x96 and 64x128; batches of 1 and 7 over the sources below - up- and down-scaling, windows touching each
border, offsets behind odd-sized images, the smallest image last but one and a 3-pixel-wide one last."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fence, valdata_ref as vr

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(96, 96), (64, 128)]
SOURCES = [(33, 47), (47, 33), (96, 96), (5, 7), (200, 13), (1, 1), (130, 3)]
SENTINEL = -77
_cache = {}


def _images():
    if 'img' not in _cache:
        rs = np.random.RandomState(7)
        imgs = [rs.randint(0, 256, size=d + (3,)).astype(np.uint8) for d in SOURCES]
        imgs[0][0, 0] = (0, 255, 255)
        imgs[2][-1, -1] = (255, 0, 255)
        _cache['img'] = imgs
    return _cache['img']


def _expected(size, mode):
    """The reference images of all sources, computed once per (size, mode) and left unchanged."""
    key = ('exp', size, mode)
    if key not in _cache:
        from oracle.preprocess import letterbox_image
        out = [vr.validate_image(im, size) if mode == 1 else letterbox_image(im, size)[0] for im in _images()]
        for o in out:
            o.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _pack(images, size, mode, dev, fill=0xA5):
    """-> (table, packed source on the device, table bytes on the device): the staging a caller does, byte by byte."""
    from yoloret_amd import runtime as rt
    table = rt.ingest_geometry([im.shape[:2] for im in images], size, mode)
    buf = np.full(table.packed_bytes, fill, np.uint8)      # the padding between images must not matter
    for im, off in zip(images, table.host['src_off']):
        buf[off:off + im.size] = im.reshape(-1)
    table.upload(dev)
    return table, torch.from_numpy(buf).to(dev), table.device


def _ingest(dev, table, src, tab, size, boxes=None, counts=None, max_boxes=20, with_kept=True):
    """One fenced call of yr_ingest_batch -> (dst, boxes_out, kept); the outputs start as NaN / SENTINEL."""
    from yoloret_amd import runtime as rt
    L = rt.lib()
    b, (h, w) = table.batch, size
    dst = torch.full((b, h, w, 3), float('nan'), dtype=torch.float32, device=dev)
    boxes_out = kept = None
    max_in = 0
    if boxes is not None:
        max_in = boxes.shape[1]
        boxes_out = torch.full((b, max_boxes, 5), float('nan'), dtype=torch.float32, device=dev)
        kept = torch.full((b,), SENTINEL, dtype=torch.int32, device=dev) if with_kept else None

    def call(moved):
        p = lambda t: rt._ptr(moved(t)) if t is not None else None
        rt.check(L.yr_ingest_batch(table.mode, p(src), p(tab), b, p(dst), h, w, p(boxes), p(counts), max_in, p(boxes_out), p(kept),
                                   max_boxes, rt.stream_ptr(dev)))
    fence.run(call, writes=[dst, boxes_out, kept], reads=[src, tab, boxes, counts], batch=b)
    torch.cuda.synchronize()
    return dst, boxes_out, kept


# ----------------------------------------------------------------------------- images
@pytest.mark.parametrize('mode', [0, 1], ids=['letterbox', 'validate'])
@pytest.mark.parametrize('size', SIZES, ids=['96x96', '64x128'])
def test_images_batch_of_7_and_batches_of_1(dev, size, mode):
    from yoloret_amd import runtime as rt
    images, want = _images(), _expected(size, mode)
    table, src, tab = _pack(images, size, mode, dev)
    assert table.host['src_off'][1] % 16 == 0 and table.host['src_off'][1] != images[0].size      # an offset behind an odd-sized image
    dst, _, _ = _ingest(dev, table, src, tab, size)
    got = dst.cpu().numpy()
    for i, im in enumerate(images):
        assert np.array_equal(_bits(got[i]), _bits(want[i])), 'batch of 7, image %d %s' % (i, SOURCES[i])
        if mode == rt.INGEST_LETTERBOX:
            one = rt.letterbox(torch.from_numpy(im).to(dev), size)
            assert np.array_equal(_bits(one), _bits(got[i])), 'yr_letterbox, image %d %s' % (i, SOURCES[i])
    for i, im in enumerate(images):
        t1, s1, g1 = _pack([im], size, mode, dev, fill=0x3C)
        d1, _, _ = _ingest(dev, t1, s1, g1, size)
        assert np.array_equal(_bits(d1[0]), _bits(want[i])), 'batch of 1, image %d %s' % (i, SOURCES[i])


def test_the_two_rules_differ_on_at_least_three_sources(dev):
    size = (96, 96)
    a, b = _expected(size, 0), _expected(size, 1)
    differ = [SOURCES[i] for i in range(len(SOURCES)) if not np.array_equal(_bits(a[i]), _bits(b[i]))]
    print('sources on which LETTERBOX and VALIDATE differ at 96x96:', differ)
    assert len(differ) >= 3 and {(33, 47), (5, 7), (200, 13)} <= set(differ)
    images = _images()
    outs = []
    for mode in (0, 1):
        table, src, tab = _pack(images, size, mode, dev)
        outs.append(_ingest(dev, table, src, tab, size)[0].cpu().numpy())
    got = [SOURCES[i] for i in range(len(SOURCES)) if not np.array_equal(_bits(outs[0][i]), _bits(outs[1][i]))]
    assert got == differ


def test_output_size_that_is_no_multiple_of_four(dev):
    """B * H * W = 3 * 7 * 9 = 189 pixels: the last lane writes one pixel with scalar stores, quads cross rows and images."""
    from oracle.preprocess import letterbox_image
    size = (7, 9)
    images = _images()[:3]
    for mode in (0, 1):
        table, src, tab = _pack(images, size, mode, dev)
        got = _ingest(dev, table, src, tab, size)[0].cpu().numpy()
        for i, im in enumerate(images):
            want = vr.validate_image(im, size) if mode == 1 else letterbox_image(im, size)[0]
            assert np.array_equal(_bits(got[i]), _bits(want)), (mode, i)


# ----------------------------------------------------------------------------- boxes
def _extent(lo, hi, dims, size, axis):
    """The mapped, clipped extent of a box whose `axis` runs from lo to hi on a source of `dims` (the other axis is wide)."""
    ih, iw = dims
    row = np.array([[lo, 0.1 * ih, hi, 0.9 * ih, 0]] if axis == 0 else [[0.1 * iw, lo, 0.9 * iw, hi, 0]], F)
    info = vr.map_boxes(row, ih, iw, size)[2]
    return (info['w'] if axis == 0 else info['h'])[0]


def _edge_pair(dims, size, axis):
    """(lo, hi_drop, hi_keep): with the reference on the CPU, a box whose mapped extent along `axis` is EXACTLY 1.0 (dropped) and the
    next float32 above hi_drop, whose extent is the next value above 1 or more (kept); None where no start gives exactly 1.0."""
    n_src = dims[1 - axis]
    g = vr.validate_geometry(dims[0], dims[1], size)
    n_f = float(g[5] if axis == 0 else g[4])
    for lo in (0.0, 1.0, 2.0, 10.0, 0.25 * n_src):
        lo = F(lo)
        hi = F(float(lo) + n_src / n_f)
        for _ in range(400):
            if not _extent(lo, hi, dims, size, axis) > 1:
                break
            hi = np.nextafter(hi, F(-np.inf))
        for _ in range(400):
            up = np.nextafter(hi, F(np.inf))
            if _extent(lo, up, dims, size, axis) > 1:
                break
            hi = up
        else:
            continue
        if _extent(lo, hi, dims, size, axis) == 1 and _extent(lo, up, dims, size, axis) > 1:
            return lo, hi, up
    return None


def _box_case(size, max_in):
    """Rows and counts of the 7 sources.  Image 0: full; image 1: count 0 (its rows must not be read as boxes); image 6: only
    degenerate rows (nothing kept with a count > 0).  Edge rows go to the sources on which the reference finds them."""
    key = ('boxes', size, max_in)
    if key in _cache:
        return _cache[key]
    rs = np.random.RandomState(100 + max_in)
    boxes = np.zeros((len(SOURCES), max_in, 5), F)
    counts = np.zeros(len(SOURCES), np.int32)
    edges = {'w': 0, 'h': 0}
    for i, (ih, iw) in enumerate(SOURCES):
        rows = [[0.2 * iw, 0.2 * ih, 0.8 * iw, 0.8 * ih, 3],
                [-5, 0.2 * ih, 0.5 * iw, 0.8 * ih, 1], [0.5 * iw, 0.2 * ih, iw + 50, 0.8 * ih, 2],      # clipped left, right
                [0.2 * iw, -9, 0.8 * iw, 0.5 * ih, 4], [0.2 * iw, 0.5 * ih, 0.8 * iw, ih + 70, 5]]      # clipped top, bottom
        for axis, name in ((0, 'w'), (1, 'h')):
            e = _edge_pair((ih, iw), size, axis)
            if e is not None:
                lo, drop, keep = e
                edges[name] += 1
                for hi in (drop, keep):
                    rows.append([lo, 0.1 * ih, hi, 0.9 * ih, 6] if axis == 0 else [0.1 * iw, lo, 0.9 * iw, hi, 7])
        if i == 6:
            rows = [[1, 1, 1, 100, 8], [0, 5, 3, 5, 9], [2, 2, 1, 1, 10]]      # zero width, zero height, negative extent
        while len(rows) < max_in:
            x = np.sort(rs.uniform(-0.2 * iw, 1.2 * iw, 2))
            y = np.sort(rs.uniform(-0.2 * ih, 1.2 * ih, 2))
            rows.append([x[0], y[0], x[1], y[1], rs.randint(0, 20)])
        if max_in < len(rows):      # small max_in: rotate, so that different kinds of rows lead on different images
            rows = rows[i % len(rows):] + rows[:i % len(rows)]
        boxes[i] = np.asarray(rows[:max_in], F)
        counts[i] = max_in if i in (0, 6) else (0 if i == 1 else rs.randint(0, max_in + 1))
    counts[6] = min(3, max_in)
    boxes.setflags(write=False)
    _cache[key] = (boxes, counts, edges)
    return _cache[key]


@pytest.mark.parametrize('max_boxes', [20, 1])
@pytest.mark.parametrize('max_in', [1, 20, 21, 64, 65, 256])
@pytest.mark.parametrize('size', SIZES, ids=['96x96', '64x128'])
def test_boxes(dev, size, max_in, max_boxes):
    from yoloret_amd import runtime as rt
    images = _images()
    boxes, counts, edges = _box_case(size, max_in)
    want, want_kept, seen = [], [], {'drop_w_exact': 0, 'drop_h_exact': 0, 'kept_just_above': 0, 'cap': 0, 'nothing': 0}
    for i, (ih, iw) in enumerate(SOURCES):
        out, kept, info = vr.map_boxes(boxes[i, :counts[i]], ih, iw, size, max_boxes)
        want.append(out)
        want_kept.append(kept)
        above = np.nextafter(F(1), F(2))
        seen['drop_w_exact'] += int((info['w'] == 1).sum())
        seen['drop_h_exact'] += int(((info['w'] > 1) & (info['h'] == 1)).sum())
        seen['kept_just_above'] += int((((info['w'] > 1) & (info['w'] <= F(1.0001))) | ((info['h'] > 1) & (info['h'] <= F(1.0001)))).sum())
        seen['cap'] += int(info['passed'] > max_boxes)
        seen['nothing'] += int(counts[i] > 0 and kept == 0)
        assert above > 1
    print('size %s max_in %d max_boxes %d: counts %s kept %s, reference branches %s, edge sources %s'
          % (size, max_in, max_boxes, counts.tolist(), want_kept, seen, edges))
    if max_in >= 64:     # the reference itself must take every branch (with few rows the leading ones are the plain boxes)
        assert edges['w'] >= 1 and edges['h'] >= 1
        assert seen['drop_w_exact'] >= 1 and seen['drop_h_exact'] >= 1 and seen['kept_just_above'] >= 2, seen
        assert seen['cap'] >= 1 and seen['nothing'] >= 1, seen
        assert counts[0] == max_in and counts[1] == 0
    table, src, tab = _pack(images, size, rt.INGEST_VALIDATE, dev)
    dst, boxes_out, kept = _ingest(dev, table, src, tab, size, torch.from_numpy(np.array(boxes)).to(dev), torch.from_numpy(counts).to(dev), max_boxes)
    assert kept.cpu().tolist() == want_kept
    got = boxes_out.cpu().numpy()
    for i in range(len(SOURCES)):
        assert np.array_equal(_bits(got[i]), _bits(want[i])), 'image %d %s: %s != %s' % (i, SOURCES[i], got[i, :3], want[i][:3])
    ref = _expected(size, 1)
    img = dst.cpu().numpy()
    assert all(np.array_equal(_bits(img[i]), _bits(ref[i])) for i in range(len(SOURCES)))      # the image part is the same with boxes


def test_boxes_without_kept_and_label_bits(dev):
    """kept may be null; the label's bits are copied through (a NaN payload, -0.0, a fraction)."""
    from yoloret_amd import runtime as rt
    size = (96, 96)
    images = _images()[:2]
    boxes = np.zeros((2, 3, 5), F)
    boxes[0, :, :4] = (5, 5, 30, 30)
    boxes[1, :, :4] = (2, 2, 40, 40)
    labels = np.array([0x7fc01234, 0x80000000, 0x3fc00000, 0xffffffff, 0x00000001, 0x41a00000], np.uint32)
    boxes.view(np.uint32)[:, :, 4] = labels.reshape(2, 3)
    table, src, tab = _pack(images, size, rt.INGEST_VALIDATE, dev)
    counts = torch.tensor([3, 3], dtype=torch.int32, device=dev)
    _, boxes_out, kept = _ingest(dev, table, src, tab, size, torch.from_numpy(boxes).to(dev), counts, 20, with_kept=False)
    assert kept is None
    got = boxes_out.cpu().numpy().view(np.uint32)
    assert got[:, :3, 4].reshape(-1).tolist() == labels.tolist() and not got[:, 3:].any()


# ----------------------------------------------------------------------------- stager, reproducibility, wrapper
def test_two_batches_back_to_back_through_the_stager(dev):
    """Two different batches are staged one right after the other, before anything is waited for: the second packing must not
    overtake the first copy.  Then both are ingested (fenced) and compared; the wrapper gives the same bytes."""
    from yoloret_amd import runtime as rt
    size = (96, 96)
    images = _images()
    first, second = images[:4], [images[6], images[4], images[2]]
    stager = rt.RaggedStager(dev)
    big = [np.random.RandomState(3).randint(0, 256, size=(700, 900, 3)).astype(np.uint8)]      # a copy that takes a while
    pa, ta = stager.upload(big + first, size, rt.INGEST_VALIDATE)
    pb, tb = stager.upload(second, size, rt.INGEST_LETTERBOX)
    assert stager._host.is_pinned() and pa.data_ptr() % 16 == 0 and ta.device.data_ptr() % 16 == 0
    da = _ingest(dev, ta, pa, ta.device, size)[0].cpu().numpy()
    db = _ingest(dev, tb, pb, tb.device, size)[0].cpu().numpy()
    assert np.array_equal(_bits(da[0]), _bits(vr.validate_image(big[0], size)))
    for i in range(4):
        assert np.array_equal(_bits(da[1 + i]), _bits(_expected(size, 1)[i])), i
    for k, i in enumerate((6, 4, 2)):
        assert np.array_equal(_bits(db[k]), _bits(_expected(size, 0)[i])), i
    wa = rt.ingest_batch(pa, ta, size)
    wb = rt.ingest_batch(pb, tb, size, out=torch.empty((3, 96, 96, 3), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(wa), _bits(da)) and np.array_equal(_bits(wb), _bits(db))
    # the buffer is reused, not reallocated, for a batch that fits
    host = stager._host.data_ptr()
    stager.upload(second, size, rt.INGEST_LETTERBOX)
    assert stager._host.data_ptr() == host
    torch.cuda.synchronize()


def test_same_call_twice_gives_the_same_bytes(dev):
    from yoloret_amd import runtime as rt
    size = (64, 128)
    boxes, counts, _ = _box_case(size, 65)
    table, src, tab = _pack(_images(), size, rt.INGEST_VALIDATE, dev)
    b, c = torch.from_numpy(np.array(boxes)).to(dev), torch.from_numpy(counts).to(dev)
    one = _ingest(dev, table, src, tab, size, b, c, 20)
    two = _ingest(dev, table, src, tab, size, b, c, 20)
    for x, y in zip(one, two):
        assert np.array_equal(_bits(x), _bits(y))
    wx, wb, wk = rt.ingest_batch(src, table, size, boxes=b, box_count=c, max_boxes=20)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(wx), _bits(one[0])) and np.array_equal(_bits(wb), _bits(one[1])) and wk.cpu().tolist() == one[2].cpu().tolist()


def test_argument_errors_leave_the_outputs_alone(dev):
    from yoloret_amd import runtime as rt
    L = rt.lib()
    size = (96, 96)
    images = _images()[:2]
    boxes = torch.zeros((2, 4, 5), dtype=torch.float32, device=dev)
    counts = torch.zeros((2,), dtype=torch.int32, device=dev)
    lb, src, tab = _pack(images, size, rt.INGEST_LETTERBOX, dev)
    with pytest.raises(rt.YoloretHipError, match='VALIDATE mode only'):      # LETTERBOX with boxes, at the C entry
        _ingest(dev, lb, src, tab, size, boxes, counts)
    with pytest.raises(ValueError, match='VALIDATE mode only'):               # ... and at the wrapper
        rt.ingest_batch(src, lb, size, boxes=boxes, box_count=counts)
    va, src, tab = _pack(images, size, rt.INGEST_VALIDATE, dev)
    many = torch.zeros((2, 257, 5), dtype=torch.float32, device=dev)
    with pytest.raises(rt.YoloretHipError, match='max_in'):
        _ingest(dev, va, src, tab, size, many, counts)
    with pytest.raises(ValueError, match='max_in'):
        rt.ingest_batch(src, va, size, boxes=many, box_count=counts)
    dst = torch.full((2, 96, 96, 3), float('nan'), dtype=torch.float32, device=dev)
    out = torch.full((2, 20, 5), float('nan'), dtype=torch.float32, device=dev)
    p, s = rt._ptr, rt.stream_ptr(dev)
    for args in ((None, p(tab), p(dst), p(boxes), p(counts), p(out)), (p(src), None, p(dst), p(boxes), p(counts), p(out)),
                 (p(src), p(tab), None, p(boxes), p(counts), p(out)), (p(src), p(tab), p(dst), p(boxes), None, p(out)),
                 (p(src), p(tab), p(dst), p(boxes), p(counts), None)):
        rc = L.yr_ingest_batch(1, args[0], args[1], 2, args[2], 96, 96, args[3], args[4], 4, args[5], None, 20, s)
        assert rc == -1 and (b'null' in L.yr_last_error() or b'without' in L.yr_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(dst).all() and torch.isnan(out).all()
    with pytest.raises(ValueError, match='uploaded IngestTable'):
        rt.ingest_batch(src, rt.ingest_geometry([(5, 7)], size, 0), size)
    with pytest.raises(ValueError, match='computed for'):
        rt.ingest_batch(src, va, (64, 128))
    assert ctypes.sizeof(rt.YrIngestGeom) == 64
