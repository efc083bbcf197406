"""The validation data path without a GPU: what the header declares and the library exports (yr_ingest_geometry, yr_ingest_batch),
the geometry entry - pure host arithmetic - swept against tests/valdata_ref.py and the oracle, the yardstick itself pinned by
answers derived by hand, and Dataset's error paths and deterministic order.  tests/test_gpu_ingest.py and test_gpu_valdata.py
hold the parity tests."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import valdata_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ----------------------------------------------------------------------------- the yardstick, by hand
# (ih, iw) at 96x96 -> VALIDATE (nh, nw, dy, dx), letterbox_image (nh, nw, dy, dx)
HAND = [((33, 47), (67, 96, 14, 0), (67, 95, 14, 0)),
        ((5, 7), (68, 96, 13, 0), (68, 96, 14, 0)),
        ((200, 13), (96, 6, 0, 44), (96, 6, 0, 45))]


@pytest.mark.parametrize('dims,validate,letterbox', HAND, ids=['33x47', '5x7', '200x13'])
def test_reference_geometries_by_hand(dims, validate, letterbox):
    from oracle.preprocess import letterbox_image
    assert vr.validate_geometry(dims[0], dims[1], (96, 96))[:4] == validate
    assert vr.letterbox_geometry(dims[0], dims[1], (96, 96)) == letterbox
    assert letterbox_image(np.zeros(dims + (3,), np.uint8), (96, 96))[1] == letterbox
    assert validate != letterbox


def test_reference_boxes_by_hand():
    """A 375x500 image at 416: m = fl(416/500), nw_f = 416, nh_f = 312, dy_f = 52, dx_f = 0.  The box (100, 50, 300, 250) maps to
    x = 100 * 416 / 500 = fl(83.2) and 300 * 416 / 500 = fl(249.6) (exact products, one rounded division), y = fl(fl(41.6) + 52) and
    250 * 312 / 375 + 52 = 260 exactly."""
    nh, nw, dy, dx, nh_f, nw_f, dy_f, dx_f = vr.validate_geometry(375, 500, (416, 416))
    assert (nh, nw, dy, dx) == (312, 416, 52, 0)
    assert (nh_f, nw_f, dy_f, dx_f) == (F(312), F(416), F(52), F(0)) and all(type(v) is F for v in (nh_f, nw_f, dy_f, dx_f))
    boxes = np.array([[100, 50, 300, 250, 7],      # kept
                      [10, 10, 11, 200, 3],        # mapped width 0.832: dropped
                      [-50, -20, 700, 500, 1],     # clipped on all four sides: (0, 36, 415, 415)
                      [20, 30, 200, 31, 2]], F)    # mapped height 0.832: dropped
    out, kept, info = vr.map_boxes(boxes, 375, 500, (416, 416))
    assert kept == 2 and info['drop_w'] == 1 and info['drop_h'] == 1
    assert tuple(out[0]) == (F(83.2), F(F(41.6) + F(52)), F(249.6), F(260), F(7))
    assert tuple(out[1]) == (F(0), F(F(-20) * F(312) / F(375) + F(52)), F(415), F(415), F(1))
    assert not out[2:].any()
    # the cap: 25 copies of the first row -> 20
    out, kept, info = vr.map_boxes(np.repeat(boxes[:1], 25, axis=0), 375, 500, (416, 416))
    assert kept == 20 and info['passed'] == 25 and (out == out[0]).all()


# ----------------------------------------------------------------------------- ABI
def test_c_abi_declares_exports_and_builds_the_ingest():
    from yoloret_amd import build, runtime as rt
    header = open(os.path.join(ROOT, 'include', 'yoloret_hip.h')).read()
    assert re.search(r'\bint\s+yr_ingest_geometry\s*\(', header) and re.search(r'\bint\s+yr_ingest_batch\s*\(', header)
    assert re.search(r'^#define\s+YR_INGEST_LETTERBOX\s+0\b', header, re.M) and rt.INGEST_LETTERBOX == 0
    assert re.search(r'^#define\s+YR_INGEST_VALIDATE\s+1\b', header, re.M) and rt.INGEST_VALIDATE == 1
    assert re.search(r'^#define\s+YR_INGEST_MAX_BOXES\s+256\b', header, re.M) and rt.INGEST_MAX_BOXES == 256
    assert re.search(r'\}\s*yr_ingest_geom\s*;', header)
    assert 'yr_ingest_geometry' in rt.EXPORTS and 'yr_ingest_batch' in rt.EXPORTS and 'ingest.hip' in build.SOURCES
    assert rt.ABI_VERSION == 9 and re.search(r'^#define\s+YR_ABI_VERSION\s+9\b', header, re.M)
    L = ctypes.CDLL(build.build())
    assert hasattr(L, 'yr_ingest_geometry') and hasattr(L, 'yr_ingest_batch')
    L.yr_abi_sizeof.argtypes = [ctypes.c_int]
    assert L.yr_abi_sizeof(3) == 64 == ctypes.sizeof(rt.YrIngestGeom) == rt.INGEST_GEOM_DTYPE.itemsize
    assert [(n, rt.INGEST_GEOM_DTYPE.fields[n][1]) for n in rt.INGEST_GEOM_DTYPE.names] == \
        [(n, getattr(rt.YrIngestGeom, n).offset) for n, _ in rt.YrIngestGeom._fields_]
    rt.lib()    # the binding's own load-time checks


def test_image_kernel_does_not_spill():
    from yoloret_amd import build as b
    b.build()
    rows = b.kernel_resources()['ingest.hip']
    assert len(rows) == 1 and 'ingest_kernel' in rows[0][0]
    assert rows[0][2] == 0, 'ingest_kernel keeps %d bytes per lane in scratch' % rows[0][2]


# ----------------------------------------------------------------------------- yr_ingest_geometry
SIZES = [(96, 96), (64, 128)]


@pytest.mark.parametrize('size', SIZES, ids=['96x96', '64x128'])
@pytest.mark.parametrize('mode', [0, 1], ids=['letterbox', 'validate'])
def test_geometry_sweep(size, mode):
    """Every (ih, iw) in 1..130 x 1..130 in one call per mode: == valdata_ref, in LETTERBOX mode also == the oracle's tuple;
    sizes that collapse are refused one by one, naming the image."""
    from oracle.preprocess import letterbox_image
    from yoloret_amd import runtime as rt
    dims = [(ih, iw) for ih in range(1, 131) for iw in range(1, 131)]
    if mode == rt.INGEST_VALIDATE:
        want = [vr.validate_geometry(ih, iw, size) for ih, iw in dims]
    else:
        want = [vr.letterbox_geometry(ih, iw, size) + (F(0),) * 4 for ih, iw in dims]
    good = [i for i, g in enumerate(want) if g[0] > 0 and g[1] > 0]
    bad = [i for i, g in enumerate(want) if not (g[0] > 0 and g[1] > 0)]
    assert len(good) > 16000 and len(bad) > 50
    table = rt.ingest_geometry([dims[i] for i in good], size, mode)
    t = table.host
    assert t.shape == (len(good),) and table.mode == mode and table.input_hw == size
    got = list(zip(t['nh'].tolist(), t['nw'].tolist(), t['dy'].tolist(), t['dx'].tolist()))
    assert got == [want[i][:4] for i in good]
    for k, name in enumerate(('nh_f', 'nw_f', 'dy_f', 'dx_f')):
        assert np.array_equal(t[name].view(np.uint32), np.array([want[i][4 + k] for i in good], F).view(np.uint32)), name
    assert [tuple(d) for d in zip(t['ih'].tolist(), t['iw'].tolist())] == [dims[i] for i in good] and not t['reserved'].any()
    # offsets: 16-aligned, in order, non-overlapping, the end rounded up
    off = t['src_off'].astype(np.int64)
    nbytes = np.array([dims[i][0] * dims[i][1] * 3 for i in good], np.int64)
    assert off[0] == 0 and not (off % 16).any() and (off[1:] >= off[:-1] + nbytes[:-1]).all() and (off[1:] < off[:-1] + nbytes[:-1] + 16).all()
    assert table.packed_bytes % 16 == 0 and 0 <= table.packed_bytes - (off[-1] + nbytes[-1]) < 16
    if mode == rt.INGEST_LETTERBOX:     # the oracle's own tuple, on a subset (it resizes a real image)
        for i in good[::97]:
            assert letterbox_image(np.zeros(dims[i] + (3,), np.uint8), size)[1] == got[good.index(i)]
    for i in bad[::7] + bad[-1:]:
        with pytest.raises(rt.YoloretHipError, match=r'image 1 \(%dx%d\) collapses' % dims[i]):
            rt.ingest_geometry([(33, 47), dims[i]], size, mode)


def test_geometry_modes_differ_for_about_half_of_the_sizes():
    from yoloret_amd import runtime as rt
    rs = np.random.RandomState(0)
    dims = [d for d in rs.randint(5, 600, size=(2000, 2)).tolist()      # (sizes that collapse under either rule are left out)
            if min(vr.letterbox_geometry(d[0], d[1], (96, 96))[:2] + vr.validate_geometry(d[0], d[1], (96, 96))[:2]) > 0]
    assert len(dims) > 1800
    a =rt.ingest_geometry(dims, (96, 96), rt.INGEST_LETTERBOX).host
    b = rt.ingest_geometry(dims, (96, 96), rt.INGEST_VALIDATE).host
    differ = sum(any(a[n][i] != b[n][i] for n in ('nh', 'nw', 'dy', 'dx')) for i in range(len(dims)))
    assert 0.3 < differ / len(dims) < 0.7, differ


def test_geometry_by_hand_through_the_library():
    from yoloret_amd import runtime as rt
    dims = [d for d, _, _ in HAND]
    for mode, col in ((rt.INGEST_VALIDATE, 1), (rt.INGEST_LETTERBOX, 2)):
        t = rt.ingest_geometry(dims, (96, 96), mode).host
        assert [(int(g['nh']), int(g['nw']), int(g['dy']), int(g['dx'])) for g in t] == [h[col] for h in HAND]
    t = rt.ingest_geometry([(375, 500)], (416, 416), rt.INGEST_VALIDATE).host[0]
    assert (t['nh_f'], t['nw_f'], t['dy_f'], t['dx_f']) == (312, 416, 52, 0)


def test_geometry_argument_errors():
    from yoloret_amd import runtime as rt
    L = rt.lib()
    dims = np.array([[33, 47]], np.int32)
    geom = np.zeros(1, rt.INGEST_GEOM_DTYPE)
    packed = ctypes.c_int64(-1)

    def call(mode=0, batch=1, d=dims.ctypes.data, h=96, w=96, g=geom.ctypes.data):
        return L.yr_ingest_geometry(mode, batch, d, h, w, g, ctypes.byref(packed))
    assert call() == 0 and packed.value == 33 * 47 * 3 + 16 - (33 * 47 * 3) % 16
    for kw in ({'mode': 2}, {'batch': 0}, {'d': None}, {'g': None}, {'h': 0}, {'w': -1}):
        assert call(**kw) == -1, kw
        assert b'ingest_geometry' in L.yr_last_error()
    zero = np.array([[0, 47]], np.int32)
    assert call(d=zero.ctypes.data) == -1 and b'image 0' in L.yr_last_error()
    with pytest.raises(ValueError, match='no image'):
        rt.ingest_geometry([], (96, 96), 0)


def test_batch_entry_refuses_before_the_device_is_touched():
    """Nothing is launched on an argument error, so fake pointers do."""
    from yoloret_amd import runtime as rt
    L = rt.lib()
    p = 0x10000

    def call(mode=1, src=p, geom=p, batch=2, dst=p, h=96, w=96, boxes=p, count=p, max_in=20, out=p, kept=p, max_boxes=20):
        return L.yr_ingest_batch(mode, src, geom, batch, dst, h, w, boxes, count, max_in, out, kept, max_boxes, None)
    for kw, word in (({'mode': 0}, b'VALIDATE mode only'), ({'max_in': 257}, b'max_in'), ({'max_in': 0}, b'max_in'), ({'src': None}, b'null'),
                     ({'geom': None}, b'null'), ({'dst': None}, b'null'), ({'count': None}, b'box_count'), ({'out': None}, b'boxes_out'),
                     ({'max_boxes': 0}, b'max_boxes'), ({'batch': 0}, b'bad arguments'), ({'h': 0}, b'bad arguments'), ({'mode': 5}, b'mode'),
                     ({'dst': p + 4}, b'aligned'), ({'batch': 40000, 'h': 416, 'w': 416}, b'2\\^31')):
        assert call(**kw) == -1, kw
        assert re.search(word, L.yr_last_error()), (kw, L.yr_last_error())


def test_wrapper_errors_without_a_device():
    import torch
    from yoloret_amd import runtime as rt
    table = rt.ingest_geometry([(33, 47)], (96, 96), rt.INGEST_LETTERBOX)
    with pytest.raises(ValueError, match='uint8 CUDA'):
        rt.ingest_batch(torch.zeros(16, dtype=torch.uint8), table, (96, 96))


# ----------------------------------------------------------------------------- Dataset
def _dataset(**kw):
    from yoloret_amd.yolo3.data import Dataset
    from yoloret_amd.yolo3.enums import DATASET_MODE
    from tests.util import ANCHORS
    args = dict(anchors=ANCHORS, num_classes=20, input_shape=(96, 96), num_scales=3, mode=DATASET_MODE.VALIDATE)
    args.update(kw)
    return Dataset(args.pop('glob_path'), args.pop('batch_size', 2), **args)


def test_dataset_mode_values_are_the_reference_s():
    from yoloret_amd.yolo3.enums import DATASET_MODE
    assert [(m.name, m.value) for m in DATASET_MODE] == [('TRAIN', 0), ('VALIDATE', 1), ('TEST', 2)]


def test_dataset_constructor_is_the_reference_s():
    import inspect
    from yoloret_amd.yolo3.data import Dataset
    from yoloret_amd.yolo3.enums import DATASET_MODE
    p = inspect.signature(Dataset.__init__).parameters
    assert list(p)[1:] == ['glob_path', 'batch_size', 'anchors', 'num_classes', 'input_shape', 'num_scales', 'mode', 'zoom_in', 'device', 'root']
    assert p['mode'].default is DATASET_MODE.TRAIN and p['zoom_in'].default is False
    assert all(p[n].default is None for n in ('anchors', 'num_classes', 'input_shape', 'num_scales', 'device', 'root'))


def test_dataset_error_paths(tmp_path):
    from yoloret_amd.yolo3.enums import DATASET_MODE
    assert _dataset(glob_path=None).build() == (None, 0)
    with pytest.raises(ValueError, match='^No file found$'):
        _dataset(glob_path=str(tmp_path / '*.txt')).build()
    (tmp_path / 'labels.txt').write_text('a.jpg 1 2 3 4 0\n')
    with pytest.raises(ValueError, match='<name>_<number>.<extension>'):
        _dataset(glob_path=str(tmp_path / 'labels.txt')).build()
    (tmp_path / 'val_2.txt').write_text('a.jpg 1 2 3 4 0\nb.jpg\n')
    (tmp_path / 'rec_5.tfrecords').write_bytes(b'')
    with pytest.raises(NotImplementedError, match='TFRecord'):
        _dataset(glob_path=str(tmp_path / '*_*.*')).build()
    one = str(tmp_path / 'val_2.txt')
    with pytest.raises(NotImplementedError, match='TRAIN'):
        _dataset(glob_path=one, mode=DATASET_MODE.TRAIN).build()
    with pytest.raises(NotImplementedError, match='zoom'):
        _dataset(glob_path=one, zoom_in=True).build()
    for mode in (DATASET_MODE.VALIDATE, DATASET_MODE.TEST):
        it, num = _dataset(glob_path=one, mode=mode).build()
        assert num == 2 and it is not None


def test_dataset_order_and_batches_are_deterministic(tmp_path):
    """Files sorted, lines in order, batches of batch_size with a shorter last one; num is the sum of the numbers in the names."""
    (tmp_path / 'b_3.txt').write_text('b0.jpg 1 2 3 4 0\n\nb1.jpg\nb2.jpg 5 6 7 8 1 9 10 11 12 2\n')
    (tmp_path / 'a_4.txt').write_text('a0.jpg 1 2 3 4 5\na1.jpg 1 2 3 4 6\na2.jpg\na3.jpg 0 0 9 9 7\n')
    ds = _dataset(glob_path=str(tmp_path / '*.txt'), batch_size=3)
    it, num = ds.build()
    assert num == 7 and it.files == [str(tmp_path / 'a_4.txt'), str(tmp_path / 'b_3.txt')]
    for _ in range(2):
        batches = list(ds.record_batches(it.files))
        assert [[r[0] for r in b] for b in batches] == [['a0.jpg', 'a1.jpg', 'a2.jpg'], ['a3.jpg', 'b0.jpg', 'b1.jpg'], ['b2.jpg']]
    assert batches[0][2][1].shape == (0, 5) and batches[2][0][1].shape == (2, 5) and batches[2][0][1].dtype == np.float32
    assert batches[2][0][1].tolist() == [[5, 6, 7, 8, 1], [9, 10, 11, 12, 2]]
    # the iterable hands each batch of records to load_batch, in that order
    seen = []
    ds.load_batch = lambda records: seen.append([r[0] for r in records]) or len(seen)
    assert list(it) == [1, 2, 3] and seen == [[r[0] for r in b] for b in batches]
