"""The training data path without a GPU: the yardstick tests/augment_ref.py pinned by answers derived by hand, the host entry
yr_augment_geometry swept against it field for field, the colour kernels' known answers, the error paths, the seeded order of
AugmentedDataset, and the ABI.  tests/test_gpu_augment.py holds the parity tests."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import augment_cases as ac, augment_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
F = np.float32
REST = (.5,) * 5      # flip, hue, sat, gamma, contrast: not read by the geometry under test


# ----------------------------------------------------------------------------- geometry, by hand
# a = b = 1 for j1 = j2 = .5, so new_ar = W / H.  At 36x52 new_ar = 1.444 >= 1: nw = scale * 52, nh = max(scale / new_ar, 1) * 52.
#   scale(.1) = .25 + .1 * 1.75 = .425: ratio .294 -> 1 (clamped); nw = 22.1, nh = 52 > 36: crop y; dx = .3 * 29.9 = 8.97 -> pad x 8,
#                                       dy = .6 * (36 - 52) = -9.6 -> crop y 9, window min(36, 52) = 36 rows
#   scale(.9) = 1.825: ratio 1.2635 (no clamp); nw = 94.9, nh = 65.7; dx = .3 * -42.9 = -12.87 -> crop x 12; dy = .6 * -29.7 = -17.82 -> crop y 17
#   (.1, .9): a = .76, b = 1.24, new_ar = .8853 < 1; scale(.3) = .775; ratio .686 -> 1; nw = 1 * 36 = 36, nh = .775 * 36 = 27.9: pad only,
#                                       dx = .5 * 16 = 8, dy = .5 * 8.1 = 4.05 -> pad (4, 8)
#   all 0: a = b = .7, scale .25; nw = 13, nh = 52: crop y at 0, window 36 x 13 at (0, 0)
# At 52x36 new_ar = .6923 < 1: nw = max(scale * new_ar, 1) * 52, nh = scale * 52.
#   scale(.1) = .425: ratio -> 1; nw = 52 > 36: crop x; nh = 22.1; dx = .3 * -16 = -4.8 -> crop x 4; dy = .6 * 29.9 = 17.94 -> pad y 17
HAND = [((36, 52), (.5, .5, .1, .3, .6), dict(rh=52, wh=36, cy=9, py=0, rw=22, ww=22, cx=0, px=8, clamped=1), (52, 22.1), 'crop_y'),
        ((36, 52), (.5, .5, .9, .3, .6), dict(rh=65, wh=36, cy=17, py=0, rw=94, ww=52, cx=12, px=0, clamped=0), (65.7, 94.9), 'crop_xy'),
        ((36, 52), (.1, .9, .3, .5, .5), dict(rh=27, wh=27, cy=0, py=4, rw=36, ww=36, cx=0, px=8, clamped=1), (27.9, 36), 'pad'),
        ((36, 52), (0, 0, 0, 0, 0), dict(rh=52, wh=36, cy=0, py=0, rw=13, ww=13, cx=0, px=0, clamped=1), (52, 13), 'crop_y'),
        ((52, 36), (.5, .5, .1, .3, .6), dict(rh=22, wh=22, cy=0, py=17, rw=52, ww=36, cx=4, px=0, clamped=1), (22.1, 52), 'crop_x')]


def _table(dims, size, draws, **kw):
    from yoloret_amd import runtime as rt
    return rt.augment_geometry(dims, size, draws, **kw)


@pytest.mark.parametrize('size,five,want,floats,kind', HAND, ids=['36x52-crop_y', '36x52-crop_xy', '36x52-pad', '36x52-zeros', '52x36-crop_x'])
def test_geometry_by_hand(size, five, want, floats, kind):
    draws = np.array(five + REST, F)
    g = ar.geometry(61, 45, size, draws)
    t = _table([(61, 45)], size, draws[None]).host[0]
    for src, get in ((g, lambda k: g[k]), (t, lambda k: t[k])):
        assert {k: int(get(k)) for k in want} == want
        assert abs(float(get('nh_f')) - floats[0]) < 1e-4 and abs(float(get('nw_f')) - floats[1]) < 1e-4
    assert ar.window_kind(g, size) == kind
    assert all(type(g[k]) is F for k in ('nh_f', 'nw_f', 'dy_f', 'dx_f', 'hue6', 'sat', 'gamma', 'cont'))


def test_the_shared_draws_reach_every_branch():
    kinds, flips, clamps = ac.coverage()
    assert kinds == {'pad', 'crop_x', 'crop_y', 'crop_xy'} and flips == {0, 1} and clamps == {0, 1}


def _same(table_row, g):
    for k, v in g.items():
        got = table_row[k]
        if isinstance(v, F):
            assert got.dtype == F and got.view(np.uint32) == v.view(np.uint32), (k, got, v)
        else:
            assert int(got) == v, (k, got, v)


def test_table_equals_the_restatement_field_for_field():
    from yoloret_amd import runtime as rt
    rs = np.random.RandomState(5)
    n = bad = 0
    kinds = set()
    for trial in range(500):
        size = (int(rs.randint(8, 97)), int(rs.randint(8, 97)))
        b = 8
        dims = rs.randint(1, 300, size=(b, 2))
        draws = rs.random_sample((b, 10)).astype(F)
        stages = int(rs.randint(0, 32))
        params = {} if trial % 2 else dict(jitter=float(rs.uniform(0, .6)), min_scale=float(rs.uniform(.1, 1)), max_scale=float(rs.uniform(1, 3)),
                                           hue=float(rs.uniform(0, .5)), sat=float(rs.uniform(0, 1)), min_gamma=float(rs.uniform(.2, 1)),
                                           max_gamma=float(rs.uniform(1, 3)), cont=float(rs.uniform(0, 1)))
        want = []
        try:
            for i in range(b):
                want.append(ar.geometry(dims[i, 0], dims[i, 1], size, draws[i], stages, **params))
        except ValueError:
            bad += 1
            with pytest.raises(rt.YoloretHipError, match='image %d' % len(want)):
                _table(dims, size, draws, stages=stages, **params)
            continue
        t = _table(dims, size, draws, stages=stages, **params)
        off = 0
        for i in range(b):
            _same(t.host[i], want[i])
            assert t.host[i]['src_off'] == off and not t.host[i]['reserved'].any()
            off = (off + int(dims[i, 0]) * int(dims[i, 1]) * 3 + 15) // 16 * 16
            kinds.add(ar.window_kind(want[i], size))
            n += 1
        assert t.packed_bytes == off and t.stages == stages
    print('%d images compared, %d batches refused by both sides, window kinds %s' % (n, bad, sorted(kinds)))
    assert n >= 3000 and kinds == {'pad', 'crop_x', 'crop_y', 'crop_xy'}


def test_stage_mask_follows_the_reference_conditions():
    from yoloret_amd import runtime as rt
    assert rt.augment_stages() == rt.AUG_HUE | rt.AUG_SAT | rt.AUG_GAMMA | rt.AUG_CONTRAST == 15
    assert rt.augment_stages(flip=False, hue=0, sat=0, min_gamma=1, max_gamma=1, cont=0) == rt.AUG_NOFLIP
    draws = np.full((1, 10), .25, F)
    on, off = _table([(9, 9)], (36, 52), draws).host[0], _table([(9, 9)], (36, 52), draws, flip=False, hue=0, sat=0, min_gamma=2, cont=0).host[0]
    assert on['flip'] == 1 and off['flip'] == 0
    assert (off['hue6'], off['sat'], off['gamma'], off['cont']) == (0, 1, 1, 1)
    # delta = -.5 + .25 * 1 = -.25 -> -1.5; sat = .5 + .25 * 1; gamma = .8 + .25 * 1.2 = 1.1; cont = .9 + .25 * .2 = .95
    assert on['hue6'] == F(-1.5) and on['sat'] == F(.75) and abs(on['gamma'] - 1.1) < 1e-6 and abs(on['cont'] - .95) < 1e-6


# ----------------------------------------------------------------------------- colour, known answers
PRIMARIES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
GREYS = np.array([[0, 0, 0], [.25, .25, .25], [1, 1, 1], [F(1 / 255.0)] * 3], F)
TIES = np.array([[.5, .5, .2], [.2, .5, .5], [.5, .2, .5], [.7, .7, .7], [1, 1, 0], [0, 1, 1]], F)


def test_hue_known_answers():
    third = F(F(1 / 3.0) * F(6))      # delta = 1/3: exactly 2 sextants in float32
    assert third == F(2)
    assert np.array_equal(ar.adjust_hue(PRIMARIES, third), PRIMARIES[[1, 2, 0]])      # red -> green -> blue -> red
    assert np.array_equal(ar.adjust_hue(PRIMARIES, F(-2)), PRIMARIES[[2, 0, 1]])
    for d in (F(0), F(1.7), F(-3), F(2.999)):
        assert np.array_equal(ar.adjust_hue(GREYS, d), GREYS)      # v_max == v_min: every channel is v_min, whatever the hue
    # delta 0: v_max and v_min are copied; v_mid = v_min + ratio * range with ratio rebuilt from h = cat + ratio, one rounding at a
    # magnitude below 8 (half an ulp: 2^-22) on top of the division's and the product's: within 2^-21 in all
    rs = np.random.RandomState(1)
    x = np.concatenate([rs.random_sample((4000, 3)).astype(F), TIES, PRIMARIES])
    y = ar.adjust_hue(x, F(0))
    assert np.array_equal(y.max(axis=1), x.max(axis=1)) and np.array_equal(y.min(axis=1), x.min(axis=1))
    assert np.abs(y - x).max() <= 2.0 ** -21
    # every category both ways, and the wrap: a rotation by +d then -d returns within the same bound twice over
    z = ar.adjust_hue(ar.adjust_hue(x, F(2.5)), F(-2.5))
    assert np.abs(z - x).max() <= 2.0 ** -19
    assert (ar.adjust_hue(x, F(2.999)) >= 0).all()


def test_saturation_known_answers():
    rs = np.random.RandomState(2)
    x = np.concatenate([rs.random_sample((4000, 3)).astype(F), TIES, PRIMARIES, GREYS])
    v = x.max(axis=1)
    assert np.array_equal(ar.adjust_saturation(x, F(0)), np.stack([v, v, v], axis=1))      # factor 0: grey at v, exactly
    # factor 1: h carries at most four roundings of 2^-24, dh = 6 h adds half an ulp at a magnitude below 8 (2^-22), x three more:
    # 24 + 4 + 3 < 32 units of 2^-24 = 2^-19
    y = ar.adjust_saturation(x, F(1))
    assert np.abs(y - x).max() <= 2.0 ** -19
    assert np.array_equal(ar.adjust_saturation(GREYS, F(1.5)), GREYS)      # range == 0: h = 0, s = 0
    # ties r == g == v take the first branch (h from g - b), g == b == v the second
    t = ar.adjust_saturation(TIES, F(1))
    assert np.abs(t - TIES).max() <= 2.0 ** -19
    # a saturated primary stays put under any factor >= 1 (s is clamped to 1), and halves its saturation under .5
    assert np.array_equal(ar.adjust_saturation(PRIMARIES, F(1.5)), PRIMARIES)
    assert np.array_equal(ar.adjust_saturation(PRIMARIES, F(.5)), np.where(PRIMARIES > 0, F(1), F(.5)))
    assert (ar.adjust_saturation(x, F(1.5)) >= 0).all() and (ar.adjust_saturation(x, F(.5)) >= 0).all()


def test_gamma_contrast_known_answers():
    g = dict(gamma=F(2), cont=F(.5))
    x = np.zeros((2, 2, 3), F)
    x[0, 0] = (.5, 1, 0)
    out, mean = ar.gamma_contrast(x, g, ar.GAMMA | ar.CONTRAST)
    # v ** 2 = (.25, 1, 0) at one pixel of four: means (.0625, .25, 0), over the whole canvas, padding included
    assert np.array_equal(mean, np.array([.0625, .25, 0], F))
    assert np.array_equal(out[0, 0], np.array([(.25 - .0625) * .5 + .0625, (1 - .25) * .5 + .25, 0], F))
    assert np.array_equal(out[1, 1], np.array([.03125, .125, 0], F))
    out64, mean64 = ar.gamma_contrast(x, g, ar.GAMMA | ar.CONTRAST, np.float64)
    assert out64.dtype == np.float64 and np.array_equal(out64, out.astype(np.float64))
    # contrast off: gamma and the clip alone
    assert np.array_equal(ar.gamma_contrast(np.full((1, 1, 3), 1.5, F), dict(gamma=F(1), cont=F(1)), ar.GAMMA)[0], np.ones((1, 1, 3), F))


def test_pow_sees_no_negative_base():
    """The tensor adjust_gamma reads - canvas, hue, saturation - of every input of the GPU tests."""
    for size in ac.CANVASES:
        for stages in (0, ar.HUE | ar.SAT, 15):
            for im, g in zip(ac.images(), ac.geometries(size, stages)):
                x = ar.pre_gamma(im, size, g, stages)
                assert x.dtype == F and x.shape == size + (3,) and (x >= 0).all() and np.isfinite(x).all()


def test_canvas_window_and_flip():
    """A 2x2 source on a pad-only window: the canvas is zero outside the window and mirrored under the flip."""
    im = np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 255]]], np.uint8)
    g = dict(ih=2, iw=2, rh=2, rw=2, cy=0, cx=0, wh=2, ww=2, py=1, px=3, flip=0)
    c = ar.canvas(im, (4, 8), g)
    assert np.array_equal(c[1:3, 3:5], im.astype(F) * F(1 / 255.0)) and c.sum() == 6
    f = ar.canvas(im, (4, 8), dict(g, flip=1))
    assert np.array_equal(f, c[:, ::-1]) and np.array_equal(f[1, 8 - 1 - 3], c[1, 3])


def test_boxes_by_hand():
    """W = 52: x' = x * nw / iw + dx; under the flip (xmin, xmax) -> (52 - xmax', 52 - xmin'), then the clip to [0, 51]."""
    g = dict(ih=10, iw=10, nh_f=F(20), nw_f=F(20), dy_f=F(2), dx_f=F(-4), flip=0)
    rows = np.array([[2.25, 1, 8, 6, 3],      # x: .5 .. 12, y: 4 .. 14
                     [0, 0, 2.4, 9, 5]], F)      # x: -4 .. .8 -> clipped 0 .. .8: dropped after the crop, 4.8 wide before
    out, kept, info = ar.map_boxes(rows, g, (36, 52))
    assert kept == 1 and tuple(out[0]) == (F(.5), F(4), F(12), F(14), F(3)) and info['raw'][1, 2] - info['raw'][1, 0] > 1
    out, kept, info = ar.map_boxes(rows, dict(g, flip=1), (36, 52))
    # (.5, 12) -> (40, 51.5): the flip moves xmax across the clip edge 51;  (-4, .8) -> (51.2, 56) -> (51, 51): dropped
    assert kept == 1 and tuple(out[0]) == (F(40), F(4), F(51), F(14), F(3))
    assert tuple(info['raw'][0, [0, 2]]) == (F(40), F(51.5))


# ----------------------------------------------------------------------------- error paths
def test_geometry_error_paths():
    from yoloret_amd import runtime as rt
    ok = np.full((2, 10), .5, F)
    tiny = ok.copy()
    tiny[1, 2] = 0      # scale = min_scale = .01: 52 * .01 truncates to 0
    with pytest.raises(rt.YoloretHipError, match=r'image 1.*zero size'):
        _table([(9, 9), (9, 9)], (36, 52), tiny, min_scale=.01)
    with pytest.raises(ValueError, match='zero size'):
        ar.geometry(9, 9, (36, 52), tiny[1], min_scale=.01)
    # a precondition of crop_to_bounding_box / pad_to_bounding_box: no draw in [0, 1) is known to fail one (the sweep above finds
    # none); a dx draw of 1.5 puts the window beyond the canvas, as it would in TensorFlow
    far = ok.copy()
    far[0, 2], far[0, 3] = .1, 1.5      # nw = 22.1, dx = 1.5 * 29.9 = 44.85: 44 + 22 > 52
    with pytest.raises(rt.YoloretHipError, match=r'image 0.*pad_to_bounding_box'):
        _table([(9, 9), (9, 9)], (36, 52), far)
    with pytest.raises(ValueError, match='pad_to_bounding_box'):
        ar.geometry(9, 9, (36, 52), far[0])
    crop = ok.copy()
    crop[1, 2], crop[1, 4] = .9, 1.5      # nh = 65.7 > 36 and dy = 1.5 * -29.7: the crop leaves the resized image
    with pytest.raises(rt.YoloretHipError, match=r'image 1.*crop_to_bounding_box'):
        _table([(9, 9), (9, 9)], (36, 52), crop)
    bad = ok.copy()
    bad[0, 7] = np.nan
    with pytest.raises(rt.YoloretHipError, match='image 0.*not finite'):
        _table([(9, 9), (9, 9)], (36, 52), bad)
    with pytest.raises(rt.YoloretHipError, match='image 1 has size'):
        _table([(9, 9), (0, 9)], (36, 52), ok)
    with pytest.raises(rt.YoloretHipError, match='hue'):
        _table([(9, 9)], (36, 52), ok[:1], hue=.7)
    with pytest.raises(rt.YoloretHipError, match='stage bits'):
        _table([(9, 9)], (36, 52), ok[:1], stages=64)
    with pytest.raises(ValueError, match='draws'):
        _table([(9, 9)], (36, 52), ok)
    with pytest.raises(TypeError, match='unknown'):
        _table([(9, 9)], (36, 52), ok[:1], noise=1)
    L = rt.lib()
    assert L.yr_augment_workspace_bytes(64, 416, 416) == 64 * 169 * 3 * 4 and L.yr_augment_workspace_bytes(1, 8, 12) == 16
    assert L.yr_augment_batch(None, None, 1, 0, None, 8, 12, None, None, 0, None, None, 20, None, 0, None) == -1 and b'null' in L.yr_last_error()


def _labels(tmp_path, n=7):
    lines = []
    for k in range(n):
        name = ('demo_2011_001694.jpg', 'demo_2011_002558.jpg')[k % 2]
        lines.append('%s %d %d %d %d %d' % (os.path.join(GOLDEN, name), 10 + k, 20, 200 + k, 220, k))
    p = tmp_path / ('train_%d.txt' % n)
    p.write_text('\n'.join(lines) + '\n')
    return str(p)


def test_unbuilt_steps_raise():
    from yoloret_amd.yolo3.data import AugmentedDataset
    from yoloret_amd.yolo3.utils import get_random_data_device
    im = [np.zeros((4, 4, 3), np.uint8)]
    for kw, word in ((dict(val=.1), 'val'), (dict(noise=.05), 'noise'), (dict(blur=True), 'blur'), (dict(zoom_in=True), 'zoom')):
        with pytest.raises(NotImplementedError, match=word):
            get_random_data_device(im, np.zeros((1, 1, 5), F), np.zeros(1, np.int32), (36, 52), **kw)
        with pytest.raises(NotImplementedError, match=word):
            AugmentedDataset('x_1.txt', 2, None, 20, (96, 96), 3, **kw)
    AugmentedDataset('x_1.txt', 2, None, 20, (96, 96), 3, min_jpeg_quality=10, max_jpeg_quality=20)      # accepted and ignored


def test_augmented_dataset_host_side(tmp_path):
    from yoloret_amd.yolo3.data import AugmentedDataset, Dataset
    from yoloret_amd.yolo3.enums import DATASET_MODE
    labels = _labels(tmp_path)

    def passes(seed, n=2):
        ds = AugmentedDataset(labels, 3, None, 20, (96, 96), 3, seed=seed)
        it, num = ds.build()
        assert num == 7
        return [ds.epoch_plan(it.files, it.rng) for _ in range(n)]
    a, b, c = passes(4), passes(4), passes(5)
    order = lambda plan: [int(bb[0, 4]) for recs, _ in plan for _, bb in recs]
    for p, q in zip(a, b):      # the same seed: the same permutation and the same draws, pass by pass
        assert order(p) == order(q) and all(np.array_equal(x[1], y[1]) for x, y in zip(p, q))
    assert sorted(order(a[0])) == list(range(7)) and order(a[0]) != order(a[1]) and order(a[0]) != order(c[0])
    assert [len(recs) for recs, _ in a[0]] == [3, 3, 1]
    for recs, draws in a[0]:
        assert draws.dtype == F and draws.shape == (len(recs), 10) and (draws >= 0).all() and (draws < 1).all()
    assert not np.array_equal(a[0][0][1], a[1][0][1])
    # build()'s errors are Dataset's
    with pytest.raises(ValueError, match='No file found'):
        AugmentedDataset(str(tmp_path / 'none_*.txt'), 2).build()
    assert AugmentedDataset(None, 2).build() == (None, 0)
    # ... and Dataset(mode=TRAIN) still raises, now naming the class
    with pytest.raises(NotImplementedError, match='TRAIN.*AugmentedDataset'):
        Dataset(labels, 2, None, 20, (96, 96), 3, mode=DATASET_MODE.TRAIN).build()


# ----------------------------------------------------------------------------- ABI
def test_c_abi_declares_exports_and_builds_the_augmentation():
    from yoloret_amd import build, runtime as rt
    header = open(os.path.join(ROOT, 'include', 'yoloret_hip.h')).read()
    for name in ('yr_augment_geometry', 'yr_augment_workspace_bytes', 'yr_augment_batch'):
        assert re.search(r'\b%s\s*\(' % name, header) and name in rt.EXPORTS
    for name, bit in (('HUE', 1), ('SAT', 2), ('GAMMA', 4), ('CONTRAST', 8), ('NOFLIP', 16), ('ALL', 31)):
        assert re.search(r'^#define\s+YR_AUG_%s\s+%d\b' % (name, bit), header, re.M) and getattr(rt, 'AUG_' + name) == bit
    assert (ar.HUE, ar.SAT, ar.GAMMA, ar.CONTRAST, ar.NOFLIP) == (1, 2, 4, 8, 16)
    assert re.search(r'\}\s*yr_augment_geom\s*;', header) and 'augment.hip' in build.SOURCES
    assert rt.ABI_VERSION == 9 and re.search(r'^#define\s+YR_ABI_VERSION\s+9\b', header, re.M)
    L = ctypes.CDLL(build.build())
    L.yr_abi_sizeof.argtypes = [ctypes.c_int]
    assert L.yr_abi_sizeof(4) == 96 == ctypes.sizeof(rt.YrAugmentGeom) == rt.AUGMENT_GEOM_DTYPE.itemsize and 96 % 16 == 0
    assert L.yr_abi_sizeof(3) == 64 and L.yr_abi_sizeof(5) == 0
    assert [(n, rt.AUGMENT_GEOM_DTYPE.fields[n][1]) for n in rt.AUGMENT_GEOM_DTYPE.names] == \
        [(n, getattr(rt.YrAugmentGeom, n).offset) for n, _ in rt.YrAugmentGeom._fields_]
    assert rt.AUGMENT_DRAWS == ar.DRAWS and rt.AUGMENT_DEFAULTS == ar.DEFAULTS
    rt.lib()    # the binding's own load-time checks


def test_augment_kernels_do_not_spill():
    from yoloret_amd import build as b
    b.build()
    rows = b.kernel_resources()['augment.hip']
    assert sorted(r[0].split('7AugArgs')[0] for r in rows) == ['_Z17aug_finish_kernel', '_Z17aug_pixels_kernel']
    for name, vgprs, scratch, occ, lds in rows:
        assert scratch == 0, '%s keeps %d bytes per lane in scratch' % (name, scratch)
