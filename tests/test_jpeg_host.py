"""Host side of random_jpeg_quality: tests/jpeg_ref.py (the NumPy restatement of the JPEG round trip the kernels of
yoloret_amd/csrc/jpeg.hip are tested against) pinned byte for byte against Pillow on libjpeg-turbo - live where such a Pillow is
installed, and against the committed goldens of tests/golden/jpeg_cases.npz always -, step a at every boundary, the quality draw,
and the host-side behaviour of the Python surface.  No GPU is touched."""
import os

import numpy as np
import pytest

from tests import jpeg_cases as jc, jpeg_ref as jr

F = np.float32
_golden = {}


def golden():
    if not _golden:
        with np.load(os.path.join(jc.GOLDEN, 'jpeg_cases.npz')) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def _turbo():
    try:
        from PIL import features
        return bool(features.check_feature('libjpeg_turbo'))
    except Exception:
        return False


@pytest.mark.skipif(not _turbo(), reason='needs a Pillow built on libjpeg-turbo (another libjpeg upsamples differently); the goldens below never skip')
@pytest.mark.parametrize('shape', jc.HOST_SHAPES, ids=['%dx%d' % s for s in jc.HOST_SHAPES])
def test_restatement_equals_pillow(shape):
    for content in jc.CONTENTS:
        u = jc.image(content, shape)
        for q in jc.QUALITIES:
            want, got = jc.pillow_roundtrip(u, q), jr.roundtrip_u8(u, q)
            assert np.array_equal(got, want), '%s %s quality %d: %d bytes differ, max %d' % (
                content, shape, q, (got != want).sum(), np.abs(got.astype(int) - want).max())


def test_restatement_equals_committed_goldens():
    g = golden()
    n = 0
    for content, (h, w) in jc.GOLDEN_CASES:
        u = g['in/%s/%dx%d' % (content, h, w)]
        assert np.array_equal(u, jc.image(content, (h, w))), 'the generator of %s %dx%d changed: rerun tests/golden/make_jpeg_golden.py' % (content, h, w)
        for q in jc.GOLDEN_QUALITIES:
            want, got = g['out/%s/%dx%d/q%d' % (content, h, w, q)], jr.roundtrip_u8(u, q)
            assert np.array_equal(got, want), '%s %dx%d quality %d: %d bytes differ' % (content, h, w, q, (got != want).sum())
            n += 1
    assert n == len(jc.GOLDEN_CASES) * 5 and {s for _, s in jc.GOLDEN_CASES} == set(jc.GOLDEN_SHAPES)
    # the round trip is not the identity on these inputs, and the qualities differ from one another
    noise = [g['out/noise/48x80/q%d' % q] for q in jc.GOLDEN_QUALITIES]
    assert all(not np.array_equal(a, b) for a, b in zip(noise, noise[1:])) and not np.array_equal(noise[-1], g['in/noise/48x80'])


def test_float_path_of_the_restatement():
    u = jc.image('noise', (16, 48))
    x = u.astype(F) * F(1.0 / 255)
    assert np.array_equal(jr.float_to_u8(x), u)      # u / 255 comes back as u: the goldens can be fed as floats
    out = jr.roundtrip(x, 87)
    assert out.dtype == F and np.array_equal(out.view(np.uint32), (golden()['out/noise/16x48/q87'].astype(F) * F(1.0 / 255)).view(np.uint32))
    for bad in (np.zeros((24, 16, 3), np.uint8), np.zeros((16, 40, 3), np.uint8), np.zeros((16, 16, 3), F)):
        with pytest.raises(ValueError):
            jr.roundtrip_u8(bad, 50)


def test_step_a_at_every_boundary():
    """trunc(min(max(x * 255.5f, 0), 255)) with the product in float32, at the float32 values just below, at and just above k / 255.5."""
    v = jc.step_a_values()
    assert v.dtype == F and v.size == 3 * 256 + 4
    got = jr.float_to_u8(v).astype(int)
    prod = v * F(255.5)
    assert prod.dtype == F
    want = np.trunc(np.clip(prod.astype(np.float64), 0, 255)).astype(int)      # (the float32 product, widened exactly)
    assert np.array_equal(got, want)
    assert set(got.tolist()) == set(range(256))      # every byte is reached
    below, at, above = got[0:768:3], got[1:768:3], got[2:768:3]
    assert (at >= below).all() and (above >= at).all() and (above - below <= 1).all()
    assert got[768:].tolist() == [0, 255, 0, 255]      # 0, 1, -0.0, 1 + ulp
    assert jr.float_to_u8(np.array([-3.0, 7.0, 0.5], F)).tolist() == [0, 255, 127]
    img = jc.step_a_image((16, 48))
    assert img.shape == (16, 48, 3) and set(img.reshape(-1).view(np.uint32).tolist()) == set(v.view(np.uint32).tolist())


@pytest.mark.parametrize('bounds', [(80, 100), (0, 1), (0, 100), (99, 100)])
def test_quality_draw(bounds):
    from yoloret_amd.yolo3.utils import draw_jpeg_quality
    lo, hi = bounds
    top = F(1) - F(2.0 ** -24)
    assert top < 1 and np.nextafter(top, F(2)) == 1
    for draw in (draw_jpeg_quality, jr.draw_quality):
        assert draw(F(0), lo, hi) == max(lo, 1)
        assert draw(top, lo, hi) == max(hi - 1, 1)
        qs = [draw(u, lo, hi) for u in np.linspace(0, 1, 4001, dtype=F)[:-1]]
        assert min(qs) >= max(lo, 1) and max(qs) <= max(hi - 1, 1) and 0 not in qs
        assert sorted(qs) == qs and set(qs) == set(range(max(lo, 1), max(hi - 1, 1) + 1))      # every quality of [min, max) is drawn
    assert all(draw_jpeg_quality(u, lo, hi) == jr.draw_quality(u, lo, hi) for u in np.random.default_rng(5).random(200, dtype=F))


def test_quantisation_tables():
    lum, chrom = jr.quant_tables(50)
    assert np.array_equal(lum, jr.LUMINANCE) and np.array_equal(chrom, jr.CHROMINANCE)
    assert all((t == 1).all() for t in jr.quant_tables(100))
    lum1, chrom1 = jr.quant_tables(1)
    assert lum1.max() == 255 and (chrom1 == 255).all() and lum1.min() > 1
    assert all(np.array_equal(a, b) for a, b in zip(jr.quant_tables(0), jr.quant_tables(1)))      # libjpeg reads 0 as 1
    # step f's division through the kernels' multiplier: n / d == (n * (floor((2^32 - 1) / d) + 1)) >> 32 for every n the DCT can give
    n = np.arange(0, 1 << 16, dtype=np.uint64)
    for t in range(1, 256):
        d = 8 * t
        m = np.uint64((2 ** 32 - 1) // d + 1)
        assert np.array_equal((n * m) >> np.uint64(32), n // np.uint64(d)), t


def test_value_errors_of_the_surface():
    from yoloret_amd.yolo3.data import AugmentedDataset
    from yoloret_amd.yolo3.utils import get_random_data_device, random_jpeg_quality_device
    x = np.zeros((1, 16, 16, 3), F)      # (the bounds are checked before the images are looked at)
    for lo, hi in ((-1, 50), (50, 101), (60, 60), (70, 20), (100, 100)):
        with pytest.raises(ValueError, match='jpeg'):
            random_jpeg_quality_device(x, lo, hi)
    im = [np.zeros((4, 4, 3), np.uint8)]
    with pytest.raises(ValueError, match='between 0 and 100'):
        get_random_data_device(im, np.zeros((1, 1, 5), F), np.zeros(1, np.int32), (32, 32), apply_jpeg=True, min_jpeg_quality=-5, max_jpeg_quality=20)
    with pytest.raises(ValueError, match='multiples of 16'):
        get_random_data_device(im, np.zeros((1, 1, 5), F), np.zeros(1, np.int32), (36, 52), apply_jpeg=True)
    with pytest.raises(ValueError, match='between 0 and 100'):
        AugmentedDataset('x_1.txt', 2, None, 20, (96, 96), 3, apply_jpeg=True, min_jpeg_quality=50, max_jpeg_quality=120)
    # off, or on with the reference's condition false: the bounds are accepted and unused
    assert AugmentedDataset('x_1.txt', 2, None, 20, (96, 96), 3, min_jpeg_quality=50, max_jpeg_quality=120).jpeg is False
    assert AugmentedDataset('x_1.txt', 2, None, 20, (96, 96), 3, apply_jpeg=True, min_jpeg_quality=90, max_jpeg_quality=90).jpeg is False
    assert AugmentedDataset('x_1.txt', 2, None, 20, (96, 96), 3, apply_jpeg=True).jpeg is True


def test_apply_jpeg_leaves_the_plan_and_the_draws_alone(tmp_path):
    """Host side only: records, their order and the ten draws per image of a seed do not depend on apply_jpeg, and without it they
    are the stream of np.random.default_rng(seed) as before; the qualities come from default_rng((seed, 1))."""
    from yoloret_amd.yolo3.data import AugmentedDataset
    lines = ['img_%d.jpg %d %d %d %d %d' % (k, 3 * k, 2 * k, 3 * k + 20, 2 * k + 30, k % 20) for k in range(7)]
    labels = tmp_path / 'train_7.txt'
    labels.write_text('\n'.join(lines) + '\n')

    def plans(seed, **kw):
        ds = AugmentedDataset(str(labels), 3, None, 20, (96, 96), 3, seed=seed, **kw)
        it, num = ds.build()
        assert num == 7
        return it, [ds.epoch_plan(it.files, it.rng) for _ in range(2)]
    it_off, off = plans(4)
    it_on, on = plans(4, apply_jpeg=True)
    rng = np.random.default_rng(4)      # today's stream: one permutation, then [b,10] float32 draws per batch
    for p, q in zip(off, on):
        order = rng.permutation(7)
        assert [r[0] for recs, _ in p for r in recs] == ['img_%d.jpg' % k for k in order]
        assert [len(recs) for recs, _ in p] == [3, 3, 1]
        for (recs_a, draws_a), (recs_b, draws_b) in zip(p, q):
            assert [r[0] for r in recs_a] == [r[0] for r in recs_b]
            want = rng.random((len(recs_a), 10), dtype=F)
            assert draws_a.dtype == F and np.array_equal(draws_a, want) and np.array_equal(draws_b, want)
    second = np.random.default_rng((4, 1))
    assert np.array_equal(it_on.jpeg_rng.random(3, dtype=F), second.random(3, dtype=F))
    assert np.array_equal(it_off.rng.random(5), rng.random(5))      # nothing else was drawn from the first generator
