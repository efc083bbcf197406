"""Inputs shared by tests/test_jpeg_host.py, tests/test_gpu_jpeg.py and tests/golden/make_jpeg_golden.py: uint8 [H,W,3] images whose
sides are multiples of 16, by content and shape, deterministic.

    noise      uniform bytes: every coefficient of every block is alive
    demo       a crop of one of the two committed demo JPEGs (natural statistics: most high coefficients quantise to 0)
    ramp       a smooth ramp along both axes, a different slope per channel
    black, white   constants: DC only, and the clamps of the colour transforms at both ends
    primaries  the six saturated primaries, white and black in 1-pixel stripes, shifted by two per row: the largest chroma steps
               there are, decoded values beyond 0..255 before the clamps of the inverse DCT and of YCbCr -> RGB
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEMOS = ('demo_2011_001694.jpg', 'demo_2011_002558.jpg')
# 16x16: one MCU, every upsampling edge rule at once; 16x48 / 48x16: left, middle, right / top, middle, bottom MCUs; 48x80: an MCU
# with all eight neighbours, not square
GOLDEN_SHAPES = ((16, 16), (16, 48), (48, 16), (32, 32), (48, 80))
HOST_SHAPES = GOLDEN_SHAPES + ((16, 32), (32, 48), (32, 64), (96, 96))
CONTENTS = ('noise', 'demo', 'ramp', 'black', 'white', 'primaries')
QUALITIES = (1, 37, 50, 80, 87, 93, 99, 100)
GOLDEN_QUALITIES = (1, 50, 87, 99, 100)
# the committed goldens (tests/golden/jpeg_cases.npz): every content at the four small shapes; at 48x80 the two contents whose every
# coefficient is alive and the constants - a natural image and a ramp of that size would double the file and add no rule
GOLDEN_CASES = tuple((c, s) for c in CONTENTS for s in GOLDEN_SHAPES if s != (48, 80) or c in ('noise', 'primaries', 'black', 'white'))
_PRIMARIES = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
_cache = {}


def _demo(k):
    if ('demo', k) not in _cache:
        from PIL import Image
        with Image.open(os.path.join(GOLDEN, DEMOS[k])) as img:
            _cache['demo', k] = np.array(img.convert('RGB'), dtype=np.uint8)
    return _cache['demo', k]


def image(content, shape):
    """uint8 [H,W,3], read-only, the same array on every call."""
    key = (content, tuple(shape))
    if key not in _cache:
        h, w = shape
        if content == 'noise':
            u = np.random.RandomState(1000 * h + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        elif content == 'demo':
            src = _demo((h + w) // 16 % 2)
            y0, x0 = (src.shape[0] - h) // 3, (src.shape[1] - w) // 2
            u = src[y0:y0 + h, x0:x0 + w].copy()
        elif content == 'ramp':
            yy, xx = np.mgrid[0:h, 0:w]
            u = np.stack([(255 * xx) // (w - 1), (255 * yy) // (h - 1), (255 * (xx + yy)) // (h + w - 2)], axis=-1).astype(np.uint8)
        elif content in ('black', 'white'):
            u = np.full((h, w, 3), 0 if content == 'black' else 255, np.uint8)
        elif content == 'primaries':
            yy, xx = np.mgrid[0:h, 0:w]
            u = _PRIMARIES[(xx + 2 * yy) % 8]
        else:
            raise KeyError(content)
        u.setflags(write=False)
        _cache[key] = u
    return _cache[key]


def pillow_roundtrip(u, quality):
    """Pillow's encode and decode of a uint8 image: the independent implementation (libjpeg-turbo where PIL.features says so)."""
    import io
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(u)).save(f, format='JPEG', quality=int(quality), subsampling=2)
    f.seek(0)
    with Image.open(f) as img:
        return np.array(img.convert('RGB'), dtype=np.uint8)


def step_a_values():
    """float32 values around every boundary of trunc(min(max(x * 255.5f, 0), 255)): for k in 0..255 the float32 just below, at and
    just above k / 255.5, then 0, 1, -0.0 and 1 + ulp."""
    at = (np.arange(256, dtype=np.float64) / 255.5).astype(np.float32)
    below, above = np.nextafter(at, np.float32(-1)), np.nextafter(at, np.float32(2))
    extra = np.array([0.0, 1.0, -0.0, np.nextafter(np.float32(1), np.float32(2))], np.float32)
    return np.concatenate([np.stack([below, at, above], axis=1).reshape(-1), extra])


def step_a_image(shape):
    """float32 [H,W,3] made of step_a_values(), repeated in a stride that is prime to the row: every value next to every other."""
    h, w = shape
    v = step_a_values()
    idx = (np.arange(h * w * 3, dtype=np.int64) * 7) % v.size
    return v[idx].reshape(h, w, 3)
