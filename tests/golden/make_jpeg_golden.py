"""Writes tests/golden/jpeg_cases.npz: the inputs of tests/jpeg_cases.py listed in GOLDEN_CASES and what Pillow (on libjpeg-turbo) makes of
them at GOLDEN_QUALITIES - Image.save(format='JPEG', quality=q, subsampling=2), then Image.open.  tests/jpeg_ref.py and the kernels
of yoloret_amd/csrc/jpeg.hip are compared with these bytes where no Pillow on libjpeg-turbo is at hand.

    python tests/golden/make_jpeg_golden.py

Keys: 'in/<content>/<H>x<W>' uint8 [H,W,3]; 'out/<content>/<H>x<W>/q<quality>' uint8 [H,W,3]; 'pillow' the version string."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import PIL
    from PIL import features
    from tests import jpeg_cases as jc
    if not features.check_feature('libjpeg_turbo'):
        raise SystemExit('this Pillow is not built on libjpeg-turbo: another libjpeg upsamples differently')
    out = {'pillow': np.array('%s libjpeg-turbo %s' % (PIL.__version__, features.version_feature('libjpeg_turbo')))}
    for content, (h, w) in jc.GOLDEN_CASES:
        u = jc.image(content, (h, w))
        out['in/%s/%dx%d' % (content, h, w)] = u
        for q in jc.GOLDEN_QUALITIES:
            out['out/%s/%dx%d/q%d' % (content, h, w, q)] = jc.pillow_roundtrip(u, q)
    path = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
