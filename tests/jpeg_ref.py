"""The JPEG round trip of tf.image.random_jpeg_quality (reference code/yolo3/utils.py:228-230) restated in NumPy, integers only:
the definition yoloret_amd/csrc/jpeg.hip is tested against.  Entropy coding is lossless, so an encode followed by a decode is
colour transform, 2x2 chroma averaging, forward DCT, quantise | dequantise, inverse DCT, triangle-filter chroma upsampling, inverse
colour transform - each step as libjpeg's text specifies it (jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c, jidctint.c, jdsample.c,
jdcolor.c; 4:2:0 subsampling, the "islow" DCT, fancy upsampling: libjpeg's and TensorFlow's defaults).  tests/test_jpeg_host.py pins
it against Pillow on libjpeg-turbo, byte for byte.  Sizes are multiples of 16: whole MCUs, no edge replication, no dummy blocks.

All arithmetic is int64; `>>` on a NumPy integer array is an arithmetic shift."""
import numpy as np

I = np.int64

# JPEG Annex K, tables K.1 and K.2, in natural (row-major) order
LUMINANCE = np.array([16, 11, 10, 16, 24, 40, 51, 61,
                      12, 12, 14, 19, 26, 58, 60, 55,
                      14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77,
                      24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101,
                      72, 92, 95, 98, 112, 100, 103, 99], I).reshape(8, 8)
CHROMINANCE = np.array([17, 18, 24, 47, 99, 99, 99, 99,
                        18, 21, 26, 66, 99, 99, 99, 99,
                        24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99], I).reshape(8, 8)


def fix16(v):
    return int(v * 65536 + 0.5)


def fix13(v):
    return int(v * 8192 + 0.5)


F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = fix13(0.298631336), fix13(0.390180644), fix13(0.541196100), fix13(0.765366865)
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = fix13(0.899976223), fix13(1.175875602), fix13(1.501321110), fix13(1.847759065)
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = fix13(1.961570560), fix13(2.053119869), fix13(2.562915447), fix13(3.072711026)


def descale(v, n):
    return (v + (1 << (n - 1))) >> n


def float_to_u8(x):
    """convert_image_dtype(float32 -> uint8, saturate=True): the product in float32, truncated."""
    x = np.asarray(x, np.float32)
    return np.minimum(np.maximum(x * np.float32(255.5), np.float32(0)), np.float32(255)).astype(np.uint8)


def u8_to_float(u):
    """convert_image_dtype(uint8 -> float32)."""
    return u.astype(np.float32) * np.float32(1.0 / 255)


def draw_quality(u, min_jpeg_quality, max_jpeg_quality):
    """The quality of one image from a float32 uniform u in [0, 1): TensorFlow's int32 uniform over [min, max); libjpeg reads 0 as 1."""
    lo, hi = int(min_jpeg_quality), int(max_jpeg_quality)
    q = lo + int(float(np.float32(u)) * (hi - lo))
    return max(min(q, hi - 1), 1)


def quant_tables(quality):
    """(luminance, chrominance) [8,8] divisors of jpeg_set_quality(quality, force_baseline=TRUE)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMINANCE, CHROMINANCE))


def rgb_to_ycc(u):
    r, g, b = (u[..., c].astype(I) for c in range(3))
    half = 128 << 16
    y = (fix16(.299) * r + fix16(.587) * g + fix16(.114) * b + 32768) >> 16
    cb = (-fix16(.16874) * r - fix16(.33126) * g + fix16(.5) * b + half + 32767) >> 16
    cr = (fix16(.5) * r - fix16(.41869) * g - fix16(.08131) * b + half + 32767) >> 16
    return y, cb, cr


def downsample(p):
    """h2v2_downsample: the 2x2 mean with the bias 1, 2, 1, 2, ... along a row."""
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1], dtype=I) & 1)
    return (s + bias[None, :]) >> 2


def _fdct_1d(d, first):
    """jpeg_fdct_islow over the LAST axis of d [...,8]; first=True is pass 1 (rows), else pass 2 (columns)."""
    d = [d[..., k] for k in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        o[0], o[4] = descale(tmp10 + tmp11, 2), descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * F_0_541196100
    o[2] = descale(z1 + tmp13 * F_0_765366865, n)
    o[6] = descale(z1 - tmp12 * F_1_847759065, n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F_1_175875602
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F_0_298631336, tmp5 * F_2_053119869, tmp6 * F_3_072711026, tmp7 * F_1_501321110
    z1, z2, z3, z4 = -z1 * F_0_899976223, -z2 * F_2_562915447, -z3 * F_1_961570560 + z5, -z4 * F_0_390180644 + z5
    o[7], o[5], o[3], o[1] = descale(tmp4 + z1 + z3, n), descale(tmp5 + z2 + z4, n), descale(tmp6 + z2 + z3, n), descale(tmp7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _idct_1d(d, first):
    """jpeg_idct_islow over the LAST axis of d [...,8]; first=True is pass 1 (columns), else pass 2 (rows)."""
    d = [d[..., k] for k in range(8)]
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * F_0_541196100
    tmp2, tmp3 = z1 - z3 * F_1_847759065, z1 + z2 * F_0_765366865
    tmp0, tmp1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175875602
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F_0_298631336, tmp1 * F_2_053119869, tmp2 * F_3_072711026, tmp3 * F_1_501321110
    z1, z2, z3, z4 = -z1 * F_0_899976223, -z2 * F_2_562915447, -z3 * F_1_961570560 + z5, -z4 * F_0_390180644 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    n = 11 if first else 18
    o = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([descale(v, n) for v in o], axis=-1)


def _blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)      # [by,bx,row,col]


def _unblocks(b):
    by, bx = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def code_plane(p, table):
    """One component plane (values 0..255, sides multiples of 8) through forward DCT, quantise, dequantise, inverse DCT."""
    b = _blocks(p.astype(I) - 128)
    b = _fdct_1d(b, True)                                            # rows
    b = _fdct_1d(b.swapaxes(-1, -2), False).swapaxes(-1, -2)         # columns
    d = 8 * table
    c = np.sign(b) * ((np.abs(b) + (d >> 1)) // d)
    b = c * table
    b = _idct_1d(b.swapaxes(-1, -2), True).swapaxes(-1, -2)          # columns
    b = _idct_1d(b, False)                                           # rows
    return _unblocks(np.clip(b + 128, 0, 255))


def upsample(p):
    """h2v2_fancy_upsample: the triangle filter, 3/4 nearer and 1/4 further sample in each direction."""
    h, w = p.shape
    above, below = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    s = np.empty((2 * h, w), I)
    s[0::2], s[1::2] = 3 * p + above, 3 * p + below
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * h, 2 * w), I)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4      # at the two ends left / right is s itself: 4 s
    return out


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((fix16(1.402) * cr + 32768) >> 16)
    g = y + ((-fix16(.34414) * cb + 32768 - fix16(.71414) * cr) >> 16)
    b = y + ((fix16(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def roundtrip_u8(u, quality):
    """uint8 [H,W,3] -> uint8 [H,W,3]: JPEG encode at `quality` (4:2:0) and decode."""
    u = np.asarray(u)
    h, w = u.shape[:2]
    if u.dtype != np.uint8 or u.ndim != 3 or u.shape[2] != 3 or h % 16 or w % 16 or h == 0 or w == 0:
        raise ValueError('roundtrip_u8: a uint8 [H,W,3] image with H and W multiples of 16, not %s %s' % (u.dtype, u.shape))
    lum, chrom = quant_tables(quality)
    y, cb, cr = rgb_to_ycc(u)
    y = code_plane(y, lum)
    cb, cr = (upsample(code_plane(downsample(c), chrom)) for c in (cb, cr))
    return ycc_to_rgb(y, cb, cr)


def roundtrip(x, quality):
    """float32 [H,W,3] -> float32 [H,W,3]: adjust_jpeg_quality, steps a to j."""
    return u8_to_float(roundtrip_u8(float_to_u8(x), quality))
