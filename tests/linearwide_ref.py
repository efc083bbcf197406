"""The yardsticks of the wide 1x1 operators (yoloret_amd/csrc/linearwide.hip), written from the file's header comment, not from its code:
the chunk rule and the workspace of the weight gradient, which template instantiation a shape runs, and the case lists
tests/test_gpu_linearwide.py runs (tests/test_linearwide_host.py checks that they reach every instantiation and stay exact).
The products themselves are ``headtrain_ref.forward64`` / ``wgrad64`` and NumPy's float64 ``dy @ w``."""
import numpy as np

MAX_C = 1024
MIN_CHUNK, MAX_CHUNKS, CHUNK_STEP = 64, 1024, 16
PRODUCT_TILES = 16      # 16-wide output tiles per workgroup of the forward / input gradient: 4 waves x 4
WGRAD_TILES = 8         # tiles per side and workgroup of the weight gradient's stage 1: 2 waves x 4


def sizes_ok(pixels, cin, cout):
    return 1 <= pixels < 2 ** 40 and 1 <= cin <= MAX_C and 1 <= cout <= MAX_C


def kp_of(cin):
    return (cin + 3) // 4 * 4


def narrow(cin, cout):
    """both sides within the narrow entries' range: the weight gradient IS yr_linear_wgrad there (its chunk, its stage 1, its bytes)"""
    return cin <= 256 and cout <= 256


NARROW_MAX_CHUNKS = 2048


def narrow_min_chunk(cin, cout):
    """headtrain.hip's rule, restated from its header: 256 pixels, 512 where a side exceeds five tiles (80 channels)"""
    return 512 if cin > 80 or cout > 80 else 256


def min_chunk(cin, cout):
    """the chunk at few pixels: one slab (cout * kp floats) is no larger than its chunk's operands (chunk * (cin + cout) floats)"""
    if narrow(cin, cout):
        return narrow_min_chunk(cin, cout)
    c = max(MIN_CHUNK, -(-cout * kp_of(cin) // (cin + cout)))
    return -(-c // CHUNK_STEP) * CHUNK_STEP


def chunk(pixels, cin, cout):
    """pixels per workgroup of stage 1 (0: sizes the entries refuse)"""
    if not sizes_ok(pixels, cin, cout):
        return 0
    if narrow(cin, cout):
        c = max(narrow_min_chunk(cin, cout), -(-pixels // NARROW_MAX_CHUNKS))
        return -(-c // 16) * 16
    c = max(MIN_CHUNK, -(-cout * kp_of(cin) // (cin + cout)), -(-pixels // MAX_CHUNKS))
    return -(-c // CHUNK_STEP) * CHUNK_STEP


def workspace_bytes(pixels, cin, cout):
    c = chunk(pixels, cin, cout)
    return -(-pixels // c) * cout * kp_of(cin) * 4 if c else 0


def blocking(n, most):
    """n channels -> (blocks over the grid, tiles per block <= most)"""
    t = -(-n // 16)
    blocks = -(-t // most)
    return blocks, -(-t // blocks)


def idle_tiles(n, most):
    """whole tiles of the last block that lie past the channel count"""
    blocks, per = blocking(n, most)
    return blocks * per - -(-n // 16)


def product_form(n):
    """n output channels (cout of the forward, cin of the input gradient) -> WT of lw_product_kernel<WT, .>"""
    return -(-blocking(n, PRODUCT_TILES)[1] // 4)


def wgrad_form(cin, cout):
    """-> (TA, TB) of lw_wgrad_partial_kernel<TA, TB>: the output-channel side first (None: a narrow shape, the narrow entry's stage 1)"""
    if narrow(cin, cout):
        return None
    return -(-blocking(cout, WGRAD_TILES)[1] // 2), -(-blocking(cin, WGRAD_TILES)[1] // 2)


def kernel_names(cin, cout):
    """-> the names yr_last_kernel reports after the forward, the input gradient and stage 1 of the weight gradient"""
    form = wgrad_form(cin, cout)
    return ('lw_product_kernel<%d,0>' % product_form(cout), 'lw_product_kernel<%d,1>' % product_form(cin),
            'lw_wgrad_partial_kernel<%d,%d>' % form if form else 'ht_wgrad_partial_kernel')


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_linearwide.py, (cin, cout)
MODEL_SHAPES = [(216, 512), (512, 75), (424, 256), (331, 512), (272, 128), (576, 256), (512, 255)]
EDGE_SHAPES = [(257, 3), (3, 257), (257, 257), (1021, 513)]
CAP_SHAPE = (1024, 1024)
# what the lists above leave out of the 8 product and 12 gradient instantiations.  The gradient's stage 1 runs with a side above 256
# (257: three blocks of 6 tiles, TA / TB = 3; 512: four blocks of 8, 4) and any other side (1..32, 33..64, 65..96, 97..128 channels
# run 1..4): the forms with both at most 2 do not exist.  3 and 45 on the output side of the product run WT = 1, 77 and 125 WT = 2,
# 150 WT = 3 (10 tiles); the shapes narrow on both sides run the product kernels and the narrow entry's gradient.
FORM_SHAPES = ([(cin, cout) for cout in (257, 512) for cin in (3, 45, 77, 125) if (cin, cout) not in EDGE_SHAPES]
               + [(cin, cout) for cin in (257, 512) for cout in (3, 45, 77, 125) if (cin, cout) not in EDGE_SHAPES]
               + [(3, 45), (45, 3), (77, 125), (125, 77), (150, 150)])
NARROW_SHAPES = [(75, 75), (248, 128)]
EXACT_SHAPES = MODEL_SHAPES + EDGE_SHAPES + [CAP_SHAPE] + FORM_SHAPES + NARROW_SHAPES
PIXELS = [1, 5, 63, 64, 65]
ROUNDING_SHAPES = [(424, 256), (1021, 513)]
ROUNDING_PIXELS = 333      # five 64-pixel workgroups with a ragged last one; three chunks at (424, 256), one at (1021, 513)
NARROWEST_WIDE = (257, 3)
FIRST_GROWN_PIXELS = MAX_CHUNKS * MIN_CHUNK + 1      # the first pixel count whose chunk exceeds the minimum, at a shape whose minimum is 64


def wgrad_pixels(cin, cout):
    """the pixel counts of the gradient's cases: the common ones, chunk + 1 and 2 chunk + 5 (the chunk the minimum of the shape)"""
    c = min_chunk(cin, cout)
    return PIXELS + [c + 1, 2 * c + 5]


def int_weights(seed, cin, cout):
    """[cout, cin] integers in [-4, 4] -> (w float32, Wt [cout, kp] with NaN in the pad columns: they are never read)"""
    w = np.random.default_rng(seed).integers(-4, 5, (cout, cin)).astype(np.float32)
    wt = np.full((cout, kp_of(cin)), np.nan, np.float32)
    wt[:, :cin] = w
    return w, wt
