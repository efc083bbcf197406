"""Every kernel form of yoloret_amd/csrc/headtrain.hip on the device: the 25 instantiations ht_wgrad_partial_kernel<TCO, TCI> and the
5 of ht_forward_kernel<NT>, the blocked grid where the tiles do not fill it, and a gradient chunk above its minimum.  The helpers
(carrier, fence, NaN pre-fill) are those of tests/test_gpu_headtrain.py; the yardsticks those of tests/headtrain_ref.py.

Which kernel a shape runs is decided by ht_blocking, restated here as ``blocking``: n channels are t = ceil(n / 16) tiles, spread
over blocks = ceil(t / 5) grid slots of per = ceil(t / blocks) tiles each.  The gradient of (cin, cout) runs
ht_wgrad_partial_kernel<per(cout), per(cin)>, the forward ht_forward_kernel<per(cout)>.  blocks * per - t tiles of the last block lie
wholly beyond the channel count (``idle_tiles``).  tests/test_headtrain_host.py asserts (without a GPU) that the case lists below
reach every instantiation and that the ragged cases have such tiles on either side.

Exact cases: integers in [-4, 4] (headtrain_ref.int_case): every partial sum is exact in float32 whatever the order, so the result
must equal the float64 result bit for bit, pad columns +0.  Rows carry one NaN pad column (x_ld = cin + 1, dy_ld = cout + 1,
y_ld = cout + 1)."""
import numpy as np
import pytest

from tests import headtrain_ref as ref
from tests.test_gpu_headtrain import EPS24, NAN_BITS, _bits, _fenced_forward, _fenced_wgrad, _pixel_counts, _rt

pytestmark = pytest.mark.gpu

MAX_T = 5                                   # HT_MAX_T: tiles of 16 per workgroup and side
WIDTHS = [13, 29, 47, 61, 77]               # 1..5 tiles, none a multiple of 4: every dwt has pad columns
FORM_WGRAD = [(cin, cout) for cout in WIDTHS for cin in WIDTHS]                      # (cin, cout)
FORM_FORWARD = [(cin, cout) for cin in (29, 77) for cout in WIDTHS]
RAGGED_WGRAD = [(97, 193), (193, 97), (161, 161), (81, 209), (193, 3), (3, 193)]
RAGGED_FORWARD = [(97, cout) for cout in (97, 161, 193)]
RAGGED_BLOCKINGS = {97: (2, 4), 161: (3, 4), 193: (3, 5), 81: (2, 3), 209: (3, 5)}   # channels -> (blocks, tiles per block)
BIG_PIXELS, BIG_CIN, BIG_COUT = 2048 * 256 + 1, 5, 3                                 # the first pixel count whose chunk is not 256
BIG_CHUNK, BIG_SLABS = 272, 1928


def blocking(n):
    """ht_blocking: channels -> (blocks, tiles per block)."""
    t = (n + 15) // 16
    blocks = (t + MAX_T - 1) // MAX_T
    return blocks, (t + blocks - 1) // blocks


def idle_tiles(n):
    """Tiles of the last block that lie wholly at or beyond channel n."""
    blocks, per = blocking(n)
    return blocks * per - (n + 15) // 16


def wgrad_form(cin, cout):
    """(TCO, TCI) of the gradient kernel this shape runs."""
    return blocking(cout)[1], blocking(cin)[1]


def forward_form(cout):
    """NT of the forward kernel this width runs."""
    return blocking(cout)[1]


def _wgrad_exact(dev, seed, pixels, cin, cout, x_ld, dy_ld, offsets):
    kp = (cin + 3) // 4 * 4
    x, dy = ref.int_case(seed, pixels, cin, cout, x_ld, dy_ld)
    want = np.zeros((cout, kp), np.float32)
    want[:, :cin] = ref.wgrad64(x[:, :cin], dy[:, :cout])          # integers: exact, zeros are +0
    for off in offsets:
        got = _fenced_wgrad(dev, x, dy, cin, cout, off)
        assert np.all(_bits(got[:, cin:]) == 0), 'P=%d cin=%d cout=%d offset %d bytes: pad columns are not +0' % (pixels, cin, cout, 4 * off)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), 'P=%d cin=%d cout=%d <TCO %d, TCI %d> x_ld=%d dy_ld=%d offset %d bytes: %d of %d elements differ, first at %s' % (
            (pixels, cin, cout) + wgrad_form(cin, cout) + (x_ld, dy_ld, 4 * off, int(bad.sum()), want.size, tuple(np.argwhere(bad)[0])))


def _forward_exact(dev, cin, cout):
    chunk, counts = _pixel_counts(cin, cout)
    rng = np.random.default_rng(cin * 1000 + cout)
    w = rng.integers(-4, 5, (cout, cin)).astype(np.float32)
    wt = np.full((cout, (cin + 3) // 4 * 4), np.nan, np.float32)       # pad columns NaN: they are not read
    wt[:, :cin] = w
    for i, pixels in enumerate(counts):
        x, _ = ref.int_case(100 * i + cin, pixels, cin, cout, cin + 1, None)
        want = ref.forward64(x[:, :cin], w).astype(np.float32)
        for off in (0, 1):
            got = _fenced_forward(dev, x, wt, cin, cout, cout + 1, off)          # (asserts that columns >= cout kept their NaN)
            assert np.all(_bits(got[:, cout:]) == NAN_BITS)
            bad = _bits(got[:, :cout]) != _bits(want)
            assert not bad.any(), 'P=%d cin=%d cout=%d <NT %d> offset %d bytes: %d of %d elements differ, first at %s' % (
                pixels, cin, cout, forward_form(cout), 4 * off, int(bad.sum()), want.size, tuple(np.argwhere(bad)[0]))


# ----------------------------------------------------------------------------- 1. every instantiation
@pytest.mark.parametrize('cin,cout', FORM_WGRAD, ids=['%dx%d' % c for c in FORM_WGRAD])
def test_wgrad_every_instantiation(dev, cin, cout):
    chunk, _ = _pixel_counts(cin, cout)
    assert chunk == 256 and blocking(cin)[0] == blocking(cout)[0] == 1
    for i, pixels in enumerate((5, chunk + 1)):
        _wgrad_exact(dev, 100 * i + cin, pixels, cin, cout, cin + 1, cout + 1, (0, 1))


@pytest.mark.parametrize('cin,cout', FORM_FORWARD, ids=['%dx%d' % c for c in FORM_FORWARD])
def test_forward_every_instantiation(dev, cin, cout):
    assert blocking(cout)[0] == 1
    _forward_exact(dev, cin, cout)


# ----------------------------------------------------------------------------- 2. ragged blocks
@pytest.mark.parametrize('cin,cout', RAGGED_WGRAD, ids=['%dx%d' % c for c in RAGGED_WGRAD])
def test_wgrad_ragged_blocks(dev, cin, cout):
    """A grid of blocks x per tiles that the channel count does not fill: the last block's trailing tiles lie wholly beyond cin
    (193 -> 3 x 5 slots for 13 tiles) or cout, and write nothing."""
    rt = _rt()
    assert all(rt.linear_wgrad_chunk(p, cin, cout) == 512 for p in (1, 5, 513))
    for i, pixels in enumerate((5, 513)):
        _wgrad_exact(dev, 100 * i + cin, pixels, cin, cout, cin + 1, cout + 1, (0, 1))


@pytest.mark.parametrize('cin,cout', RAGGED_FORWARD, ids=['%dx%d' % c for c in RAGGED_FORWARD])
def test_forward_ragged_blocks(dev, cin, cout):
    assert blocking(cout) == RAGGED_BLOCKINGS[cout]
    _forward_exact(dev, cin, cout)


# ----------------------------------------------------------------------------- 3. a chunk above the minimum
def _big_wgrad(dev, x, dy):
    rt = _rt()
    pixels = x.shape[0]
    return _fenced_wgrad(dev, x, dy, BIG_CIN, BIG_COUT), rt.linear_wgrad_chunk(pixels, BIG_CIN, BIG_COUT)


# (pixels, chunk): 524 289 leaves 145 pixels to the last of 1928 workgroups - waves 0 and 1 full (68), wave 2 two quartets and one
# pixel, wave 3 none; 524 357 (68 more) ends on wave 3 instead; 524 286 is back at chunk 256, the full grid of 2048 workgroups, and
# ends two pixels short of wave 3's range
BIG_EXACT = [(BIG_PIXELS, BIG_CHUNK), (BIG_PIXELS - 3, 256), (BIG_PIXELS + 68, BIG_CHUNK)]


@pytest.mark.parametrize('pixels,chunk', BIG_EXACT, ids=['P%d' % p for p, _ in BIG_EXACT])
def test_wgrad_large_chunk_exact(dev, pixels, chunk):
    """chunk 272: 68 pixels = 17 quartets per wave, so every wave of every workgroup runs eight groups of two quartets and then the
    single-quartet loop, and stage 2 adds 1928 slabs.  Integers in [-4, 4]: |sum| <= 16 P < 2^24, exact in any order."""
    assert 16 * pixels < 2 ** 24 and 16 * BIG_PIXELS == 8388624
    rt = _rt()
    assert rt.linear_wgrad_chunk(pixels, BIG_CIN, BIG_COUT) == chunk
    slabs = -(-pixels // chunk)
    assert slabs == {BIG_PIXELS: BIG_SLABS, BIG_PIXELS - 3: 2048, BIG_PIXELS + 68: BIG_SLABS}[pixels]
    assert rt.linear_wgrad_workspace_bytes(pixels, BIG_CIN, BIG_COUT) == slabs * BIG_COUT * 8 * 4
    x, dy = ref.int_case(pixels, pixels, BIG_CIN, BIG_COUT)
    want = np.zeros((BIG_COUT, 8), np.float32)
    want[:, :BIG_CIN] = ref.wgrad64(x, dy)
    assert np.abs(want).max() <= 16 * pixels
    got, _ = _big_wgrad(dev, x, dy)
    assert np.all(_bits(got[:, BIG_CIN:]) == 0), 'pad columns are not +0'
    assert np.array_equal(_bits(got), _bits(want)), 'P=%d chunk %d: got %s, want %s' % (pixels, chunk, got[:, :BIG_CIN], want[:, :BIG_CIN])


def test_wgrad_large_chunk_rounding(dev):
    """P = 524 289 standard-normal pixels, 5 -> 3 channels, chunk 272: each element is a sum of 68 products per wave in sequence, 4
    waves in order, 1928 slabs in order.  A CPU emulation of that order gave 0.5 - 1.8 x the figure of NumPy's float32 product over
    six seeds (seed 7: E_numpy 5.72e-07, emulated 3.04e-07, bar 2.35e-06); a float32 running sum in pixel order sits at 20 x.
    Measured on an MI355X: device 2.72e-07, E_ref 5.72e-07, bar 2.35e-06."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((BIG_PIXELS, BIG_CIN)).astype(np.float32)
    dy = rng.standard_normal((BIG_PIXELS, BIG_COUT)).astype(np.float32)
    r64 = ref.wgrad64(x, dy)
    e_ref = ref.rel_err(dy.T @ x, r64)
    got, chunk = _big_wgrad(dev, x, dy)
    assert chunk == BIG_CHUNK
    e_dev = ref.rel_err(got[:, :BIG_CIN], r64)
    print('wgrad %dx%d P=%d chunk %d: device %.3e, NumPy float32 %.3e, bar %.3e' % (BIG_CIN, BIG_COUT, BIG_PIXELS, chunk, e_dev, e_ref, 4 * e_ref + EPS24))
    assert np.all(_bits(got[:, BIG_CIN:]) == 0)
    assert e_dev <= 4 * e_ref + EPS24
