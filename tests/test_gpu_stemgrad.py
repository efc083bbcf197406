"""The 3 x 3 entry-convolution operators on the device (yoloret_amd/csrc/stemgrad.hip behind yr_conv3x3_forward / _dgrad / _wgrad and
autograd.conv3x3) against tests/stemgrad_ref.py.

Every launch of a C entry runs between the guards of tests/fence.py (``test_gpu_convgrad.fenced``: outputs and workspaces pre-filled with
NaN, the data in carriers at two alignments, the pad columns of a written tensor must keep their bytes).

The forward and the input gradient are ONE chain of fmaf per element in the order the header documents, the weight gradient a fixed
tree of such chains: on standard-normal data the device must equal the float32 restatement BIT FOR BIT, not within a bar.

The tiles.  Neither kernel has a two-dimensional tile: a workgroup of the forward owns 256 consecutive output pixels in (image, row,
column) order, one of the input gradient 256 consecutive cells of the padded input grid (a cell = stride x stride input pixels) in
the same order.  With T = 256 the boundary maps give T + 1 = 257 outputs as one row and as one column, and 2 T - 1 = 511 as a 7 x 73
block, at either stride (BOUNDARY_MAPS; tests/test_stemgrad_host.py counts the pixels and cells)."""
import numpy as np
import pytest
import torch

from tests import stemgrad_ref as ref
from tests.test_gpu_autograd import Calls, _within_bar
from tests.test_gpu_convgrad import _bits, fenced

pytestmark = pytest.mark.gpu

CHANNELS = [(3, 8), (3, 24), (3, 40), (3, 64), (1, 24), (4, 24), (3, 5), (2, 27)]      # (cin, cout); the last two: the guarded form
MAPS = [(1, 1), (2, 3), (8, 8), (7, 9), (9, 7)]
BATCHES = [1, 3]
ZERO_PAD = (0, 0, 1, 1)                                  # the ZeroPadding2D form: nothing in front, one row / column behind
BOUNDARY_MAPS = {1: [(1, 257), (257, 1), (7, 73)], 2: [(1, 513), (513, 1), (13, 145)]}
TILE = 256
# the weight gradient's chunk cases (stride 1, 'same', so the output is the map): B, H, W -> what the case reaches
CHUNK_CASES = [((1, 16, 16), 'exactly one chunk'), ((1, 32, 16), 'two chunks'), ((2, 12, 16), 'a chunk that spans two images, a partial last chunk'),
               ((1, 20, 16), 'a partial last chunk'), ((1, 2049, 256), 'a chunk above the minimum')]
CHUNK_CHANNELS = [(3, 24), (3, 40), (3, 64), (2, 5)]     # 4, 2, 1 partial sums; a partial channel quad
ROUNDING_CASES = [(2, 40, 37, 3, 24, 2), (1, 30, 30, 3, 48, 1)]


def _rt():
    from yoloret_amd import runtime
    return runtime


def _case(seed, b, h, w, cin, cout, stride, padding):
    rng = np.random.default_rng(seed)
    pads, (oh, ow) = ref.geometry(h, w, stride, padding)
    x = rng.standard_normal((b, h, w, cin)).astype(np.float32)
    wt = rng.standard_normal((9 * cin, cout)).astype(np.float32)
    dy = rng.standard_normal((b, oh, ow, cout)).astype(np.float32)
    return x, wt, dy, (b, h, w, cin, cout, stride, pads[0], pads[1], oh, ow)


def dev_forward(dev, x, wt, g, y_ld, off=0):
    rt = _rt()

    def launch(r, w, _):
        rt.check(rt.lib().yr_conv3x3_forward(r[0], x.shape[3], r[1], *g, w[0], y_ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [x, wt], [(g[0], g[8], g[9], y_ld)], [g[4]])[0]


def dev_dgrad(dev, dy, wt, g, dx_ld, off=0):
    rt = _rt()

    def launch(r, w, _):
        rt.check(rt.lib().yr_conv3x3_dgrad(r[0], dy.shape[3], r[1], *g, w[0], dx_ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [dy, wt], [(g[0], g[1], g[2], dx_ld)], [g[3]])[0]


def dev_wgrad(dev, x, dy, g, off=0, ws_fill=0xFF):
    rt = _rt()
    need = rt.conv3x3_wgrad_workspace_bytes(g[0], g[8], g[9], g[3], g[4])
    assert need > 0

    def launch(r, w, ws):
        rt.check(rt.lib().yr_conv3x3_wgrad(r[0], x.shape[3], r[1], dy.shape[3], *g, ws, need, w[0], rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [x, dy], [(9 * g[3], g[4])], [g[4]], ws_bytes=need, ws_fill=ws_fill)[0]


def _check_all(dev, seed, b, h, w, cin, cout, stride, padding, wide, off, wgrad=True):
    """the three entries on one case, bit for bit; wide: leading dimensions above the channels, NaN in the pad channels"""
    x, wt, dy, g = _case(seed, b, h, w, cin, cout, stride, padding)
    x_ld, y_ld = (cin + 2, cout + 3) if wide else (cin, cout)
    what = 'B=%d %dx%d %d->%d s=%d %s ld=(%d, %d) off=%d' % (b, h, w, cin, cout, stride, padding, x_ld, y_ld, off)
    got = dev_forward(dev, ref.padded(x, x_ld), wt, g, y_ld, off)
    assert np.array_equal(_bits(got[..., :cout]), _bits(ref.forward32(x, wt, stride, padding))), 'forward ' + what
    got = dev_dgrad(dev, ref.padded(dy, y_ld), wt, g, x_ld, off)
    assert np.array_equal(_bits(got[..., :cin]), _bits(ref.dgrad32(dy, wt, (h, w), stride, padding))), 'dgrad ' + what
    if wgrad:
        got = dev_wgrad(dev, ref.padded(x, x_ld), ref.padded(dy, y_ld), g, off)
        assert np.array_equal(_bits(got), _bits(ref.wgrad32(x, dy, stride, padding))), 'wgrad ' + what


# ----------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('cin,cout', CHANNELS)
def test_entries_equal_the_restatement(dev, cin, cout, stride):
    n = 0
    for h, w in MAPS:
        for b in BATCHES:
            for padding in ('same', ZERO_PAD):
                if padding != 'same' and (h + 1 < 3 or w + 1 < 3):
                    continue          # (the padded map is smaller than the kernel)
                n += 1
                _check_all(dev, 1000 * n + 10 * cout + cin, b, h, w, cin, cout, stride, padding, wide=n % 2 == 1, off=(n // 2) % 2)


@pytest.mark.parametrize('stride', [1, 2])
def test_workgroup_boundaries(dev, stride):
    """257 = T + 1 and 511 = 2 T - 1 outputs (and cells of the input gradient) for the T = 256 of both kernels: see the module text"""
    for i, (h, w) in enumerate(BOUNDARY_MAPS[stride]):
        _check_all(dev, 77 + i, 1, h, w, 3, 24, stride, 'same', wide=bool(i % 2), off=i % 2, wgrad=False)
    _check_all(dev, 99, 2, *BOUNDARY_MAPS[stride][2], 3, 24, stride, 'same', wide=False, off=0, wgrad=False)      # the second image begins inside a workgroup


# ----------------------------------------------------------------------------- the weight gradient's chunks
@pytest.mark.parametrize('cin,cout', CHUNK_CHANNELS)
def test_wgrad_chunk_edges(dev, cin, cout):
    for (b, h, w), what in CHUNK_CASES[:4]:
        x, wt, dy, g = _case(b * 1000 + h, b, h, w, cin, cout, 1, 'same')
        want = _bits(ref.wgrad32(x, dy, 1, 'same'))
        got = dev_wgrad(dev, x, dy, g, off=h % 2)
        assert np.array_equal(_bits(got), want), '%s: B=%d %dx%d %d->%d' % (what, b, h, w, cin, cout)
        again = dev_wgrad(dev, x, dy, g, off=h % 2, ws_fill=0x7F)          # another NaN pattern in the workspace: its contents do not matter
        assert np.array_equal(_bits(again), want), 'the same call gives the same bytes'


def test_wgrad_chunk_above_the_minimum(dev):
    (b, h, w), _ = CHUNK_CASES[4]
    x, wt, dy, g = _case(5, b, h, w, 1, 4, 1, 'same')
    assert _rt().conv3x3_wgrad_chunk(b, h, w, 1, 4) == 2
    got = dev_wgrad(dev, x, dy, g)
    assert np.array_equal(_bits(got), _bits(ref.wgrad32(x, dy, 1, 'same')))


# ----------------------------------------------------------------------------- against float64
@pytest.mark.parametrize('b,h,w,cin,cout,stride', ROUNDING_CASES)
def test_rounding_against_float64(dev, b, h, w, cin, cout, stride):
    """Measured on an MI355X (device = float32 restatement, bar): 40x37 3->24 s=2 forward 1.608e-07, 7.030e-07; dgrad 3.319e-07, 1.387e-06; wgrad
    1.918e-07, 8.269e-07;  30x30 3->48 s=1 forward 1.338e-07, 5.947e-07; dgrad 6.767e-07, 2.766e-06; wgrad 3.268e-07, 1.367e-06"""
    x, wt, dy, g = _case(h, b, h, w, cin, cout, stride, 'same')
    y64 = ref.forward64(x, wt, stride, 'same')
    dx64, dw64 = ref.grads64(x, wt, dy, stride, 'same')
    res = [('forward', dev_forward(dev, x, wt, g, cout), ref.forward32(x, wt, stride, 'same'), y64),
           ('dgrad', dev_dgrad(dev, dy, wt, g, cin), ref.dgrad32(dy, wt, (h, w), stride, 'same'), dx64),
           ('wgrad', dev_wgrad(dev, x, dy, g), ref.wgrad32(x, dy, stride, 'same'), dw64)]
    ok = [_within_bar('conv3x3 %s %dx%d %d->%d s=%d' % (name, h, w, cin, cout, stride), torch.from_numpy(got), r32, r64) for name, got, r32, r64 in res]
    assert all(ok)


# ----------------------------------------------------------------------------- autograd.conv3x3
@pytest.mark.parametrize('gx,gw', [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize('stride,padding', [(2, 'same'), (1, 'same'), (2, ZERO_PAD)])
def test_autograd_conv3x3(dev, monkeypatch, stride, padding, gx, gw):
    from yoloret_amd import autograd
    calls = Calls(monkeypatch, ['conv3x3_forward', 'conv3x3_dgrad', 'conv3x3_wgrad'])
    x, wt, dy, g = _case(7 + stride, 2, 7, 9, 3, 24, stride, padding)
    tx = torch.from_numpy(x).to(dev).requires_grad_(gx)
    tw = torch.from_numpy(wt).to(dev).requires_grad_(gw)
    y = autograd.conv3x3(tx, tw, stride=stride, padding=padding)
    assert tuple(y.shape) == (2, g[8], g[9], 24) and y.requires_grad == (gx or gw)
    assert np.array_equal(_bits(y.detach().cpu().numpy()), _bits(ref.forward32(x, wt, stride, padding)))
    if gx or gw:
        (y * torch.from_numpy(dy).to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert calls.n == {'conv3x3_forward': 1, 'conv3x3_dgrad': int(gx), 'conv3x3_wgrad': int(gw)}, 'a gradient nobody asks for launches nothing'
    if gx:
        assert np.array_equal(_bits(tx.grad.cpu().numpy()), _bits(ref.dgrad32(dy, wt, (7, 9), stride, padding)))
    else:
        assert tx.grad is None
    if gw:
        assert np.array_equal(_bits(tw.grad.cpu().numpy()), _bits(ref.wgrad32(x, dy, stride, padding)))
    else:
        assert tw.grad is None
