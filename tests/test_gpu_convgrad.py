"""The backward operators on the device (yoloret_amd/csrc/convgrad.hip behind yr_linear_dgrad, yr_depthwise_forward / _dgrad / _wgrad and
yr_bn_act_forward / _backward) against tests/convgrad_ref.py.

Every launch of a C entry runs between the guards of tests/fence.py with outputs and workspaces pre-filled with NaN.  As in
tests/test_gpu_headtrain.py the data of a case lives in a CARRIER (`off` NaN floats, the data, 63 NaN floats): off = 1 puts every
base pointer 4 (and 20) bytes past a 256-byte boundary.  The NaN floats around the data and in the pad columns of a written tensor
must keep their bytes.

Exact cases: integers in [-4, 4] (dyadic numbers for the BatchNorm), so every product and every partial sum is exact in float32
whatever the order: the result must equal the float64 result bit for bit.  Rounding cases: standard-normal inputs;
max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24 with E_ref the same figure of the float32 restatement.  Every rounding case
prints its figures before it asserts (run with -s); the measured ones are in the docstrings."""
import ctypes

import numpy as np
import pytest
import torch

from tests import convgrad_ref as ref, fence

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
YR_ERR_ARG = -1
NAN_BITS = np.float32(np.nan).view(np.uint32)
ACT_ID = {None: 0, 'relu6': 1, 'swish': 2}

DGRAD_PIXELS = [1, 3, 15, 16, 17, 69]
DGRAD_SHAPES = [(1, 1), (16, 16), (17, 15), (75, 75), (80, 75), (3, 256), (256, 3), (255, 255), (40, 130)]      # (cin, cout); the last: three tiles
DW_MAPS = [(1, 1), (2, 3), (5, 7), (13, 13), (16, 17), (6, 4), (3, 6)]      # (the last two: even widths, a whole column quartet and half of one)
DW_CHANNELS = [1, 3, 4, 5, 64, 67]
DW_FORMS = [(3, 1, 'same'), (3, 2, 'same'), (3, 2, 'mobilenet'), (5, 1, 'same'), (5, 2, 'same'), (5, 2, 'mobilenet')]      # (k, stride, padding)
DW_BATCHES = [1, 3]
DW_CHUNK_OW = 7              # the chunk cases: B = 1, a map of (rows x 7) outputs at stride 1
BN_PIXELS = [1, 63, 64, 65]
BN_CHANNELS = [1, 75, 256]


def _rt():
    from yoloret_amd import runtime
    return runtime


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _carrier(a, dev, off):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    host = np.full((off + a.size + 63,), np.nan, np.float32)
    host[off:off + a.size] = a
    return torch.from_numpy(host).to(dev), a.size


def _inner(carrier, n, off, shape):
    host = carrier.cpu().numpy()
    pad = np.concatenate([host[:off], host[off + n:]]).view(np.uint32)
    assert np.all(pad == NAN_BITS), 'floats around the data were written'
    return host[off:off + n].reshape(shape)


def fenced(dev, off, launch, reads, write_shapes, cols, ws_bytes=0, ws_fill=0xFF):
    """launch(read pointers, write pointers, workspace pointer) between the guards.  reads: arrays; write_shapes: the shapes of the
    outputs, NaN-prefilled; cols: per output the columns the entry may write (the rest of each row must stay NaN).  -> the outputs."""
    rt = _rt()
    cr = [_carrier(a, dev, off) for a in reads]
    cw = [_carrier(np.full(s, np.nan, np.float32), dev, off) for s in write_shapes]
    ws = torch.full((max(ws_bytes, 1),), ws_fill, dtype=torch.uint8, device=dev) if ws_bytes else None

    def at(moved, c):
        return ctypes.c_void_p(moved(c).data_ptr() + 4 * off)

    def call(moved):
        launch([at(moved, c) for c, _ in cr], [at(moved, c) for c, _ in cw], rt._ptr(moved(ws)) if ws is not None else None)
    with torch.cuda.device(dev):
        fence.run(call, writes=[c for c, _ in cw], reads=[c for c, _ in cr], scratch=[ws] if ws is not None else [])
    outs = []
    for (c, n), shape, ncol in zip(cw, write_shapes, cols):
        o = _inner(c, n, off, shape)
        assert np.all(_bits(o[..., ncol:]) == NAN_BITS), 'pad columns of an output were written'
        outs.append(o)
    return outs


# ----------------------------------------------------------------------------- launchers
def dev_linear_dgrad(dev, dy, wt, cin, cout, dx_ld, off=0):
    rt = _rt()
    pixels = dy.shape[0]

    def launch(r, w, _):
        rt.check(rt.lib().yr_linear_dgrad(r[0], dy.shape[1], r[1], pixels, cin, cout, w[0], dx_ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [dy, wt], [(pixels, dx_ld)], [cin])[0]


def _dw_args(x_shape, c, k, stride, padding):
    b, h, w = x_shape[:3]
    pads, (oh, ow) = ref.geometry(h, w, k, stride, padding)
    return (b, h, w, c, k, stride, pads[0], pads[1], oh, ow)


def dev_dw_forward(dev, x, w, c, k, stride, padding, y_ld, off=0):
    rt = _rt()
    g = _dw_args(x.shape, c, k, stride, padding)

    def launch(r, wr, _):
        rt.check(rt.lib().yr_depthwise_forward(r[0], x.shape[3], r[1], *g, wr[0], y_ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [x, w], [(g[0], g[8], g[9], y_ld)], [c])[0]


def dev_dw_dgrad(dev, dy, w, hw, c, k, stride, padding, dx_ld, off=0):
    rt = _rt()
    g = _dw_args((dy.shape[0], hw[0], hw[1]), c, k, stride, padding)
    assert dy.shape[1:3] == (g[8], g[9])

    def launch(r, wr, _):
        rt.check(rt.lib().yr_depthwise_dgrad(r[0], dy.shape[3], r[1], *g, wr[0], dx_ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [dy, w], [(g[0], hw[0], hw[1], dx_ld)], [c])[0]


def dev_dw_wgrad(dev, x, dy, c, k, stride, padding, off=0, ws_fill=0xFF):
    rt = _rt()
    g = _dw_args(x.shape, c, k, stride, padding)
    need = rt.depthwise_wgrad_workspace_bytes(g[0], g[8], g[9], c, k)
    assert need > 0

    def launch(r, wr, ws):
        rt.check(rt.lib().yr_depthwise_wgrad(r[0], x.shape[3], r[1], dy.shape[3], *g, ws, need, wr[0], rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [x, dy], [(k * k, c)], [c], ws_bytes=need, ws_fill=ws_fill)[0]


def dev_bn_forward(dev, z, scale, shift, c, act, ld, off=0, keep_u=True):
    rt = _rt()
    pixels = z.shape[0]

    def launch(r, w, _):
        rt.check(rt.lib().yr_bn_act_forward(r[0], z.shape[1], r[1], r[2], pixels, c, ACT_ID[act], w[0], ld, w[1] if keep_u else None, ld,
                                            rt.stream_ptr(dev)))
    outs = fenced(dev, off, launch, [z, scale, shift], [(pixels, ld)] * (2 if keep_u else 1), [c] * (2 if keep_u else 1))
    return outs if keep_u else outs[0]


def dev_bn_backward(dev, da, u, scale, c, act, ld, off=0):
    rt = _rt()
    pixels = da.shape[0]

    def launch(r, w, _):
        rt.check(rt.lib().yr_bn_act_backward(r[0], da.shape[1], r[1], u.shape[1], r[2], pixels, c, ACT_ID[act], w[0], ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [da, u, scale], [(pixels, ld)], [c])[0]


# ----------------------------------------------------------------------------- 1x1 input gradient
@pytest.mark.parametrize('cin,cout', DGRAD_SHAPES)
def test_linear_dgrad_exact_integers(dev, cin, cout):
    rng = np.random.default_rng(1000 * cin + cout)
    w = ref.ints(rng, (cout, cin))
    kp = (cin + 3) // 4 * 4
    wt = ref.padded(w, kp)                       # NaN in the pad columns: they are not read
    for i, pixels in enumerate(DGRAD_PIXELS):
        dy = ref.ints(rng, (pixels, cout))
        want = (dy.astype(np.float64) @ w.astype(np.float64)).astype(np.float32)
        if i == 0:
            assert np.array_equal(want, ref.linear_grads(np.zeros((pixels, cin)), w, dy)[0])      # the restatement says the same
        for j, (dy_ld, dx_ld) in enumerate(((cout, cin), (cout + 1, cin + 3))):
            got = dev_linear_dgrad(dev, ref.padded(dy, dy_ld), wt, cin, cout, dx_ld, off=(i + j) % 2)
            assert np.array_equal(_bits(got[:, :cin]), _bits(want)), 'P=%d cin=%d cout=%d dy_ld=%d dx_ld=%d' % (pixels, cin, cout, dy_ld, dx_ld)


@pytest.mark.parametrize('cin,cout', [(75, 75), (255, 255)])
def test_linear_dgrad_rounding(dev, cin, cout):
    """Measured on an MI355X, P = 2704 standard-normal rows: 75 <- 75 device 4.023e-07, E_ref 4.023e-07, bar 1.669e-06; 255 <- 255 device
    6.709e-07, E_ref 6.709e-07, bar 2.743e-06 (the largest deviations are final roundings that both orders share)."""
    pixels = 2704
    rng = np.random.default_rng(17)
    dy = rng.standard_normal((pixels, cout)).astype(np.float32)
    w = (rng.standard_normal((cout, cin)) / np.sqrt(cout)).astype(np.float32)
    x0 = np.zeros((pixels, cin), np.float32)
    r64 = ref.linear_grads(x0, w, dy)[0]
    e_ref = ref.rel_err(ref.linear_grads(x0, w, dy, np.float32)[0], r64)
    got = dev_linear_dgrad(dev, dy, ref.pack_wt(w), cin, cout, cin)
    e_dev = ref.rel_err(got, r64)
    print('linear_dgrad %d<-%d P=%d: device %.3e, float32 restatement %.3e, bar %.3e' % (cin, cout, pixels, e_dev, e_ref, 4 * e_ref + EPS24))
    assert e_dev <= 4 * e_ref + EPS24


# ----------------------------------------------------------------------------- depthwise
def _dw_case(rng, b, h, w, c, k, stride, padding, ints=True):
    _, (oh, ow) = ref.geometry(h, w, k, stride, padding)
    draw = (lambda s: ref.ints(rng, s)) if ints else (lambda s: rng.standard_normal(s).astype(np.float32))
    return draw((b, h, w, c)), draw((k * k, c)), draw((b, oh, ow, c))


@pytest.mark.parametrize('k,stride,padding', DW_FORMS)
def test_depthwise_exact_integers(dev, k, stride, padding):
    n = 0
    for h, w in DW_MAPS:
        for c in DW_CHANNELS:
            for b in DW_BATCHES:
                rng = np.random.default_rng(h * 100000 + w * 1000 + c * 10 + b)
                x, taps, dy = _dw_case(rng, b, h, w, c, k, stride, padding)
                y64 = ref.depthwise(x, taps, k, stride, padding)
                dx64, dw64 = ref.depthwise_grads(x, taps, dy, k, stride, padding)
                n += 1
                off, ld = n % 2, c + (n // 2) % 2 * 3          # dense / padded rows and both alignments, alternating
                what = '%dx%d C=%d B=%d k=%d s=%d %s ld=%d' % (h, w, c, b, k, stride, padding, ld)
                got = dev_dw_forward(dev, ref.padded(x, ld), taps, c, k, stride, padding, ld, off)
                assert np.array_equal(_bits(got[..., :c]), _bits(y64)), 'forward ' + what
                got = dev_dw_dgrad(dev, ref.padded(dy, ld), taps, (h, w), c, k, stride, padding, ld, off)
                assert np.array_equal(_bits(got[..., :c]), _bits(dx64)), 'dgrad ' + what
                got = dev_dw_wgrad(dev, ref.padded(x, ld), ref.padded(dy, ld), c, k, stride, padding, off)
                assert np.array_equal(_bits(got), _bits(dw64)), 'wgrad ' + what


def dw_chunk_rows():
    """output-row counts around the chunk the library reports for a (rows x DW_CHUNK_OW) output at B = 1"""
    rt = _rt()
    chunk = rt.depthwise_wgrad_chunk(1, 1, DW_CHUNK_OW, 5, 3)
    rows = [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    assert all(rt.depthwise_wgrad_chunk(1, r, DW_CHUNK_OW, 5, 3) == chunk for r in rows)
    return chunk, rows


@pytest.mark.parametrize('k', [3, 5])
def test_depthwise_wgrad_chunk_edges(dev, k):
    chunk, rows = dw_chunk_rows()
    for r in rows:
        for b in (1, 2):
            rng = np.random.default_rng(r * 10 + b)
            x, _, dy = _dw_case(rng, b, r, DW_CHUNK_OW, 5, k, 1, 'same')
            _, dw64 = ref.depthwise_grads(x, np.zeros((k * k, 5)), dy, k, 1, 'same')
            got = dev_dw_wgrad(dev, x, dy, 5, k, 1, 'same')
            assert np.array_equal(_bits(got), _bits(dw64)), 'rows %d (chunk %d) B=%d k=%d' % (r, chunk, b, k)


@pytest.mark.parametrize('g,c', [(13, 512), (26, 256)])
def test_depthwise_rounding(dev, g, c):
    """3x3, stride 1, 'same', batch 2, standard-normal data.  Measured on an MI355X (device, E_ref, bar):
    13x13x512  forward 1.112e-07, 1.112e-07, 5.046e-07;  dgrad 1.451e-07, 1.451e-07, 6.400e-07;  wgrad 9.826e-08, 3.300e-07, 1.379e-06
    26x26x256  forward 1.125e-07, 1.125e-07, 5.097e-07;  dgrad 1.245e-07, 1.245e-07, 5.577e-07;  wgrad 1.518e-07, 4.642e-07, 1.917e-06"""
    rng = np.random.default_rng(g)
    x, taps, dy = _dw_case(rng, 2, g, g, c, 3, 1, 'same', ints=False)
    y64 = ref.depthwise(x, taps, 3, 1, 'same')
    dx64, dw64 = ref.depthwise_grads(x, taps, dy, 3, 1, 'same')
    dx32, dw32 = ref.depthwise_grads(x, taps, dy, 3, 1, 'same', np.float32)
    res = [('forward', dev_dw_forward(dev, x, taps, c, 3, 1, 'same', c), ref.depthwise(x, taps, 3, 1, 'same', np.float32), y64),
           ('dgrad', dev_dw_dgrad(dev, dy, taps, (g, g), c, 3, 1, 'same', c), dx32, dx64),
           ('wgrad', dev_dw_wgrad(dev, x, dy, c, 3, 1, 'same'), dw32, dw64)]
    bad = []
    for name, got, r32, r64 in res:
        e_dev, e_ref = ref.rel_err(got, r64), ref.rel_err(r32, r64)
        print('depthwise %s %dx%dx%d: device %.3e, float32 restatement %.3e, bar %.3e' % (name, g, g, c, e_dev, e_ref, 4 * e_ref + EPS24))
        if not e_dev <= 4 * e_ref + EPS24:
            bad.append(name)
    assert not bad


def test_depthwise_batch_independence(dev):
    for k, stride, padding in ((3, 2, 'mobilenet'), (5, 1, 'same')):
        rng = np.random.default_rng(k)
        x, taps, dy = _dw_case(rng, 3, 5, 7, 67, k, stride, padding, ints=False)
        y3 = dev_dw_forward(dev, x, taps, 67, k, stride, padding, 67)
        y1 = dev_dw_forward(dev, x[:1], taps, 67, k, stride, padding, 67)
        assert np.array_equal(_bits(y3[0]), _bits(y1[0]))
        d3 = dev_dw_dgrad(dev, dy, taps, (5, 7), 67, k, stride, padding, 67)
        d1 = dev_dw_dgrad(dev, dy[:1], taps, (5, 7), 67, k, stride, padding, 67)
        assert np.array_equal(_bits(d3[0]), _bits(d1[0]))


def test_same_call_same_bytes(dev):
    rt = _rt()
    rng = np.random.default_rng(9)
    chunk, rows = dw_chunk_rows()
    x, taps, dy = _dw_case(rng, 2, rows[-1], DW_CHUNK_OW, 67, 3, 1, 'same', ints=False)
    first = [dev_dw_wgrad(dev, x, dy, 67, 3, 1, 'same', ws_fill=f) for f in (0xFF, 0x7B)]
    assert np.isfinite(first[0]).all() and np.array_equal(_bits(first[0]), _bits(first[1]))
    tx, tdy, tw = (torch.from_numpy(a).to(dev) for a in (x, dy, taps))
    need = rt.depthwise_wgrad_workspace_bytes(2, rows[-1], DW_CHUNK_OW, 67, 3)
    ws = torch.empty((need + 64,), dtype=torch.uint8, device=dev).random_(0, 256)
    out = torch.full((9, 67), float('nan'), dtype=torch.float32, device=dev)
    assert rt.depthwise_wgrad(tx, tdy, 3, out=out, workspace=ws) is out
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(first[0]))
    assert np.array_equal(_bits(rt.depthwise_wgrad(tx, tdy, 3).cpu().numpy()), _bits(first[0]))
    # the one-launch entries: the wrapper twice, and against the fenced call
    for fn, fenced_result in ((lambda: rt.depthwise_forward(tx, tw), dev_dw_forward(dev, x, taps, 67, 3, 1, 'same', 67)),
                              (lambda: rt.depthwise_dgrad(tdy, tw, x.shape[1:3]), dev_dw_dgrad(dev, dy, taps, x.shape[1:3], 67, 3, 1, 'same', 67))):
        a, b = fn().cpu().numpy(), fn().cpu().numpy()
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(fenced_result))
    w = rng.standard_normal((75, 67)).astype(np.float32)
    twt = torch.from_numpy(ref.pack_wt(w)).to(dev)
    d = torch.from_numpy(rng.standard_normal((69, 75)).astype(np.float32)).to(dev)
    a, b = rt.linear_dgrad(d, twt, 67).cpu().numpy(), rt.linear_dgrad(d, twt, 67).cpu().numpy()
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(a), _bits(dev_linear_dgrad(dev, d.cpu().numpy(), ref.pack_wt(w), 67, 75, 67)))


# ----------------------------------------------------------------------------- frozen BatchNorm + activation
BN_SCALES = np.array([1.0, -1.0, 0.0, 0.5, 2.0, 1.5, -0.5], np.float32)
BN_SHIFTS = np.array([0.0, 2.0, 6.0, -1.0, 3.0], np.float32)


def bn_exact_case(pixels, c):
    """dyadic z, scale and shift: u is exact; element (0, 0) has u = 0 exactly and the next element (row-major) u = 6 exactly"""
    rng = np.random.default_rng(pixels * 1000 + c)
    z = ref.ints(rng, (pixels, c))
    scale = BN_SCALES[np.arange(c) % len(BN_SCALES)].copy()
    shift = BN_SHIFTS[np.arange(c) % len(BN_SHIFTS)].copy()
    z[0, 0] = 0.0                                   # channel 0: scale 1, shift 0 -> u = 0
    if c > 1:
        z[0, 1] = -4.0                              # channel 1: scale -1, shift 2 -> u = 6
    elif pixels > 1:
        z[1, 0] = 6.0
    da = ref.ints(rng, (pixels, c))
    return z, scale, shift, da


@pytest.mark.parametrize('act', [None, 'relu6', 'swish'])
def test_bn_act_exact_dyadic(dev, act):
    n = 0
    for pixels in BN_PIXELS:
        for c in BN_CHANNELS:
            z, scale, shift, da = bn_exact_case(pixels, c)
            a64, u64 = ref.bn_act(z, scale, shift, act)
            assert (u64 == 0).any() and ((u64 == 6).any() or pixels * c == 1)
            if c >= len(BN_SCALES):
                assert (scale < 0).any() and (scale == 0).any()
            dz64 = ref.bn_act_backward(da, u64, scale, act)
            n += 1
            off, ld = n % 2, c + (n // 2) % 2 * 3
            a, u = dev_bn_forward(dev, ref.padded(z, ld), scale, shift, c, act, ld, off)
            a_only = dev_bn_forward(dev, ref.padded(z, ld), scale, shift, c, act, ld, off, keep_u=False)
            assert np.array_equal(_bits(a[:, :c]), _bits(a_only[:, :c]))
            assert np.array_equal(_bits(u[:, :c]), _bits(u64)), 'u P=%d C=%d' % (pixels, c)
            dz = dev_bn_backward(dev, ref.padded(da, ld), u, scale, c, act, ld, off)
            if act == 'swish':
                assert float(np.abs(u64).max()) < 87.0          # below the clamp of the forward's expf
                a32, _ = ref.bn_act(z, scale, shift, act, np.float32)
                dz32 = ref.bn_act_backward(da, u64, scale, act, np.float32)
                for name, got, r32, r64 in (('a', a[:, :c], a32, a64), ('dz', dz[:, :c], dz32, dz64)):
                    if np.abs(r64).max() == 0:
                        assert not got.any()
                        continue
                    e_dev, e_ref = ref.rel_err(got, r64), ref.rel_err(r32, r64)
                    assert e_dev <= 4 * e_ref + EPS24, 'swish %s P=%d C=%d: device %.3e, E_ref %.3e' % (name, pixels, c, e_dev, e_ref)
                tie = u64 == 0                                  # Swish'(0) = 1 / 2 exactly
                assert np.array_equal(dz[:, :c][tie], ((da * np.float32(0.5)) * scale[None, :])[tie])
            else:
                assert np.array_equal(a[:, :c], a64.astype(np.float32)), 'a P=%d C=%d' % (pixels, c)
                assert np.array_equal(_bits(dz[:, :c]), _bits(dz64)), 'dz P=%d C=%d' % (pixels, c)
                if act == 'relu6':
                    assert not dz[:, :c][(u64 == 0) | (u64 == 6)].any(), 'ReLU6 passes no gradient AT 0 and 6'
    if act is None:     # the derivative of the affine alone reads no u
        rt = _rt()
        z, scale, shift, da = bn_exact_case(65, 75)
        got = rt.bn_act_backward(torch.from_numpy(da).to(dev), None, torch.from_numpy(scale).to(dev), None)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(da * scale[None, :]))


def test_bn_act_relu6_gives_plus_zero_outside_the_open_interval(dev):
    """dz is +0 (bit pattern 0x00000000) wherever u is not inside (0, 6): at 0, at 6, below and above, under a negative scale too.
    (A kernel that formed g = da * act'(u) first and multiplied by the scale afterwards would write 0 * -2 = -0 there.)"""
    u = np.array([[0.0, 6.0, -1.0, 7.0, 3.0],
                  [6.0, 0.0, 7.0, -1.0, 0.0],
                  [-2.5, 8.0, 0.0, 6.0, 6.0]], np.float32)
    scale = np.array([1.0, -2.0, 0.5, 3.0, 1.5], np.float32)          # channel 1: u = 6, 0 and 8 under a negative scale
    da = np.array([[1.0, -2.0, 3.0, -4.0, 2.0],
                   [-1.0, 2.0, -3.0, 4.0, -2.0],
                   [2.0, 3.0, -1.0, 1.0, -3.0]], np.float32)
    outside = ~((u > 0) & (u < 6))
    assert outside.sum() == 14 and not outside[0, 4]
    want = ref.bn_act_backward(da, u, scale, 'relu6')
    assert np.all(_bits(want)[outside] == 0) and want[0, 4] == 3.0, 'the definition itself: +0 outside'
    dz = dev_bn_backward(dev, da, u, scale, 5, 'relu6', 5)
    assert np.all(_bits(dz)[outside] == 0), 'bits %s' % [hex(b) for b in _bits(dz)[outside]]
    assert np.array_equal(_bits(dz), _bits(want))


def test_bn_act_swish_rounding(dev):
    """Standard-normal z (x 3), P = 65, C = 75.  Measured on an MI355X (device, E_ref, bar): a 8.120e-08, 8.120e-08, 3.844e-07;
    dz 2.640e-07, 2.640e-07, 1.116e-06."""
    rng = np.random.default_rng(21)
    z = (3 * rng.standard_normal((65, 75))).astype(np.float32)
    scale, shift = rng.uniform(-2, 2, 75).astype(np.float32), rng.standard_normal(75).astype(np.float32)
    da = rng.standard_normal((65, 75)).astype(np.float32)
    a64, u64 = ref.bn_act(z, scale, shift, 'swish')
    assert float(np.abs(u64).max()) < 87.0
    a, u = dev_bn_forward(dev, z, scale, shift, 75, 'swish', 75)
    dz = dev_bn_backward(dev, da, u, scale, 75, 'swish', 75)
    a32, u32 = ref.bn_act(z, scale, shift, 'swish', np.float32)
    assert np.array_equal(_bits(u), _bits(u32)), 'u is one float32 multiply and one float32 add'
    dz64, dz32 = ref.bn_act_backward(da, u, scale, 'swish'), ref.bn_act_backward(da, u, scale, 'swish', np.float32)
    bad = []
    for name, got, r32, r64 in (('a', a, a32, a64), ('dz', dz, dz32, dz64)):
        e_dev, e_ref = ref.rel_err(got, r64), ref.rel_err(r32, r64)
        print('bn_act swish %s: device %.3e, float32 restatement %.3e, bar %.3e' % (name, e_dev, e_ref, 4 * e_ref + EPS24))
        if not e_dev <= 4 * e_ref + EPS24:
            bad.append(name)
    assert not bad


# ----------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(dev):
    rt = _rt()
    L = rt.lib()
    p, s = rt._ptr, rt.stream_ptr(dev)
    nan = float('nan')
    pixels, cin, cout, kp = 40, 75, 75, 76
    dy = torch.zeros((pixels, cout), dtype=torch.float32, device=dev)
    wt = torch.zeros((cout, kp), dtype=torch.float32, device=dev)
    dx = torch.full((pixels, cin), nan, dtype=torch.float32, device=dev)
    dgrad = [
        ('cin 0', (p(dy), cout, p(wt), pixels, 0, cout, p(dx), cin, s)),
        ('cin 257', (p(dy), cout, p(wt), pixels, 257, cout, p(dx), 300, s)),
        ('cout 0', (p(dy), cout, p(wt), pixels, cin, 0, p(dx), cin, s)),
        ('cout 257', (p(dy), 300, p(wt), pixels, cin, 257, p(dx), cin, s)),
        ('pixels 0', (p(dy), cout, p(wt), 0, cin, cout, p(dx), cin, s)),
        ('pixels 2^40', (p(dy), cout, p(wt), 1 << 40, cin, cout, p(dx), cin, s)),
        ('dy_ld < cout', (p(dy), cout - 1, p(wt), pixels, cin, cout, p(dx), cin, s)),
        ('dx_ld < cin', (p(dy), cout, p(wt), pixels, cin, cout, p(dx), cin - 1, s)),
        ('null dy', (None, cout, p(wt), pixels, cin, cout, p(dx), cin, s)),
        ('null wt', (p(dy), cout, None, pixels, cin, cout, p(dx), cin, s)),
        ('null dx', (p(dy), cout, p(wt), pixels, cin, cout, None, cin, s)),
        ('dx not 4-byte aligned', (p(dy), cout, p(wt), pixels - 1, cin, cout, ctypes.c_void_p(dx.data_ptr() + 2), cin, s)),
    ]
    b, h, w, c, k = 2, 5, 7, 8, 3
    x = torch.zeros((b, h, w, c), dtype=torch.float32, device=dev)
    taps = torch.zeros((25, c), dtype=torch.float32, device=dev)
    y = torch.full((b, h, w, c), nan, dtype=torch.float32, device=dev)
    dw = torch.full((25, c), nan, dtype=torch.float32, device=dev)
    need = rt.depthwise_wgrad_workspace_bytes(b, h, w, c, k)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)

    def geo(**kw):
        g = dict(B=b, H=h, W=w, C=c, k=k, stride=1, pt=1, pl=1, OH=h, OW=w)
        g.update(kw)
        return tuple(g[n] for n in ('B', 'H', 'W', 'C', 'k', 'stride', 'pt', 'pl', 'OH', 'OW'))
    bad_geo = [('k 4', geo(k=4)), ('k 7', geo(k=7)), ('stride 3', geo(stride=3)), ('stride 0', geo(stride=0)), ('OH too large', geo(OH=h + 2)),
               ('OW too large', geo(OW=w + 2)), ('OH too small', geo(OH=h - 2)),      # (h + 1: a bottom pad of 2; h - 1: none - both consistent) ('stride-2 output at stride 1', geo(OH=3, OW=4)),
               ('pad_top 3', geo(pt=3)), ('pad_left -1', geo(pl=-1)), ('B 0', geo(B=0)), ('C 0', geo(C=0)), ('H 0', geo(H=0))]
    fwd = [(what, (p(x), c, p(taps)) + g + (p(y), c, s)) for what, g in bad_geo]
    fwd += [('x_ld < C', (p(x), c - 1, p(taps)) + geo() + (p(y), c, s)), ('y_ld < C', (p(x), c, p(taps)) + geo() + (p(y), c - 1, s)),
            ('null x', (None, c, p(taps)) + geo() + (p(y), c, s)), ('null w', (p(x), c, None) + geo() + (p(y), c, s)),
            ('null y', (p(x), c, p(taps)) + geo() + (None, c, s))]
    wg = [(what, (p(x), c, p(x), c) + g + (p(ws), need, p(dw), s)) for what, g in bad_geo]
    wg += [('short workspace', (p(x), c, p(x), c) + geo() + (p(ws), need - 1, p(dw), s)),
           ('misaligned workspace', (p(x), c, p(x), c) + geo() + (ctypes.c_void_p(ws.data_ptr() + 4), need, p(dw), s)),
           ('null workspace', (p(x), c, p(x), c) + geo() + (None, need, p(dw), s)), ('null dw', (p(x), c, p(x), c) + geo() + (p(ws), need, None, s))]
    sc = torch.zeros((c,), dtype=torch.float32, device=dev)
    z2, a2 = x.reshape(-1, c), y.reshape(-1, c)
    n = z2.shape[0]
    bnf = [('act 3', (p(z2), c, p(sc), p(sc), n, c, 3, p(a2), c, None, c, s)), ('act -1', (p(z2), c, p(sc), p(sc), n, c, -1, p(a2), c, None, c, s)),
           ('pixels 0', (p(z2), c, p(sc), p(sc), 0, c, 1, p(a2), c, None, c, s)), ('C 0', (p(z2), c, p(sc), p(sc), n, 0, 1, p(a2), c, None, c, s)),
           ('a_ld < C', (p(z2), c, p(sc), p(sc), n, c, 1, p(a2), c - 1, None, c, s)), ('u_ld < C', (p(z2), c, p(sc), p(sc), n, c, 1, p(a2), c, p(a2), c - 1, s)),
           ('null scale', (p(z2), c, None, p(sc), n, c, 1, p(a2), c, None, c, s)), ('null a', (p(z2), c, p(sc), p(sc), n, c, 1, None, c, None, c, s))]
    bnb = [('act 4', (p(z2), c, p(z2), c, p(sc), n, c, 4, p(a2), c, s)), ('null u for ReLU6', (p(z2), c, None, c, p(sc), n, c, 1, p(a2), c, s)),
           ('pixels -1', (p(z2), c, p(z2), c, p(sc), -1, c, 2, p(a2), c, s)), ('dz_ld < C', (p(z2), c, p(z2), c, p(sc), n, c, 2, p(a2), c - 1, s)),
           ('null dz', (p(z2), c, p(z2), c, p(sc), n, c, 2, None, c, s))]
    with torch.cuda.device(dev):
        for entry, cases in ((L.yr_linear_dgrad, dgrad), (L.yr_depthwise_forward, fwd), (L.yr_depthwise_dgrad, fwd), (L.yr_depthwise_wgrad, wg),
                             (L.yr_bn_act_forward, bnf), (L.yr_bn_act_backward, bnb)):
            for what, args in cases:
                assert entry(*args) == YR_ERR_ARG, what
                assert L.yr_last_error()
    torch.cuda.synchronize()
    for t in (dx, y, dw):
        assert np.all(_bits(t.cpu().numpy()) == NAN_BITS)
    assert bool((ws == 0xFF).all()) and not bool(x.any()) and not bool(taps.any()) and not bool(dy.any()) and not bool(wt.any())
    for bad in ((0, 5, 7, 8, 3), (2, 5, 7, 8, 4), (2, 0, 7, 8, 3), (2, 5, 7, 0, 5)):
        assert rt.depthwise_wgrad_chunk(*bad) == 0 and rt.depthwise_wgrad_workspace_bytes(*bad) == 0
    # the binding's own checks
    with pytest.raises(ValueError):
        rt.linear_dgrad(dy, wt[:, :75].contiguous(), 75)
    with pytest.raises(ValueError):
        rt.linear_dgrad(dy, wt, 75, out=torch.empty((pixels, 76), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        rt.depthwise_forward(x, taps[:16].contiguous())
    with pytest.raises(ValueError):
        rt.depthwise_forward(x, taps, stride=3)
    with pytest.raises(ValueError):
        rt.depthwise_forward(x, taps, padding='valid')
    with pytest.raises(ValueError):
        rt.depthwise_dgrad(x, taps, (h + 1, w))
    with pytest.raises(ValueError):
        rt.depthwise_wgrad(x, x, 3, workspace=torch.empty(16, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        rt.bn_act_forward(z2, sc, sc, 'sigmoid')
    with pytest.raises(ValueError):
        rt.bn_act_backward(z2, None, sc, 'relu6')
    with pytest.raises(ValueError):
        rt.bn_act_forward(z2.cpu(), sc, sc, None)
