"""The wide 1x1 operators on the device (yoloret_amd/csrc/linearwide.hip behind yr_linear_wide_forward / _dgrad / _wgrad) against float64
NumPy, on the case lists of tests/linearwide_ref.py (tests/test_linearwide_host.py shows that they reach every instantiation).

Every launch of a C entry runs between the guards of tests/fence.py.  As in tests/test_gpu_convgrad.py the data of a case lives in
a CARRIER (`off` NaN floats, the data, 63 NaN floats): off = 1 puts every base pointer 4 (and 20) bytes past a 256-byte boundary.
Every row has one NaN pad column (ld = channels + 1) that must keep its NaN, the pad columns of wt hold NaN (they are never read),
outputs are pre-filled with NaN, and the weight gradient runs twice, on a workspace of 0xFF bytes and on one of random bytes: the
same bytes must come out.

Exact cases: integers in [-4, 4]: every partial sum is an integer of at most 16 * 1024 (the products) or 16 * pixels < 2^24 (the
gradient), exact in float32 in any order: the result must equal the float64 result bit for bit.  Rounding cases: standard-normal data;
max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24 with E_ref the same figure of NumPy's float32 product on the same data.  Every
rounding case prints its figures before it asserts (run with -s); the measured ones are in the docstrings."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fence, headtrain_ref as href, linearwide_ref as ref

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
YR_ERR_ARG = -1
NAN_BITS = np.float32(np.nan).view(np.uint32)


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


def fenced(dev, off, launch, reads, write_shape, cols, ws=None):
    """launch(read pointers, write pointer, workspace pointer) between the guards; the output is NaN-prefilled and only its first
    `cols` columns may change.  -> the output."""
    rt = _rt()
    cr = [_carrier(a, dev, off) for a in reads]
    cw, n = _carrier(np.full(write_shape, np.nan, np.float32), dev, off)

    def at(moved, c):
        return ctypes.c_void_p(moved(c).data_ptr() + 4 * off)

    def call(moved):
        launch([at(moved, c) for c, _ in cr], at(moved, cw), rt._ptr(moved(ws)) if ws is not None else None)
    with torch.cuda.device(dev):
        fence.run(call, writes=[cw], reads=[c for c, _ in cr], scratch=[ws] if ws is not None else [])
    out = _inner(cw, n, off, write_shape)
    assert np.all(_bits(out[..., cols:]) == NAN_BITS), 'pad columns of an output were written'
    return out


def _name():
    return _rt().lib().yr_last_kernel().decode()


def dev_forward(dev, x, wt, cin, cout, off=0):
    rt = _rt()
    pixels = x.shape[0]

    def launch(r, w, _):
        rt.check(rt.lib().yr_linear_wide_forward(r[0], x.shape[1], r[1], pixels, cin, cout, w, cout + 1, rt.stream_ptr(dev)))
    out = fenced(dev, off, launch, [x, wt], (pixels, cout + 1), cout)
    assert _name() == ref.kernel_names(cin, cout)[0]
    return out[:, :cout]


def dev_dgrad(dev, dy, wt, cin, cout, off=0):
    rt = _rt()
    pixels = dy.shape[0]

    def launch(r, w, _):
        rt.check(rt.lib().yr_linear_wide_dgrad(r[0], dy.shape[1], r[1], pixels, cin, cout, w, cin + 1, rt.stream_ptr(dev)))
    out = fenced(dev, off, launch, [dy, wt], (pixels, cin + 1), cin)
    assert _name() == ref.kernel_names(cin, cout)[1]
    return out[:, :cin]


def dev_wgrad(dev, x, dy, cin, cout, off=0, fill='ff'):
    rt = _rt()
    pixels = x.shape[0]
    need = rt.linear_wide_wgrad_workspace_bytes(pixels, cin, cout)
    assert need == ref.workspace_bytes(pixels, cin, cout) > 0
    if fill == 'ff':
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    else:
        gen = torch.Generator(device=dev)
        gen.manual_seed(pixels + cin)
        ws = torch.randint(0, 256, (need,), dtype=torch.uint8, device=dev, generator=gen)

    def launch(r, w, wsp):
        rt.check(rt.lib().yr_linear_wide_wgrad(r[0], x.shape[1], r[1], dy.shape[1], pixels, cin, cout, wsp, need, w, rt.stream_ptr(dev)))
    out = fenced(dev, off, launch, [x, dy], (cout, ref.kp_of(cin)), ref.kp_of(cin), ws=ws)
    assert _name() == ref.kernel_names(cin, cout)[2]      # (stage 2 is one kernel for the library and notes no name)
    return out


def _padded(a, ld):
    out = np.full(a.shape[:-1] + (ld,), np.nan, np.float32)
    out[..., :a.shape[-1]] = a
    return out


def _wgrad_both_fills(dev, x, dy, cin, cout, off, what):
    a = dev_wgrad(dev, x, dy, cin, cout, off, 'ff')
    b = dev_wgrad(dev, x, dy, cin, cout, off, 'random')
    assert np.array_equal(_bits(a), _bits(b)), 'the workspace\'s bytes reached the result: ' + what
    return a


def _check_exact(dev, cin, cout, pixel_counts, entries=('forward', 'dgrad', 'wgrad')):
    w, wt = ref.int_weights(1000 * cin + cout, cin, cout)
    kp = ref.kp_of(cin)
    for i, pixels in enumerate(pixel_counts):
        off = i % 2
        x, dy = href.int_case(7 * pixels + cin, pixels, cin, cout, cin + 1, cout + 1)      # one NaN pad column per row
        what = 'P=%d cin=%d cout=%d off=%d' % (pixels, cin, cout, off)
        if 'forward' in entries:
            want = href.forward64(x[:, :cin], w).astype(np.float32)
            assert np.array_equal(_bits(dev_forward(dev, x, wt, cin, cout, off)), _bits(want)), 'forward ' + what
        if 'dgrad' in entries:
            want = (dy[:, :cout].astype(np.float64) @ w.astype(np.float64)).astype(np.float32)
            assert np.array_equal(_bits(dev_dgrad(dev, dy, wt, cin, cout, off)), _bits(want)), 'dgrad ' + what
        if 'wgrad' in entries:
            want = np.zeros((cout, kp), np.float32)      # pad columns +0
            want[:, :cin] = href.wgrad64(x[:, :cin], dy[:, :cout])
            assert np.array_equal(_bits(_wgrad_both_fills(dev, x, dy, cin, cout, off, what)), _bits(want)), 'wgrad ' + what


# ----------------------------------------------------------------------------- exact
@pytest.mark.parametrize('cin,cout', ref.EXACT_SHAPES)
def test_exact_integers(dev, cin, cout):
    _check_exact(dev, cin, cout, ref.PIXELS)


@pytest.mark.parametrize('cin,cout', ref.MODEL_SHAPES + ref.EDGE_SHAPES + [ref.CAP_SHAPE] + ref.NARROW_SHAPES)
def test_wgrad_exact_across_chunks(dev, cin, cout):
    rt = _rt()
    c = ref.min_chunk(cin, cout)
    counts = ref.wgrad_pixels(cin, cout)[len(ref.PIXELS):]
    assert counts == [c + 1, 2 * c + 5] and all(rt.linear_wide_wgrad_chunk(p, cin, cout) == c for p in counts)
    _check_exact(dev, cin, cout, counts, entries=('wgrad',))


def test_wgrad_exact_where_the_chunk_leaves_its_minimum(dev):
    rt = _rt()
    cin, cout = ref.NARROWEST_WIDE
    pixels = ref.FIRST_GROWN_PIXELS
    assert rt.linear_wide_wgrad_chunk(pixels - 1, cin, cout) == ref.MIN_CHUNK == ref.min_chunk(cin, cout)
    assert rt.linear_wide_wgrad_chunk(pixels, cin, cout) == ref.MIN_CHUNK + ref.CHUNK_STEP
    _check_exact(dev, cin, cout, [pixels], entries=('wgrad',))


# ----------------------------------------------------------------------------- rounding
def _rounding(dev, cin, cout, pixels):
    rng = np.random.default_rng(cin + cout)
    x = rng.standard_normal((pixels, cin)).astype(np.float32)
    dy = rng.standard_normal((pixels, cout)).astype(np.float32)
    w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    wt = href.pack_wt(w)
    res = [('forward', dev_forward(dev, _padded(x, cin + 1), wt, cin, cout), x @ w.T, href.forward64(x, w)),
           ('dgrad', dev_dgrad(dev, _padded(dy, cout + 1), wt, cin, cout), dy @ w, dy.astype(np.float64) @ w.astype(np.float64)),
           ('wgrad', _wgrad_both_fills(dev, _padded(x, cin + 1), _padded(dy, cout + 1), cin, cout, 0, 'rounding')[:, :cin], dy.T @ x,
            href.wgrad64(x, dy))]
    bad = []
    for name, got, r32, r64 in res:
        assert r32.dtype == np.float32
        e_dev, e_ref = href.rel_err(got, r64), href.rel_err(r32, r64)
        print('linear_wide %s %d->%d P=%d: device %.3e, NumPy float32 %.3e, bar %.3e' % (name, cin, cout, pixels, e_dev, e_ref, 4 * e_ref + EPS24))
        if not e_dev <= 4 * e_ref + EPS24:
            bad.append(name)
    assert not bad


@pytest.mark.parametrize('cin,cout', ref.ROUNDING_SHAPES)
def test_rounding(dev, cin, cout):
    """Measured on an MI355X, P = 333 standard-normal rows (device, E_ref, bar):
    424 -> 256   forward 7.777e-07, 7.777e-07, 3.171e-06;  dgrad 5.363e-07, 5.363e-07, 2.205e-06;  wgrad 4.222e-07, 7.632e-07, 3.112e-06
    1021 -> 513  forward 1.416e-06, 7.540e-07, 3.075e-06;  dgrad 7.617e-07, 4.841e-07, 1.996e-06;  wgrad 7.964e-07, 7.964e-07, 3.245e-06
    (the closest to its bar: the forward over 1021 channels, one sequential chain per element, 0.46 of it)."""
    _rounding(dev, cin, cout, ref.ROUNDING_PIXELS)


@pytest.mark.parametrize('cin,cout', ref.NARROW_SHAPES)
def test_narrow_widths_rounding(dev, cin, cout):
    """The narrow widths through the wide entries (their exact cases are in test_exact_integers).
    Measured on an MI355X, P = 333 (device, E_ref, bar):
    75 -> 75     forward 3.176e-07, 3.176e-07, 1.330e-06;  dgrad 3.105e-07, 3.105e-07, 1.301e-06;  wgrad 1.993e-07, 5.928e-07, 2.431e-06
    248 -> 128   forward 6.266e-07, 6.266e-07, 2.566e-06;  dgrad 4.717e-07, 4.717e-07, 1.946e-06;  wgrad 2.901e-07, 5.811e-07, 2.384e-06
    (the weight gradient at these widths is the narrow entry's)"""
    _rounding(dev, cin, cout, ref.ROUNDING_PIXELS)


def test_narrow_widths_give_the_narrow_entries_bytes(dev):
    """The forward and the input gradient add in the narrow entries' order (csrc/linearwide.hip's header), and the weight gradient of a
    shape that is narrow on both sides IS the narrow entry's: the same bytes in all three, the same chunk and workspace."""
    rt = _rt()
    for cin, cout in ref.NARROW_SHAPES:
        g = torch.Generator(device='cpu')
        g.manual_seed(cin)
        x = torch.randn((130, cin), generator=g).to(dev)
        dy = torch.randn((130, cout), generator=g).to(dev)
        wt = torch.from_numpy(href.pack_wt(np.random.default_rng(cout).standard_normal((cout, cin)))).to(dev)
        assert torch.equal(rt.linear_wide_forward(x, wt).view(torch.int32), rt.linear_forward(x, wt).view(torch.int32))
        assert torch.equal(rt.linear_wide_dgrad(dy, wt, cin).view(torch.int32), rt.linear_dgrad(dy, wt, cin).view(torch.int32))
        for pixels in (130, 1100):      # one chunk and several
            xs, ds = x.repeat(9, 1)[:pixels].contiguous(), dy.repeat(9, 1)[:pixels].contiguous()
            assert rt.linear_wide_wgrad_chunk(pixels, cin, cout) == rt.linear_wgrad_chunk(pixels, cin, cout)
            assert rt.linear_wide_wgrad_workspace_bytes(pixels, cin, cout) == rt.linear_wgrad_workspace_bytes(pixels, cin, cout)
            assert torch.equal(rt.linear_wide_wgrad(xs, ds).view(torch.int32), rt.linear_wgrad(xs, ds).view(torch.int32))


# ----------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(dev):
    rt = _rt()
    L = rt.lib()
    p, s = rt._ptr, rt.stream_ptr(dev)
    nan = float('nan')
    pixels, cin, cout, kp = 40, 301, 75, 304
    x = torch.zeros((pixels, cin), dtype=torch.float32, device=dev)
    dy = torch.zeros((pixels, cout), dtype=torch.float32, device=dev)
    wt = torch.zeros((cout, kp), dtype=torch.float32, device=dev)
    y = torch.full((pixels, cout), nan, dtype=torch.float32, device=dev)
    dx = torch.full((pixels, cin), nan, dtype=torch.float32, device=dev)
    dwt = torch.full((cout, kp), nan, dtype=torch.float32, device=dev)
    need = rt.linear_wide_wgrad_workspace_bytes(pixels, cin, cout)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)

    def off2(t):
        return ctypes.c_void_p(t.data_ptr() + 2)
    forward = [
        ('cin 0', 'cin 0', (p(x), cin, p(wt), pixels, 0, cout, p(y), cout, s)),
        ('cin 1025', 'cin 1025', (p(x), 1100, p(wt), pixels, 1025, cout, p(y), cout, s)),
        ('cout 0', 'cout 0', (p(x), cin, p(wt), pixels, cin, 0, p(y), cout, s)),
        ('cout 1025', 'cout 1025', (p(x), cin, p(wt), pixels, cin, 1025, p(y), 1100, s)),
        ('pixels 0', 'pixels 0', (p(x), cin, p(wt), 0, cin, cout, p(y), cout, s)),
        ('pixels 2^40', 'pixels %d' % (1 << 40), (p(x), cin, p(wt), 1 << 40, cin, cout, p(y), cout, s)),
        ('x_ld < cin', 'x_ld %d < cin %d' % (cin - 1, cin), (p(x), cin - 1, p(wt), pixels, cin, cout, p(y), cout, s)),
        ('y_ld < cout', 'y_ld %d < cout %d' % (cout - 1, cout), (p(x), cin, p(wt), pixels, cin, cout, p(y), cout - 1, s)),
        ('null x', 'null pointer', (None, cin, p(wt), pixels, cin, cout, p(y), cout, s)),
        ('null wt', 'null pointer', (p(x), cin, None, pixels, cin, cout, p(y), cout, s)),
        ('null y', 'null pointer', (p(x), cin, p(wt), pixels, cin, cout, None, cout, s)),
        ('y not 4-byte aligned', 'not 4-byte aligned', (p(x), cin, p(wt), pixels - 1, cin, cout, off2(y), cout, s)),
        ('x not 4-byte aligned', 'not 4-byte aligned', (off2(x), cin, p(wt), pixels - 1, cin, cout, p(y), cout, s)),
        ('wt not 4-byte aligned', 'not 4-byte aligned', (p(x), cin, off2(wt), pixels, cin, cout - 1, p(y), cout, s)),
        ('more than 2^37 pixels', 'more than 2^37 pixels', (p(x), cin, p(wt), 1 << 38, cin, cout, p(y), cout, s)),
        ('the last workgroup past 2^31', 'more than 2^37 pixels', (p(x), cin, p(wt), (1 << 37) - 63, cin, cout, p(y), cout, s)),
        ('byte offsets beyond 2^63', 'byte offsets beyond 2^63', (p(x), 1 << 22, p(wt), (1 << 40) - 1, cin, cout, p(y), cout, s)),
        ('byte offsets beyond 2^63 (y)', 'byte offsets beyond 2^63', (p(x), cin, p(wt), (1 << 40) - 1, cin, cout, p(y), 1 << 22, s)),
    ]
    dgrad = [
        ('cin 0', 'cin 0', (p(dy), cout, p(wt), pixels, 0, cout, p(dx), cin, s)),
        ('cin 1025', 'cin 1025', (p(dy), cout, p(wt), pixels, 1025, cout, p(dx), 1100, s)),
        ('cout 0', 'cout 0', (p(dy), cout, p(wt), pixels, cin, 0, p(dx), cin, s)),
        ('cout 1025', 'cout 1025', (p(dy), 1100, p(wt), pixels, cin, 1025, p(dx), cin, s)),
        ('pixels 0', 'pixels 0', (p(dy), cout, p(wt), 0, cin, cout, p(dx), cin, s)),
        ('pixels 2^40', 'pixels %d' % (1 << 40), (p(dy), cout, p(wt), 1 << 40, cin, cout, p(dx), cin, s)),
        ('dy_ld < cout', 'dy_ld %d < cout %d' % (cout - 1, cout), (p(dy), cout - 1, p(wt), pixels, cin, cout, p(dx), cin, s)),
        ('dx_ld < cin', 'dx_ld %d < cin %d' % (cin - 1, cin), (p(dy), cout, p(wt), pixels, cin, cout, p(dx), cin - 1, s)),
        ('null dy', 'null pointer', (None, cout, p(wt), pixels, cin, cout, p(dx), cin, s)),
        ('null wt', 'null pointer', (p(dy), cout, None, pixels, cin, cout, p(dx), cin, s)),
        ('null dx', 'null pointer', (p(dy), cout, p(wt), pixels, cin, cout, None, cin, s)),
        ('dx not 4-byte aligned', 'not 4-byte aligned', (p(dy), cout, p(wt), pixels - 1, cin, cout, off2(dx), cin, s)),
        ('dy not 4-byte aligned', 'not 4-byte aligned', (off2(dy), cout, p(wt), pixels - 1, cin, cout, p(dx), cin, s)),
        ('wt not 4-byte aligned', 'not 4-byte aligned', (p(dy), cout, off2(wt), pixels, cin, cout - 1, p(dx), cin, s)),
        ('more than 2^37 pixels', 'more than 2^37 pixels', (p(dy), cout, p(wt), 1 << 38, cin, cout, p(dx), cin, s)),
        ('byte offsets beyond 2^63', 'byte offsets beyond 2^63', (p(dy), 1 << 22, p(wt), (1 << 40) - 1, cin, cout, p(dx), cin, s)),
        ('byte offsets beyond 2^63 (dx)', 'byte offsets beyond 2^63', (p(dy), cout, p(wt), (1 << 40) - 1, cin, cout, p(dx), 1 << 22, s)),
    ]

    def wg(**kw):
        a = dict(x=p(x), x_ld=cin, dy=p(dy), dy_ld=cout, pixels=pixels, cin=cin, cout=cout, ws=p(ws), nbytes=need, dwt=p(dwt))
        a.update(kw)
        return tuple(a[k] for k in ('x', 'x_ld', 'dy', 'dy_ld', 'pixels', 'cin', 'cout', 'ws', 'nbytes', 'dwt')) + (s,)
    wgrad = [
        ('cin 0', 'cin 0', wg(cin=0)), ('cin 1025', 'cin 1025', wg(cin=1025, x_ld=1100)), ('cout 0', 'cout 0', wg(cout=0)),
        ('cout 1025', 'cout 1025', wg(cout=1025, dy_ld=1100)), ('pixels 0', 'pixels 0', wg(pixels=0)),
        ('pixels 2^40', 'pixels %d' % (1 << 40), wg(pixels=1 << 40)),
        ('x_ld < cin', 'x_ld %d < cin %d' % (cin - 1, cin), wg(x_ld=cin - 1)),
        ('dy_ld < cout', 'dy_ld %d < cout %d' % (cout - 1, cout), wg(dy_ld=cout - 1)),
        ('null x', 'null pointer', wg(x=None)), ('null dy', 'null pointer', wg(dy=None)), ('null workspace', 'null pointer', wg(ws=None)),
        ('null dwt', 'null pointer', wg(dwt=None)),
        ('dwt not 4-byte aligned', 'not 4-byte aligned', wg(dwt=off2(dwt))),
        ('x not 4-byte aligned', 'not 4-byte aligned', wg(x=off2(x), pixels=pixels - 1)),
        ('dy not 4-byte aligned', 'not 4-byte aligned', wg(dy=off2(dy), pixels=pixels - 1)),
        ('byte offsets beyond 2^63', 'byte offsets beyond 2^63', wg(pixels=(1 << 40) - 1, x_ld=1 << 22)),
        ('byte offsets beyond 2^63 (dy)', 'byte offsets beyond 2^63', wg(pixels=(1 << 40) - 1, dy_ld=1 << 22)),
        ('short workspace', 'of %d bytes, %d needed' % (need - 1, need), wg(nbytes=need - 1)),
        ('misaligned workspace', 'workspace not 16-byte aligned', wg(ws=ctypes.c_void_p(ws.data_ptr() + 4))),
    ]
    L.yr_last_error.restype = ctypes.c_char_p
    with torch.cuda.device(dev):
        for entry, who, cases in ((L.yr_linear_wide_forward, 'linear_wide_forward', forward), (L.yr_linear_wide_dgrad, 'linear_wide_dgrad', dgrad),
                                  (L.yr_linear_wide_wgrad, 'linear_wide_wgrad', wgrad)):
            for what, words, args in cases:
                assert entry(*args) == YR_ERR_ARG, who + ': ' + what
                msg = L.yr_last_error().decode()
                assert msg.startswith(who + ':') and words in msg, (who, what, msg)
    torch.cuda.synchronize()
    for t in (y, dx, dwt):
        assert np.all(_bits(t.cpu().numpy()) == NAN_BITS)
    assert bool((ws == 0xFF).all()) and not bool(x.any()) and not bool(dy.any()) and not bool(wt.any())
    # the binding's own checks
    with pytest.raises(ValueError):
        rt.linear_wide_forward(x, wt[:, :301].contiguous())
    with pytest.raises(ValueError):
        rt.linear_wide_forward(torch.zeros((4, 1025), dtype=torch.float32, device=dev), torch.zeros((8, 1028), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        rt.linear_wide_forward(x, torch.zeros((1025, kp), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        rt.linear_wide_dgrad(dy, wt, 301, out=torch.empty((pixels, 302), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        rt.linear_wide_dgrad(dy, wt, 1025)
    with pytest.raises(ValueError):
        rt.linear_wide_wgrad(x, dy[:20])
    with pytest.raises(ValueError):
        rt.linear_wide_wgrad(x, dy, workspace=torch.empty(16, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        rt.linear_wide_forward(x.cpu(), wt)
