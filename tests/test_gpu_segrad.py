"""The squeeze-excite block on the device (yoloret_amd/csrc/segrad.hip behind yr_se_forward and yr_se_backward) against
tests/segrad_ref.py.

Every launch of a C entry runs between the guards of tests/fence.py, in CARRIERS as tests/test_gpu_bntrain.py builds them (`off` NaN
floats, the data, 63 NaN floats; off = 1 puts every base pointer 4 bytes past a 256-byte boundary), with outputs pre-filled with NaN,
maps of ld = C and ld = C + 5 floats a pixel whose pad columns are NaN and must keep their bits, and the workspace pre-filled with 0xFF
(or random bytes, which must give the same bytes).  The two alignments and the two row forms alternate with the case number.

* integers: the sums over the pixels are exact in any order, so m equals plain NumPy bit for bit, and so does db2, which shows dg:
  db2 = sum_b dg[b] * (g[b] * (1 - g[b])) with the exact dg and the device's own g;
* arbitrary data: every output equals the float32 restatement in the device's documented order bit for bit, and
  max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the same figure of that restatement; the figures are printed before
  they assert (run with -s).

Measured on an MI355X over the 1275 figures of the file: the device equals the restatement bit for bit in every output of every case, so
device = E_ref in every figure: median 1.3e-07, 22 of them above 1e-06, all in C = 1 cases whose batch sums nearly cancel (the largest:
dw2 at B 3, 1 x 1, C 1, R 4, 2.3e-04 for device and restatement alike, bar 9.0e-04).  At the model's widths: 13 x 13 x 512 R 128
9.6e-08 to 2.0e-07 against bars of 4.4e-07 to 8.4e-07;  13 x 13 x 672 R 28  1.3e-07 to 3.0e-07 against 5.8e-07 to 1.2e-06."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import segrad_ref as ref
from tests.test_gpu_bntrain import _bits, _nan
from tests.test_gpu_fusegrad import _layout, _same_bits, fenced

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
YR_ERR_ARG = -1
NAN_BITS = np.float32(np.nan).view(np.uint32)
F32 = np.float32

SE_SHAPES = [(1, 1), (2, 3), (7, 5), (13, 13)]
SE_CHANNELS = [1, 3, 32, 75, 130]
SE_REDUCED = [1, 4, 33]
SE_BATCHES = [1, 3]
SE_MIN_ELEMS, SE_MAX_CHUNKS = 4096, 16          # of csrc/segrad.hip (tests/test_segrad_host.py reads them there)
WORKLOAD_LIKE = (2, 33, 33, 128, 32)            # 64 x 52 x 52 x 128, R 32, scaled down until the slab cap sets the chunk: 1089 > 16 * 64
MODEL_WIDTHS = [(2, 13, 13, 512, 128), (2, 13, 13, 672, 28)]
FWD_KEYS, BWD_KEYS = ('y', 'm', 'z1', 'g'), ('dx', 'dw1', 'db1', 'dw2', 'db2')


def se_min_chunk(c):
    return -(-SE_MIN_ELEMS // ref.cb_of(c))


def se_pixels(c):
    chunk = se_min_chunk(c)
    return [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]


def _rt():
    from yoloret_amd import runtime
    return runtime


# ----------------------------------------------------------------------------- the entries, fenced
def dev_forward(dev, x, w1, b1, w2, b2, ld, off=0, ws_fill=0xFF):
    """x [B, H, W, C] dense -> {y [B, H, W, C] (taken out of rows of ld floats whose pad columns were checked), m, z1, g}"""
    rt = _rt()
    b, h, w, c = x.shape
    r = w1.shape[1]
    need = rt.se_workspace_bytes(b, h * w, c, r)
    assert need > 0

    def launch(rd, wr, ws):
        rt.check(rt.lib().yr_se_forward(rd[0], ld, rd[1], rd[2], rd[3], rd[4], b, h, w, c, r, wr[0], ld, wr[1], wr[2], wr[3], ws, need,
                                        rt.stream_ptr(dev)))
    outs = fenced(dev, off, launch, [ref.padded(x, ld), w1, b1, w2, b2], [_nan(b, h, w, ld), _nan(b, c), _nan(b, r), _nan(b, c)], [c, c, r, c], need, ws_fill)
    return {'y': outs[0][..., :c], 'm': outs[1], 'z1': outs[2], 'g': outs[3]}


def dev_backward(dev, dy, x, w1, w2, m, z1, g, ld, off=0, need_dx=True, need_params=True, ws_fill=0xFF):
    """-> {dx, dw1, db1, dw2, db2}, None where not asked for"""
    rt = _rt()
    b, h, w, c = x.shape
    r = w1.shape[1]
    need = rt.se_workspace_bytes(b, h * w, c, r)
    assert need > 0
    writes = ([_nan(b, h, w, ld)] if need_dx else []) + ([_nan(c, r), _nan(r), _nan(r, c), _nan(c)] if need_params else [])
    cols = ([c] if need_dx else []) + ([r, r, c, c] if need_params else [])

    def launch(rd, wr, ws):
        wr = list(wr)
        dx = wr.pop(0) if need_dx else None
        par = wr if need_params else [None] * 4
        rt.check(rt.lib().yr_se_backward(rd[0], ld, rd[1], ld, rd[2], rd[3], rd[4], rd[5], rd[6], b, h, w, c, r, dx, ld, par[0], par[1], par[2], par[3],
                                         ws, need, rt.stream_ptr(dev)))
    outs = list(fenced(dev, off, launch, [ref.padded(dy, ld), ref.padded(x, ld), w1, w2, m, z1, g], writes, cols, need, ws_fill))
    out = dict.fromkeys(BWD_KEYS)
    if need_dx:
        out['dx'] = outs.pop(0)[..., :c]
    if need_params:
        out.update(zip(BWD_KEYS[1:], outs))
    return out


# ----------------------------------------------------------------------------- one case
def _check(dev, b, h, w, c, r, n, bad, random_workspace=False):
    """integers, then arbitrary data; appends (what, device, E_ref) for every figure over its bar"""
    rt = _rt()
    chunk = rt.se_chunk(b, h * w, c)
    off, ld = _layout(n, c)
    what = 'B=%d %dx%d C=%d R=%d ld=%d off=%d chunk=%d' % (b, h, w, c, r, ld, off, chunk)
    # integers: the sums over the pixels are exact in any order
    x, dy, w1, b1, w2, b2 = ref.se_case(b, h, w, c, r, exact=True)
    s_exact = x.astype(np.float64).sum(axis=(1, 2))
    dg_exact = (dy.astype(np.float64) * x.astype(np.float64)).sum(axis=(1, 2))
    assert np.abs(x).astype(np.float64).sum(axis=(1, 2)).max() < 2 ** 24 and np.abs(dy.astype(np.float64) * x).sum(axis=(1, 2)).max() < 2 ** 24
    f = dev_forward(dev, x, w1, b1, w2, b2, ld, off)
    _same_bits(f['m'], s_exact.astype(F32) / F32(h * w), 'm, integers ' + what)
    g = dev_backward(dev, dy, x, w1, w2, f['m'], f['z1'], f['g'], ld, off)
    dz2 = dg_exact.astype(F32) * (f['g'] * (F32(1) - f['g']))
    _same_bits(g['db2'], ref.batch_sum32(dz2), 'db2 (dg), integers ' + what)
    # arbitrary data: the device's order bit for bit, and the bar against float64
    x, dy, w1, b1, w2, b2 = ref.se_case(b, h, w, c, r)
    f = dev_forward(dev, x, w1, b1, w2, b2, ld, off)
    f32, f64 = ref.forward32(x, w1, b1, w2, b2, chunk), ref.forward64(x, w1, b1, w2, b2)
    for k in FWD_KEYS:
        _same_bits(f[k], f32[k], '%s in the device\'s order %s' % (k, what))
    g = dev_backward(dev, dy, x, w1, w2, f['m'], f['z1'], f['g'], ld, off)
    g32 = ref.backward32(dy, x, w1, w2, f32['m'], f32['z1'], f32['g'], chunk)
    g64 = ref.backward64(dy, x, w1, w2, f64['m'], f64['z1'], f64['g'])
    for k in BWD_KEYS:
        _same_bits(g[k], g32[k], '%s in the device\'s order %s' % (k, what))
    for k, got, r32, r64 in [(k, f[k], f32[k], f64[k]) for k in FWD_KEYS] + [(k, g[k], g32[k], g64[k]) for k in BWD_KEYS]:
        e_dev, e_ref = ref.rel_err(got, r64), ref.rel_err(r32, r64)
        print('se %s %s: device %.3e, float32 restatement %.3e, bar %.3e' % (k, what, e_dev, e_ref, 4 * e_ref + EPS24))
        if not e_dev <= 4 * e_ref + EPS24:
            bad.append((k, what, e_dev, e_ref))
    if random_workspace:
        f2 = dev_forward(dev, x, w1, b1, w2, b2, ld, off, ws_fill='random')
        g2 = dev_backward(dev, dy, x, w1, w2, f['m'], f['z1'], f['g'], ld, off, ws_fill='random')
        for k in FWD_KEYS:
            _same_bits(f2[k], f[k], '%s from a random workspace %s' % (k, what))
        for k in BWD_KEYS:
            _same_bits(g2[k], g[k], '%s from a random workspace %s' % (k, what))
    return f, g


@pytest.mark.parametrize('c', SE_CHANNELS)
def test_shapes(dev, c):
    """Every (H, W) x R x B of the lists at C = c (the figures measured on an MI355X are in the module text)."""
    bad = []
    for n, ((h, w), r, b) in enumerate(itertools.product(SE_SHAPES, SE_REDUCED, SE_BATCHES)):
        _check(dev, b, h, w, c, r, n, bad)
    assert not bad, bad


@pytest.mark.parametrize('c', SE_CHANNELS)
def test_at_the_chunk_edges(dev, c):
    """chunk - 1, chunk, chunk + 1 and 2 chunk + 1 pixels an image around the minimum chunk of C = c: one range, exactly one full range,
    two, three with a last range of one pixel; the random workspace gives the bytes of the 0xFF one."""
    bad = []
    for n, pixels in enumerate(se_pixels(c)):
        _check(dev, 2, 1, pixels, c, 4, n, bad, random_workspace=True)
    assert not bad, bad


def test_where_the_slab_cap_sets_the_chunk(dev):
    bad = []
    _check(dev, *WORKLOAD_LIKE, 1, bad, random_workspace=True)
    assert not bad, bad


@pytest.mark.parametrize('shape', MODEL_WIDTHS, ids=['%dx%dx%d-R%d' % s[1:] for s in MODEL_WIDTHS])
def test_model_widths(dev, shape):
    """The 13 x 13 heads (C 512, R 128) and EfficientNet-B0's stage 6 (C 672, R 28) at two images."""
    bad = []
    _check(dev, *shape, 0, bad)
    assert not bad, bad


def test_optional_outputs_keep_their_bits(dev):
    """with dx null the four parameter gradients keep their bits, with the parameters null dx keeps its bits; with both null nothing is
    written; the bindings give what the fenced calls gave"""
    rt = _rt()
    for n, (b, h, w, c, r) in enumerate([(3, 7, 5, 75, 33), (2, 1, 2 * se_min_chunk(130) + 1, 130, 4)]):
        x, dy, w1, b1, w2, b2 = ref.se_case(b, h, w, c, r, seed=1)
        off, ld = _layout(n + 1, c)
        f = dev_forward(dev, x, w1, b1, w2, b2, ld, off)
        full = dev_backward(dev, dy, x, w1, w2, f['m'], f['z1'], f['g'], ld, off)
        assert all(np.isfinite(full[k]).all() for k in BWD_KEYS)
        only_params = dev_backward(dev, dy, x, w1, w2, f['m'], f['z1'], f['g'], ld, off, need_dx=False)
        only_dx = dev_backward(dev, dy, x, w1, w2, f['m'], f['z1'], f['g'], ld, off, need_params=False)
        assert only_params['dx'] is None and all(only_dx[k] is None for k in BWD_KEYS[1:])
        for k in BWD_KEYS[1:]:
            _same_bits(only_params[k], full[k], '%s with dx null' % k)
        _same_bits(only_dx['dx'], full['dx'], 'dx with the parameters null')
        neither = dev_backward(dev, dy, x, w1, w2, f['m'], f['z1'], f['g'], ld, off, need_dx=False, need_params=False)
        assert all(v is None for v in neither.values())
        # the bindings
        t = [torch.from_numpy(a).to(dev) for a in (x, w1, b1, w2, b2, dy)]
        ws = torch.empty((rt.se_workspace_bytes(b, h * w, c, r) + 64,), dtype=torch.uint8, device=dev).random_(0, 256)
        y, m, z1, g = rt.se_forward(*t[:5], workspace=ws)
        for k, v in zip(FWD_KEYS, (y, m, z1, g)):
            _same_bits(v.cpu().numpy(), f[k], 'binding ' + k)
        got = rt.se_backward(t[5], t[0], t[1], t[3], m, z1, g, workspace=ws)
        for k, v in zip(BWD_KEYS, got):
            _same_bits(v.cpu().numpy(), full[k], 'binding ' + k)
        got = rt.se_backward(t[5], t[0], t[1], t[3], m, z1, g, need_dx=False)
        assert got[0] is None
        _same_bits(got[3].cpu().numpy(), full['dw2'], 'binding dw2 alone')
        got = rt.se_backward(t[5], t[0], t[1], t[3], m, z1, g, need_params=False)
        assert got[1:] == (None,) * 4
        _same_bits(got[0].cpu().numpy(), full['dx'], 'binding dx alone')


def test_an_image_alone_equals_its_slice_of_the_batch(dev):
    """the chunk does not depend on B: y, m, z1, g and dx of image 1 alone are the bits of its slice"""
    b, h, w, c, r = 3, 1, 2 * se_min_chunk(75) + 1, 75, 33
    x, dy, w1, b1, w2, b2 = ref.se_case(b, h, w, c, r, seed=2)
    f = dev_forward(dev, x, w1, b1, w2, b2, c)
    g = dev_backward(dev, dy, x, w1, w2, f['m'], f['z1'], f['g'], c, need_params=False)
    f1 = dev_forward(dev, x[1:2], w1, b1, w2, b2, c)
    g1 = dev_backward(dev, dy[1:2], x[1:2], w1, w2, f1['m'], f1['z1'], f1['g'], c, need_params=False)
    for k in FWD_KEYS:
        _same_bits(f1[k], f[k][1:2], k)
    _same_bits(g1['dx'], g['dx'][1:2], 'dx')


def test_refusals_change_nothing(dev):
    rt = _rt()
    L = rt.lib()
    p, s = rt._ptr, rt.stream_ptr(dev)
    nan = float('nan')
    b, h, w, c, r = 2, 6, 8, 8, 2
    n = h * w
    mp = torch.zeros((b, h, w, c), dtype=torch.float32, device=dev)
    par = {k: torch.ones(shape, dtype=torch.float32, device=dev) for k, shape in (('w1', (c, r)), ('b1', (r,)), ('w2', (r, c)), ('b2', (c,)), ('m', (b, c)),
                                                                                 ('z1', (b, r)), ('g', (b, c)))}
    o = {k: torch.full(shape, nan, dtype=torch.float32, device=dev)
         for k, shape in (('map', (b, h, w, c)), ('m', (b, c)), ('z1', (b, r)), ('g', (b, c)), ('dw1', (c, r)), ('db1', (r,)), ('dw2', (r, c)), ('db2', (c,)))}
    need = rt.se_workspace_bytes(b, n, c, r)
    assert need == 4 * (b * c + 2 * b * c + 2 * b * r) and rt.se_chunk(b, n, c) == 512
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)

    def order(g, keys, kw):
        g.update(kw)
        return tuple(g[k] for k in keys) + (s,)

    def fwd(**kw):
        g = dict(x=p(mp), x_ld=c, w1=p(par['w1']), b1=p(par['b1']), w2=p(par['w2']), b2=p(par['b2']), B=b, H=h, W=w, C=c, R=r, y=p(o['map']), y_ld=c,
                 m=p(o['m']), z1=p(o['z1']), g=p(o['g']), ws=p(ws), ws_bytes=need)
        return order(g, ('x', 'x_ld', 'w1', 'b1', 'w2', 'b2', 'B', 'H', 'W', 'C', 'R', 'y', 'y_ld', 'm', 'z1', 'g', 'ws', 'ws_bytes'), kw)

    def bwd(**kw):
        g = dict(dy=p(mp), dy_ld=c, x=p(mp), x_ld=c, w1=p(par['w1']), w2=p(par['w2']), m=p(par['m']), z1=p(par['z1']), g=p(par['g']), B=b, H=h, W=w, C=c, R=r,
                 dx=p(o['map']), dx_ld=c, dw1=p(o['dw1']), db1=p(o['db1']), dw2=p(o['dw2']), db2=p(o['db2']), ws=p(ws), ws_bytes=need)
        return order(g, ('dy', 'dy_ld', 'x', 'x_ld', 'w1', 'w2', 'm', 'z1', 'g', 'B', 'H', 'W', 'C', 'R', 'dx', 'dx_ld', 'dw1', 'db1', 'dw2', 'db2', 'ws',
                         'ws_bytes'), kw)
    odd = ctypes.c_void_p(o['map'].data_ptr() + 2)
    misaligned = ctypes.c_void_p(ws.data_ptr() + 4)
    huge = dict(B=1 << 19, H=1 << 10, W=1 << 10)          # 2^39 pixels: rows of 2^30 floats put byte offsets beyond 2^63
    cases = [
        (L.yr_se_forward, [('B 0', fwd(B=0)), ('H 0', fwd(H=0)), ('W -1', fwd(W=-1)), ('C 0', fwd(C=0)), ('C 4097', fwd(C=4097)), ('R 0', fwd(R=0)),
                           ('R 1025', fwd(R=1025)), ('x_ld < C', fwd(x_ld=c - 1)), ('y_ld < C', fwd(y_ld=c - 1)), ('null x', fwd(x=None)), ('null w1', fwd(w1=None)),
                           ('null b1', fwd(b1=None)), ('null w2', fwd(w2=None)), ('null b2', fwd(b2=None)), ('null y', fwd(y=None)), ('null m', fwd(m=None)),
                           ('null z1', fwd(z1=None)), ('null g', fwd(g=None)), ('y not 4-byte aligned', fwd(y=odd)), ('null workspace', fwd(ws=None)),
                           ('short workspace', fwd(ws_bytes=need - 1)), ('misaligned workspace', fwd(ws=misaligned)),
                           ('2^40 pixels', fwd(B=1 << 20, H=1 << 10, W=1 << 10)), ('row offsets', fwd(x_ld=1 << 30, y_ld=1 << 30, ws_bytes=1 << 62, **huge))]),
        (L.yr_se_backward, [('B 0', bwd(B=0)), ('H 0', bwd(H=0)), ('W 0', bwd(W=0)), ('C 0', bwd(C=0)), ('C 4097', bwd(C=4097)), ('R 0', bwd(R=0)), ('R 1025', bwd(R=1025)),
                            ('dy_ld < C', bwd(dy_ld=c - 1)), ('x_ld < C', bwd(x_ld=c - 1)), ('dx_ld < C', bwd(dx_ld=c - 1)), ('null dy', bwd(dy=None)),
                            ('null x', bwd(x=None)), ('null w1', bwd(w1=None)), ('null w2', bwd(w2=None)), ('null m', bwd(m=None)), ('null z1', bwd(z1=None)),
                            ('null g', bwd(g=None)), ('dw1 alone null', bwd(dw1=None)), ('db2 alone null', bwd(db2=None)),
                            ('db1 alone given', bwd(dw1=None, dw2=None, db2=None)), ('dx not 4-byte aligned', bwd(dx=odd)), ('null workspace', bwd(ws=None)),
                            ('short workspace', bwd(ws_bytes=need - 1)), ('misaligned workspace', bwd(ws=misaligned)),
                            ('row offsets', bwd(dy_ld=1 << 30, ws_bytes=1 << 62, **huge))]),
    ]
    with torch.cuda.device(dev):
        for entry, rows in cases:
            for what, args in rows:
                assert entry(*args) == YR_ERR_ARG, '%s: %s' % (entry.__name__, what)
                assert L.yr_last_error()
        assert L.yr_se_backward(*bwd(dx=None, dw1=None, db1=None, dw2=None, db2=None)) == 0, 'nothing asked for: nothing launched, no error'
    torch.cuda.synchronize()
    for t in o.values():
        assert np.all(_bits(t.cpu().numpy()) == NAN_BITS)
    assert bool((ws == 0xFF).all()) and not bool(mp.any()) and all(bool((t == 1).all()) for t in par.values())
    for bad in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, 0, 2), (1, 8, 4097, 2), (1 << 20, 1 << 20, 8, 2), (1, 1 << 40, 8, 2), (-1, 8, 8, 2)):
        assert rt.se_chunk(*bad[:3]) == 0 and rt.se_workspace_bytes(*bad) == 0, bad
    assert rt.se_workspace_bytes(1, 8, 8, 0) == 0 and rt.se_workspace_bytes(1, 8, 8, 1025) == 0
    # the binding's own checks
    w1, b1, w2, b2, m, z1, g = (par[k] for k in ('w1', 'b1', 'w2', 'b2', 'm', 'z1', 'g'))
    for call in (lambda: rt.se_forward(mp.cpu(), w1, b1, w2, b2), lambda: rt.se_forward(mp[0], w1, b1, w2, b2), lambda: rt.se_forward(mp, w2, b1, w2, b2),
                 lambda: rt.se_forward(mp, w1, b2, w2, b2), lambda: rt.se_forward(mp, w1, b1, w2, b1), lambda: rt.se_forward(mp, w1, b1, w1, b2),
                 lambda: rt.se_forward(mp, w1, b1, w2, b2, out=torch.empty_like(mp[:, :1])),
                 lambda: rt.se_forward(mp, w1, b1, w2, b2, workspace=torch.empty(8, dtype=torch.uint8, device=dev)),
                 lambda: rt.se_backward(mp[:, :1].contiguous(), mp, w1, w2, m, z1, g), lambda: rt.se_backward(mp, mp, w1, w2, z1, z1, g),
                 lambda: rt.se_backward(mp, mp, w1, w2, m, m, g), lambda: rt.se_backward(mp, mp, w1, w2, m, z1, z1),
                 lambda: rt.se_backward(mp, mp, w1, w2, m, z1, g, need_dx=False, out=torch.empty_like(mp))):
        with pytest.raises(ValueError):
            call()
