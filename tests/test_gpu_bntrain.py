"""BatchNorm in training mode on the device (yoloret_amd/csrc/bntrain.hip behind yr_bn_train_forward / yr_bn_train_backward) against
tests/bntrain_ref.py.

Every launch of a C entry runs between the guards of tests/fence.py, in CARRIERS as tests/test_gpu_convgrad.py builds them (`off` NaN
floats, the data, 63 NaN floats; off = 1 puts every base pointer 4 bytes past a 256-byte boundary), with outputs pre-filled with NaN,
rows of ld = C and ld = C + 5 floats whose pad columns are NaN and must keep their bits, and the workspace pre-filled with 0xFF.

Exact cases: data on which every per-channel sum is exact in float32 in any order, so the device must return the float32 restatement
(sequential sums) bit for bit.  Rounding cases: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24 with E_ref the same figure of
the float32 restatement; each prints its figures before it asserts (run with -s); the measured ones are in the docstrings."""
import ctypes

import numpy as np
import pytest
import torch

from tests import bntrain_ref as ref, fence

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
YR_ERR_ARG = -1
NAN_BITS = np.float32(np.nan).view(np.uint32)
ACT_ID = {None: 0, 'relu6': 1, 'swish': 2}
F32 = np.float32

BN_CHANNELS = [1, 3, 63, 64, 75, 130, 256]
BN_PIXELS = [1, 2, 63, 64, 65, 66, 258, 1030]
BN_EVEN_PIXELS = [p for p in BN_PIXELS if p % 2 == 0]
BN_CHUNK_CHANNELS = [3, 75]          # the chunk-edge cases: the flat form (C < 64) and two channel blocks
PAD = 5
# (gamma, beta) of the exact backward: xhat = -1 / +1 gives u = beta - gamma / beta + gamma
BWD_AFFINE = [(1.0, 1.0),        # u = 0 (masked: the tie) / 2
              (3.0, 3.0),        # 0 / 6: both ties
              (1.0, 5.0),        # 4 / 6 (masked: the tie)
              (0.5, 2.0),        # 1.5 / 2.5: inside
              (2.0, -3.0),       # -5 / -1: below
              (1.0, 8.0),        # 7 / 9: above
              (-1.5, 4.5),       # 6 (tie) / 3
              (0.25, 0.0)]       # -0.25 / 0.25


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


def fenced(dev, off, launch, reads, writes, cols, ws_bytes, ws_fill=0xFF):
    """launch(read pointers, write pointers, workspace pointer) between the guards.  reads: arrays; writes: the initial contents of the
    written tensors (NaN for pure outputs, values for tensors updated in place); cols: per written tensor the columns the entry may
    write (the rest of each row must stay NaN).  -> the written tensors after the call."""
    rt = _rt()
    cr = [_carrier(a, dev, off) for a in reads]
    cw = [_carrier(a, dev, off) for a in writes]
    ws = torch.full((ws_bytes,), ws_fill, dtype=torch.uint8, device=dev)

    def at(moved, c):
        return ctypes.c_void_p(moved(c).data_ptr() + 4 * off)

    def call(moved):
        launch([at(moved, c) for c, _ in cr], [at(moved, c) for c, _ in cw], rt._ptr(moved(ws)))
    with torch.cuda.device(dev):
        fence.run(call, writes=[c for c, _ in cw], reads=[c for c, _ in cr], scratch=[ws])
    outs = []
    for (c, n), init, ncol in zip(cw, writes, cols):
        o = _inner(c, n, off, np.shape(init))
        assert np.all(_bits(o[..., ncol:]) == NAN_BITS), 'pad columns of an output were written'
        outs.append(o)
    return outs


def _nan(*shape):
    return np.full(shape, np.nan, np.float32)


def dev_forward(dev, z, gamma, beta, c, eps, momentum, act, ld, off=0, moving=None, ws_fill=0xFF):
    """z [P, z_ld] (pad columns NaN) -> (a [P, ld], mean, invstd, moving_mean, moving_var); moving: (mean, var) initial values or None"""
    rt = _rt()
    pixels = z.shape[0]
    need = rt.bn_train_workspace_bytes(pixels, c)
    assert need > 0

    def launch(r, w, ws):
        mm, mv = (w[3], w[4]) if moving is not None else (None, None)
        rt.check(rt.lib().yr_bn_train_forward(r[0], z.shape[1], r[1], r[2], pixels, c, eps, momentum, ACT_ID[act], w[0], ld, w[1], w[2], mm, mv,
                                              ws, need, rt.stream_ptr(dev)))
    writes = [_nan(pixels, ld), _nan(c), _nan(c)] + ([np.array(moving[0], F32), np.array(moving[1], F32)] if moving is not None else [])
    outs = fenced(dev, off, launch, [z, gamma, beta], writes, [c] * len(writes), need, ws_fill)
    return tuple(outs) + ((None, None) if moving is None else ())


def dev_backward(dev, da, z, gamma, beta, mean, invstd, c, act, ld, off=0, need_dz=True, ws_fill=0xFF):
    """-> (dz [P, ld] or None, dgamma, dbeta)"""
    rt = _rt()
    pixels = z.shape[0]
    need = rt.bn_train_workspace_bytes(pixels, c)
    assert need > 0

    def launch(r, w, ws):
        rt.check(rt.lib().yr_bn_train_backward(r[0], da.shape[1], r[1], z.shape[1], r[2], r[3], r[4], r[5], pixels, c, ACT_ID[act],
                                               w[2] if need_dz else None, ld, w[0], w[1], ws, need, rt.stream_ptr(dev)))
    writes = [_nan(c), _nan(c)] + ([_nan(pixels, ld)] if need_dz else [])
    outs = fenced(dev, off, launch, [da, z, gamma, beta, mean, invstd], writes, [c] * len(writes), need, ws_fill)
    return (outs[2] if need_dz else None), outs[0], outs[1]


# ----------------------------------------------------------------------------- data
def exact_forward_case(pixels, c, seed=0):
    """z [P, C] of integers m_c + v: m_c in [-3, 3], the v randomly placed pairs +v / -v with v in [0, 4] (one 0 more for odd P), so the
    channel's sum is exactly m_c P in any order and the squared deviations are integers; channels with c % 3 == 2 are constant."""
    rng = np.random.default_rng(100000 * seed + 1000 * c + pixels)
    z = np.zeros((pixels, c), F32)
    m = rng.integers(-3, 4, c)
    for ch in range(c):
        v = rng.integers(0, 5, pixels // 2) if ch % 3 != 2 else np.zeros(pixels // 2, np.int64)
        col = np.concatenate([v, -v, np.zeros(pixels % 2, np.int64)])
        z[:, ch] = m[ch] + rng.permutation(col)
    gamma = rng.standard_normal(c).astype(F32)
    beta = rng.standard_normal(c).astype(F32)
    moving = (rng.standard_normal(c).astype(F32), rng.uniform(.5, 2, c).astype(F32))
    return z, m.astype(F32), gamma, beta, moving


def exact_backward_case(pixels, c, seed=0):
    """even P: z = m_c +- 2 in equal numbers (with eps = 0: var = 4, invstd = 1 / 2, xhat = -1 / +1), da integers in [-4, 4], gamma and
    beta from BWD_AFFINE, so u is exact and hits 0 and 6"""
    assert pixels % 2 == 0
    rng = np.random.default_rng(200000 * seed + 1000 * c + pixels)
    z = np.zeros((pixels, c), F32)
    m = rng.integers(-3, 4, c)
    for ch in range(c):
        z[:, ch] = m[ch] + rng.permutation(np.repeat([2, -2], pixels // 2))
    aff = np.array([BWD_AFFINE[ch % len(BWD_AFFINE)] for ch in range(c)], F32)
    da = ref.ints(rng, (pixels, c))
    return z, aff[:, 0].copy(), aff[:, 1].copy(), da


def rounding_case(pixels, c, seed=0):
    """z = offset_c + sigma_c * normal with |offset_c| up to 50 and sigma_c in [0.1, 2]; da standard normal"""
    rng = np.random.default_rng(300000 * seed + 1000 * c + pixels)
    offset = rng.uniform(-50, 50, c)
    if c > 1:
        offset[0], offset[1] = 50.0, -50.0
    sigma = rng.uniform(.1, 2, c)
    z = (offset[None, :] + sigma[None, :] * rng.standard_normal((pixels, c))).astype(F32)
    gamma = rng.uniform(.5, 1.5, c).astype(F32) * rng.choice([-1, 1], c).astype(F32)
    beta = (1 + rng.standard_normal(c)).astype(F32)
    da = rng.standard_normal((pixels, c)).astype(F32)
    return z, gamma, beta, da


def chunk_pixels(c):
    """pixel counts around the chunk the library reports for C = c: one slab, exactly one, two and three slabs"""
    rt = _rt()
    chunk = rt.bn_train_chunk(1, c)
    counts = [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    assert all(rt.bn_train_chunk(p, c) == chunk for p in counts)
    return chunk, counts


def _layout(n, c):
    """both alignments and dense / padded rows, alternating with the case number"""
    return n % 2, c + (n // 2) % 2 * PAD


# ----------------------------------------------------------------------------- exact
def _check_forward_exact(dev, pixels, c, n):
    z, m, gamma, beta, moving = exact_forward_case(pixels, c)
    for i, act in enumerate((None, 'relu6')):
        off, ld = _layout(n + i, c)
        momentum = (0.9, 0.5)[(n + i) % 2]
        want = ref.forward32(z, gamma, beta, 1e-3, momentum, act, *moving)
        assert np.array_equal(want['mean'], m), 'the generator: the mean is m exactly'
        a, mean, invstd, mm, mv = dev_forward(dev, ref.padded(z, ld), gamma, beta, c, 1e-3, momentum, act, ld, off, moving)
        what = 'P=%d C=%d act=%s ld=%d off=%d momentum=%g' % (pixels, c, act, ld, off, momentum)
        for name, got, w in (('mean', mean, want['mean']), ('invstd', invstd, want['invstd']), ('a', a[:, :c], want['a']),
                             ('moving_mean', mm, want['moving_mean']), ('moving_var', mv, want['moving_var'])):
            assert np.array_equal(_bits(got), _bits(w)), '%s %s' % (name, what)
        if pixels == 1 or c >= 3:
            const = np.arange(c) % 3 == 2 if pixels > 1 else np.ones(c, bool)
            assert np.array_equal(_bits(invstd[const]), _bits(np.full(int(const.sum()), F32(1) / np.sqrt(F32(1e-3)), F32))), 'var is +0 exactly'


@pytest.mark.parametrize('c', BN_CHANNELS)
def test_forward_exact_integers(dev, c):
    for n, pixels in enumerate(BN_PIXELS):
        _check_forward_exact(dev, pixels, c, n)


@pytest.mark.parametrize('c', BN_CHUNK_CHANNELS)
def test_forward_exact_at_the_chunk_edges(dev, c):
    for n, pixels in enumerate(chunk_pixels(c)[1]):
        _check_forward_exact(dev, pixels, c, n)


def _check_backward_exact(dev, pixels, c, n):
    z, gamma, beta, da = exact_backward_case(pixels, c)
    f = ref.forward32(z, gamma, beta, 0.0)
    assert np.all(f['var'] == 4) and np.all(f['invstd'] == 0.5) and np.all(np.abs(f['xhat']) == 1)
    for i, act in enumerate((None, 'relu6')):
        off, ld = _layout(n + i, c)
        want = ref.backward32(da, z, gamma, beta, f['mean'], f['invstd'], act)
        dz, dgamma, dbeta = dev_backward(dev, ref.padded(da, ld), ref.padded(z, ld), gamma, beta, f['mean'], f['invstd'], c, act, ld, off)
        what = 'P=%d C=%d act=%s ld=%d off=%d' % (pixels, c, act, ld, off)
        for name, got, w in (('dz', dz[:, :c], want[0]), ('dgamma', dgamma, want[1]), ('dbeta', dbeta, want[2])):
            assert np.array_equal(_bits(got), _bits(w)), '%s %s' % (name, what)


@pytest.mark.parametrize('c', BN_CHANNELS)
def test_backward_exact_even_counts(dev, c):
    for n, pixels in enumerate(BN_EVEN_PIXELS):
        _check_backward_exact(dev, pixels, c, n)


@pytest.mark.parametrize('c', BN_CHUNK_CHANNELS)
def test_backward_exact_at_the_chunk_edges(dev, c):
    for n, pixels in enumerate(p for p in chunk_pixels(c)[1] if p % 2 == 0):
        _check_backward_exact(dev, pixels, c, n)


def test_backward_relu6_passes_plus_zero_outside_the_open_interval(dev):
    """3 pixels x 5 channels, xhat = -1, 0, +1 exactly (the backward takes mean and invstd as given): u at 0 and 6 under a positive and a
    negative gamma, a channel wholly below 0 and one wholly above 6 (negative gamma).  g is +0 there, so the sums of those two channels
    are +0 to the bit, and everything equals the definition bit for bit."""
    z = np.array([[-2.0, 0.0, 2.0]], F32).T + np.array([1.0, -3.0, 0.0, 2.0, -1.0], F32)[None, :]
    mean, invstd = np.array([1.0, -3.0, 0.0, 2.0, -1.0], F32), np.full(5, 0.5, F32)
    gamma = np.array([3.0, -3.0, 1.0, -1.0, 0.5], F32)
    beta = np.array([3.0, 3.0, -3.0, 8.0, 2.0], F32)
    da = np.array([[1.0, -2.0, 3.0, -4.0, 2.0], [-1.0, 2.0, -3.0, 4.0, -2.0], [2.0, 3.0, -1.0, 1.0, -3.0]], F32)
    xhat, u = ref._xhat_u32(z, mean, invstd, gamma, beta)
    assert np.array_equal(u.T, np.array([[0, 3, 6], [6, 3, 0], [-4, -3, -2], [9, 8, 7], [1.5, 2, 2.5]], F32))
    outside = ~((u > 0) & (u < 6))
    assert np.all(_bits(ref.act_grad32(da, u, 'relu6'))[outside] == 0), 'the definition itself: +0 outside'
    want = ref.backward32(da, z, gamma, beta, mean, invstd, 'relu6')
    dz, dgamma, dbeta = dev_backward(dev, da, z, gamma, beta, mean, invstd, 5, 'relu6', 5)
    assert np.all(_bits(dbeta)[2:4] == 0) and np.all(_bits(dgamma)[2:4] == 0)
    for name, got, w in (('dz', dz, want[0]), ('dgamma', dgamma, want[1]), ('dbeta', dbeta, want[2])):
        assert np.array_equal(_bits(got), _bits(w)), name


def one_hot_da(pixels, c, where, rng):
    """da that is nonzero at one pixel per channel: each per-channel sum has one nonzero term, exact whatever xhat is"""
    da = np.zeros((pixels, c), F32)
    rows = {'first': np.zeros(c, np.int64), 'last': np.full(c, pixels - 1), 'random': rng.integers(0, pixels, c)}[where]
    da[rows, np.arange(c)] = rng.standard_normal(c).astype(F32)
    return da


@pytest.mark.parametrize('c', BN_CHANNELS)
def test_backward_exact_one_term_a_channel(dev, c):
    """any P, odd ones and P = 1 included, any z"""
    counts = BN_PIXELS + (chunk_pixels(c)[1] if c in BN_CHUNK_CHANNELS else [])
    for n, pixels in enumerate(counts):
        z, gamma, beta, _ = rounding_case(pixels, c)
        rng = np.random.default_rng(7 * pixels + c)
        f = ref.forward32(z, gamma, beta, 1e-3)
        where = ('first', 'last', 'random')[n % 3]
        act = (None, 'relu6')[(n // 3) % 2]
        da = one_hot_da(pixels, c, where, rng)
        off, ld = _layout(n, c)
        want = ref.backward32(da, z, gamma, beta, f['mean'], f['invstd'], act)
        dz, dgamma, dbeta = dev_backward(dev, ref.padded(da, ld), ref.padded(z, ld), gamma, beta, f['mean'], f['invstd'], c, act, ld, off)
        what = 'P=%d C=%d act=%s da at the %s pixel ld=%d off=%d' % (pixels, c, act, where, ld, off)
        for name, got, w in (('dz', dz[:, :c], want[0]), ('dgamma', dgamma, want[1]), ('dbeta', dbeta, want[2])):
            assert np.array_equal(_bits(got), _bits(w)), '%s %s' % (name, what)


# ----------------------------------------------------------------------------- rounding
ROUNDING_SHAPES = [(1030, 75), (258, 256), (66, 130), (65, 3), (2 * 2731 + 1, 3), (257, 64)]


def _var_of(invstd, eps):
    return 1.0 / np.asarray(invstd, np.float64) ** 2 - float(F32(eps))


@pytest.mark.parametrize('act', [None, 'relu6', 'swish'])
def test_rounding(dev, act):
    """z = offset + sigma * normal, |offset| up to 50 (what a sum-of-squares variance fails on), sigma in [0.1, 2]; da standard normal.
    Measured on an MI355X over the six shapes and three activations (every figure is printed, run with -s), device / E_ref ranges and the
    case that came closest to its bar:
    mean    7.07e-08 .. 2.39e-07 / 7.07e-08 .. 9.82e-07;  7.07e-08 against 3.42e-07 (P = 65, C = 3)
    var     9.37e-08 .. 2.31e-07 / 9.37e-08 .. 5.59e-07;  9.37e-08 against 4.34e-07 (P = 65, C = 3)
    a       5.05e-07 .. 4.53e-06 / 5.05e-07 .. 2.71e-05;  5.61e-07 against 2.30e-06 (swish, P = 65, C = 3)
    dz      1.85e-07 .. 7.37e-06 / 2.35e-07 .. 5.84e-05;  7.05e-07 against 2.88e-06 (swish, P = 65, C = 3)
    dgamma  1.47e-06 .. 3.89e-05 / 1.47e-06 .. 8.16e-05;  2.24e-06 against 9.01e-06 (relu6, P = 65, C = 3)
    dbeta   6.63e-08 .. 1.07e-05 / 1.61e-07 .. 3.32e-05;  5.01e-06 against 1.56e-05 (swish, P = 66, C = 130)
    The device was at or below E_ref in 107 of the 108 figures: its chunked sums are shorter than the sequential ones."""
    bad = []
    for pixels, c in ROUNDING_SHAPES:
        z, gamma, beta, da = rounding_case(pixels, c)
        eps = 1e-3
        r64 = ref.forward64(z, gamma, beta, eps, act)
        if act == 'relu6':
            assert min(np.abs(r64['u']).min(), np.abs(r64['u'] - 6).min()) > 1e-6, 'a kink of ReLU6 within 1e-6: choose another seed'
        assert np.abs(r64['u']).max() < 87.0
        dz64, dg64, db64 = ref.backward64(da, z, gamma, beta, eps, act)
        r32 = ref.forward32(z, gamma, beta, eps, 0.9, act)
        dz32, dg32, db32 = ref.backward32(da, z, gamma, beta, r32['mean'], r32['invstd'], act)
        a, mean, invstd, _, _ = dev_forward(dev, z, gamma, beta, c, eps, 0.9, act, c)
        dz, dgamma, dbeta = dev_backward(dev, da, z, gamma, beta, mean, invstd, c, act, c)
        for name, got, w32, w64 in (('mean', mean, r32['mean'], r64['mean']), ('var', _var_of(invstd, eps), _var_of(r32['invstd'], eps), r64['var']),
                                    ('a', a, r32['a'], r64['a']), ('dz', dz, dz32, dz64), ('dgamma', dgamma, dg32, dg64), ('dbeta', dbeta, db32, db64)):
            e_dev, e_ref = ref.rel_err(got, w64), ref.rel_err(w32, w64)
            print('bn_train %s P=%d C=%d %s: device %.3e, float32 restatement %.3e, bar %.3e' % (act, pixels, c, name, e_dev, e_ref, 4 * e_ref + EPS24))
            if not e_dev <= 4 * e_ref + EPS24:
                bad.append((pixels, c, name, e_dev, e_ref))
    assert not bad, bad


# ----------------------------------------------------------------------------- the same call, the same bytes; optional arguments
def test_same_call_same_bytes(dev):
    chunk, counts = chunk_pixels(75)
    pixels, c = counts[-1], 75
    z, gamma, beta, da = rounding_case(pixels, c, seed=1)
    moving = (np.zeros(c, F32), np.ones(c, F32))
    fw = [dev_forward(dev, z, gamma, beta, c, 1e-3, 0.9, 'swish', c, moving=moving, ws_fill=f) for f in (0xFF, 0x7B)]
    for x, y in zip(*fw):
        assert np.isfinite(x).all() and np.array_equal(_bits(x), _bits(y))
    a, mean, invstd = fw[0][:3]
    bw = [dev_backward(dev, da, z, gamma, beta, mean, invstd, c, 'swish', c, ws_fill=f) for f in (0xFF, 0x00)]
    for x, y in zip(*bw):
        assert np.isfinite(x).all() and np.array_equal(_bits(x), _bits(y))
    # dz == null: dgamma and dbeta are the same bits; no moving statistics: a, mean and invstd are the same bits
    none, dgamma, dbeta = dev_backward(dev, da, z, gamma, beta, mean, invstd, c, 'swish', c, need_dz=False)
    assert none is None and np.array_equal(_bits(dgamma), _bits(bw[0][1])) and np.array_equal(_bits(dbeta), _bits(bw[0][2]))
    plain = dev_forward(dev, z, gamma, beta, c, 1e-3, 0.9, 'swish', c)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(plain[:3], fw[0][:3]))
    # the binding gives what the fenced call gave
    rt = _rt()
    tz, tg, tb, tda = (torch.from_numpy(v).to(dev) for v in (z, gamma, beta, da))
    tm, tv = torch.from_numpy(moving[0]).to(dev), torch.from_numpy(moving[1]).to(dev)
    ws = torch.empty((rt.bn_train_workspace_bytes(pixels, c) + 64,), dtype=torch.uint8, device=dev).random_(0, 256)
    ta, tmean, tinv = rt.bn_train_forward(tz, tg, tb, 1e-3, 0.9, 'swish', tm, tv, workspace=ws)
    for got, want in ((ta, a), (tmean, mean), (tinv, invstd), (tm, fw[0][3]), (tv, fw[0][4])):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    tdz, tdg, tdb = rt.bn_train_backward(tda, tz, tg, tb, tmean, tinv, 'swish', workspace=ws)
    for got, want in ((tdz, bw[0][0]), (tdg, bw[0][1]), (tdb, bw[0][2])):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    n2, tdg2, tdb2 = rt.bn_train_backward(tda, tz, tg, tb, tmean, tinv, 'swish', need_dz=False)
    assert n2 is None and np.array_equal(_bits(tdg2.cpu().numpy()), _bits(bw[0][1])) and np.array_equal(_bits(tdb2.cpu().numpy()), _bits(bw[0][2]))


# ----------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(dev):
    rt = _rt()
    L = rt.lib()
    p, s = rt._ptr, rt.stream_ptr(dev)
    nan = float('nan')
    n, c = 40, 8
    z = torch.zeros((n, c), dtype=torch.float32, device=dev)
    vec = torch.zeros((c,), dtype=torch.float32, device=dev)
    outs = {k: torch.full((n, c) if k in ('a', 'dz') else (c,), nan, dtype=torch.float32, device=dev)
            for k in ('a', 'mean', 'invstd', 'mm', 'mv', 'dz', 'dgamma', 'dbeta')}
    need = rt.bn_train_workspace_bytes(n, c)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)
    o = outs

    def fwd(**kw):
        g = dict(z=p(z), z_ld=c, gamma=p(vec), beta=p(vec), pixels=n, C=c, eps=1e-3, momentum=0.9, act=1, a=p(o['a']), a_ld=c, mean=p(o['mean']),
                 invstd=p(o['invstd']), mm=p(o['mm']), mv=p(o['mv']), ws=p(ws), ws_bytes=need)
        g.update(kw)
        return tuple(g[k] for k in ('z', 'z_ld', 'gamma', 'beta', 'pixels', 'C', 'eps', 'momentum', 'act', 'a', 'a_ld', 'mean', 'invstd', 'mm', 'mv', 'ws',
                                    'ws_bytes')) + (s,)

    def bwd(**kw):
        g = dict(da=p(z), da_ld=c, z=p(z), z_ld=c, gamma=p(vec), beta=p(vec), mean=p(vec), invstd=p(vec), pixels=n, C=c, act=1, dz=p(o['dz']), dz_ld=c,
                 dgamma=p(o['dgamma']), dbeta=p(o['dbeta']), ws=p(ws), ws_bytes=need)
        g.update(kw)
        return tuple(g[k] for k in ('da', 'da_ld', 'z', 'z_ld', 'gamma', 'beta', 'mean', 'invstd', 'pixels', 'C', 'act', 'dz', 'dz_ld', 'dgamma', 'dbeta',
                                    'ws', 'ws_bytes')) + (s,)
    misaligned = ctypes.c_void_p(ws.data_ptr() + 4)
    forward = [('pixels 0', fwd(pixels=0)), ('pixels 2^40', fwd(pixels=1 << 40)), ('C 0', fwd(C=0)), ('z_ld < C', fwd(z_ld=c - 1)), ('a_ld < C', fwd(a_ld=c - 1)),
               ('act 3', fwd(act=3)), ('act -1', fwd(act=-1)), ('eps < 0', fwd(eps=-1e-3)), ('eps inf', fwd(eps=float('inf'))), ('eps nan', fwd(eps=nan)),
               ('momentum 1.5', fwd(momentum=1.5)), ('momentum < 0', fwd(momentum=-0.1)), ('momentum nan', fwd(momentum=nan)),
               ('only moving_mean', fwd(mv=None)), ('only moving_var', fwd(mm=None)), ('null z', fwd(z=None)), ('null gamma', fwd(gamma=None)),
               ('null beta', fwd(beta=None)), ('null a', fwd(a=None)), ('null mean', fwd(mean=None)), ('null invstd', fwd(invstd=None)),
               ('null workspace', fwd(ws=None)), ('short workspace', fwd(ws_bytes=need - 1)), ('misaligned workspace', fwd(ws=misaligned)),
               ('a not 4-byte aligned', fwd(a=ctypes.c_void_p(o['a'].data_ptr() + 2)))]
    backward = [('pixels 0', bwd(pixels=0)), ('pixels -1', bwd(pixels=-1)), ('C 0', bwd(C=0)), ('da_ld < C', bwd(da_ld=c - 1)), ('z_ld < C', bwd(z_ld=c - 1)),
                ('dz_ld < C', bwd(dz_ld=c - 1)), ('act 4', bwd(act=4)), ('null da', bwd(da=None)), ('null z', bwd(z=None)), ('null gamma', bwd(gamma=None)),
                ('null beta', bwd(beta=None)), ('null mean', bwd(mean=None)), ('null invstd', bwd(invstd=None)), ('null dgamma', bwd(dgamma=None)),
                ('null dbeta', bwd(dbeta=None)), ('null workspace', bwd(ws=None)), ('short workspace', bwd(ws_bytes=need - 1)),
                ('misaligned workspace', bwd(ws=misaligned))]
    with torch.cuda.device(dev):
        for entry, cases in ((L.yr_bn_train_forward, forward), (L.yr_bn_train_backward, backward)):
            for what, args in cases:
                assert entry(*args) == YR_ERR_ARG, what
                assert L.yr_last_error()
    torch.cuda.synchronize()
    for t in outs.values():
        assert np.all(_bits(t.cpu().numpy()) == NAN_BITS)
    assert bool((ws == 0xFF).all()) and not bool(z.any()) and not bool(vec.any())
    for bad in ((0, 8), (-1, 8), (1 << 40, 8), (40, 0), (40, -3)):
        assert rt.bn_train_chunk(*bad) == 0 and rt.bn_train_workspace_bytes(*bad) == 0
    # the binding's own checks
    with pytest.raises(ValueError):
        rt.bn_train_forward(z, vec, vec, act='sigmoid')
    with pytest.raises(ValueError):
        rt.bn_train_forward(z, vec, vec, moving_mean=vec)
    with pytest.raises(ValueError):
        rt.bn_train_forward(z, vec, vec, eps=-1.0)
    with pytest.raises(ValueError):
        rt.bn_train_forward(z, vec, vec, momentum=1.5)
    with pytest.raises(ValueError):
        rt.bn_train_forward(z, vec[:4].contiguous(), vec)
    with pytest.raises(ValueError):
        rt.bn_train_forward(z, vec, vec, workspace=torch.empty(16, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        rt.bn_train_forward(z.cpu(), vec, vec)
    with pytest.raises(ValueError):
        rt.bn_train_backward(z, z[:20].contiguous(), vec, vec, vec, vec, None)
    with pytest.raises(ValueError):
        rt.bn_train_backward(z, z, vec, vec, vec, vec, 'relu6', need_dz=False, out=torch.empty_like(z))
