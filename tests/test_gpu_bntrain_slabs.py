"""BatchNorm in training mode (yoloret_amd/csrc/bntrain.hip) at the slab counts and chunks training runs at: more than BT_TILE = 128 slabs,
so bt_slab_sum makes its second pass, up to the most (256); chunks that the `most` branch of bt_chunk sets, above the minimum and no
multiple of PP; the tile loader with a partial channel block and in the flat form (C < 64); bt_bwd_finish_kernel at those counts.  The
launchers, the fence and the generators are those of tests/test_gpu_bntrain.py; tests/test_bntrain_host.py asserts (without a GPU) that
SLAB_ROWS and ORDERED_SHAPES reach what they claim.

Exact cases as there: data whose per-channel sums are exact in float32 in any order, so the device must return the restatement with
sequential sums bit for bit.  Ordered cases: ARBITRARY data (the rounding generator) against the same restatement with its sums in the
order the header of bntrain.hip documents (bntrain_ref.ordered_sum), bit for bit - the bar of the rounding tests, 4 E_ref from a
sequential sum, sits 40x .. 180x above a correct kernel at these sizes."""
import functools

import numpy as np
import pytest
import torch

from tests import bntrain_ref as ref
from tests.test_gpu_bntrain import (EPS24, F32, ROUNDING_SHAPES, _bits, _check_forward_exact, _layout, _rt, _var_of, dev_backward, dev_forward,
                                    exact_backward_case, one_hot_da, rounding_case)

pytestmark = pytest.mark.gpu

# (pixels, C, chunk, slabs): the smallest shapes that reach each form
SLAB_ROWS = [(16385, 64, 128, 129),          # 0: the second tile holds one slab; the last range one pixel
             (18437, 75, 128, 145),          # 1: the second tile 17 slabs (one unrolled group of 16 and a tail); a second channel block of 11
             (32768, 64, 128, 256),          # 2: both tiles full, the last value of the minimum chunk
             (32769, 130, 129, 255),         # 3: a chunk above the minimum, no multiple of PP = 16; last range 3 pixels; a third block of 2 channels
             (349569, 3, 2731, 129),         # 4: the flat form (PP = 341), the tile loader with cb = 3
             (699137, 3, 2732, 256),         # 5: the flat form, a chunk above the minimum
             (1048577, 1, 8192, 129)]        # 6: C = 1, PP = 1024
SLAB_IDS = ['P%d-C%d' % r[:2] for r in SLAB_ROWS]
SAME_BYTES_ROWS = [SLAB_ROWS[3], SLAB_ROWS[5]]
WORKLOAD_LIKE = [(43264, 75), (173056, 24)]          # 64 x 26 x 26 pixels: chunk 169, 256 slabs; 64 x 52 x 52: chunk 676, PP = 42, 16 idle lanes
ORDERED_SHAPES = list(ROUNDING_SHAPES) + [SLAB_ROWS[i][:2] for i in (1, 3, 5)] + WORKLOAD_LIKE
ORDERED_IDS = ['P%d-C%d' % s for s in ORDERED_SHAPES]
AUTOGRAD_SHAPE = (5, 58, 57, 64)                     # 16530 pixels: 130 slabs of 128


def geometry(pixels, c):
    """(chunk, slabs, PP) as the library reports them"""
    rt = _rt()
    chunk = rt.bn_train_chunk(pixels, c)
    slabs = -(-pixels // chunk)
    assert rt.bn_train_workspace_bytes(pixels, c) == 2 * slabs * c * 4
    return chunk, slabs, 1024 // min(c, 64)


def next_even(pixels):
    return pixels + pixels % 2


def _equal(what, pairs):
    for name, got, want in pairs:
        bad = _bits(got) != _bits(want)
        assert not bad.any(), '%s %s: %d of %d elements differ, first at %s: got %r, want %r' % (
            name, what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), np.asarray(got)[bad][0], np.asarray(want)[bad][0])


# ----------------------------------------------------------------------------- exact
@pytest.mark.parametrize('row', SLAB_ROWS, ids=SLAB_IDS)
def test_forward_exact(dev, row):
    """act None and ReLU6, both momenta, the moving statistics: mean, invstd, a, moving_mean, moving_var bit for bit"""
    pixels, c, chunk, slabs = row
    assert geometry(pixels, c)[:2] == (chunk, slabs)
    _check_forward_exact(dev, pixels, c, SLAB_ROWS.index(row))


@pytest.mark.parametrize('row', SLAB_ROWS, ids=SLAB_IDS)
def test_backward_exact(dev, row):
    """at the next even P (the slab count is the same): dz, dgamma, dbeta bit for bit; with dz == null (bt_bwd_finish_kernel, a grid of
    its own) dgamma and dbeta have the same bits"""
    pixels, c, chunk, slabs = row
    pixels = next_even(pixels)
    assert geometry(pixels, c)[:2] == (chunk, slabs)
    z, gamma, beta, da = exact_backward_case(pixels, c)
    f = ref.forward32(z, gamma, beta, 0.0)
    assert np.all(f['var'] == 4) and np.all(f['invstd'] == 0.5) and np.all(np.abs(f['xhat']) == 1)
    for i, act in enumerate((None, 'relu6')):
        off, ld = _layout(SLAB_ROWS.index(row) + i, c)
        want = ref.backward32(da, z, gamma, beta, f['mean'], f['invstd'], act)
        zp, dap = ref.padded(z, ld), ref.padded(da, ld)
        dz, dgamma, dbeta = dev_backward(dev, dap, zp, gamma, beta, f['mean'], f['invstd'], c, act, ld, off)
        what = 'P=%d C=%d act=%s ld=%d off=%d' % (pixels, c, act, ld, off)
        _equal(what, (('dz', dz[:, :c], want[0]), ('dgamma', dgamma, want[1]), ('dbeta', dbeta, want[2])))
        none, dgamma2, dbeta2 = dev_backward(dev, dap, zp, gamma, beta, f['mean'], f['invstd'], c, act, ld, off, need_dz=False)
        assert none is None
        _equal(what + ' dz == null', (('dgamma', dgamma2, dgamma), ('dbeta', dbeta2, dbeta)))


@pytest.mark.parametrize('row', SLAB_ROWS, ids=SLAB_IDS)
def test_backward_exact_one_term_a_channel(dev, row):
    """the table's own P (odd but for one), any z: da at the first, the last and a random pixel of each channel"""
    pixels, c, chunk, slabs = row
    assert geometry(pixels, c)[:2] == (chunk, slabs)
    z, gamma, beta, _ = rounding_case(pixels, c)
    f = ref.forward32(z, gamma, beta, 1e-3)
    rng = np.random.default_rng(7 * pixels + c)
    for n, where in enumerate(('first', 'last', 'random')):
        act = (None, 'relu6')[(SLAB_ROWS.index(row) + n) % 2]
        da = one_hot_da(pixels, c, where, rng)
        off, ld = _layout(SLAB_ROWS.index(row) + n, c)
        want = ref.backward32(da, z, gamma, beta, f['mean'], f['invstd'], act)
        dz, dgamma, dbeta = dev_backward(dev, ref.padded(da, ld), ref.padded(z, ld), gamma, beta, f['mean'], f['invstd'], c, act, ld, off)
        what = 'P=%d C=%d act=%s da at the %s pixel ld=%d off=%d' % (pixels, c, act, where, ld, off)
        _equal(what, (('dz', dz[:, :c], want[0]), ('dgamma', dgamma, want[1]), ('dbeta', dbeta, want[2])))


# ----------------------------------------------------------------------------- the same call, the same bytes
@pytest.mark.parametrize('row', SAME_BYTES_ROWS, ids=['P%d-C%d' % r[:2] for r in SAME_BYTES_ROWS])
def test_same_call_same_bytes(dev, row):
    pixels, c, chunk, slabs = row
    assert geometry(pixels, c)[:2] == (chunk, slabs)
    z, gamma, beta, da = rounding_case(pixels, c, seed=1)
    moving = (np.zeros(c, F32), np.ones(c, F32))
    fw = [dev_forward(dev, z, gamma, beta, c, 1e-3, 0.9, 'swish', c, moving=moving, ws_fill=f) for f in (0xFF, 0x7B)]
    for x, y in zip(*fw):
        assert np.isfinite(x).all() and np.array_equal(_bits(x), _bits(y))
    mean, invstd = fw[0][1:3]
    bw = [dev_backward(dev, da, z, gamma, beta, mean, invstd, c, 'swish', c, ws_fill=f) for f in (0xFF, 0x00)]
    for x, y in zip(*bw):
        assert np.isfinite(x).all() and np.array_equal(_bits(x), _bits(y))


# ----------------------------------------------------------------------------- the device's order on arbitrary data
@functools.lru_cache(maxsize=1)
def _ordered_case(pixels, c):
    """the data of a shape, generated once for its three activations; nothing mutable leaves (the arrays are read-only)"""
    case = rounding_case(pixels, c)
    for a in case:
        a.setflags(write=False)
    return case


@pytest.mark.parametrize('act', [None, 'relu6', 'swish'])
@pytest.mark.parametrize('shape', ORDERED_SHAPES, ids=ORDERED_IDS)
def test_device_order_bit_for_bit(dev, shape, act):
    """z = offset + sigma * normal, da standard normal (rounding_case).  For act None and ReLU6 mean, invstd, a, dz, dgamma and dbeta must
    have the bits of the float32 restatement whose sums run in the device's documented order (the backward is fed the device's own mean and
    invstd).  For Swish only mean and invstd are compared bitwise (NumPy's exp is not the device's); a, dz, dgamma and dbeta keep the
    project's rule, max |device - ref64| / max |ref64| <= 4 E_ref + 2^-24 with E_ref the SEQUENTIAL restatement's.
    Measured on an MI355X (every figure is printed, run with -s): none and ReLU6, all 11 shapes: 0 elements of any of the six tensors
    differ.  Swish: mean and invstd 0 differ; about a tenth of a (470230 of 4259970 at 32769 x 130) and a sixth of dz differ in the last
    bits (the exp), and with them most of dgamma and dbeta.  Swish, device / sequential E_ref over the 11 shapes:
    a       5.61e-07 .. 9.19e-06 / 5.61e-07 .. 2.51e-04;  dz      7.05e-07 .. 3.22e-05 / 7.05e-07 .. 3.76e-04
    dgamma  1.60e-06 .. 3.19e-05 / 1.99e-06 .. 5.97e-04;  dbeta   6.76e-07 .. 1.07e-05 / 6.76e-07 .. 1.36e-04
    closest to its bar: dbeta at 66 x 130, 5.01e-06 against 1.56e-05; at 699137 x 3 the bar of dgamma (2.39e-03) is 534 x the device's
    4.47e-06 - which is why the other two activations are held to the bits."""
    pixels, c = shape
    chunk, slabs, pp = geometry(pixels, c)
    sums = ref.device_order(c, chunk)
    z, gamma, beta, da = _ordered_case(pixels, c)
    eps = 1e-3
    want = ref.forward32(z, gamma, beta, eps, 0.9, act, sums=sums)
    a, mean, invstd, _, _ = dev_forward(dev, z, gamma, beta, c, eps, 0.9, act, c)
    dz, dgamma, dbeta = dev_backward(dev, da, z, gamma, beta, mean, invstd, c, act, c)
    wdz, wdg, wdb = ref.backward32(da, z, gamma, beta, mean, invstd, act, sums=sums)
    what = 'P=%d C=%d act=%s chunk %d, %d slabs, PP %d' % (pixels, c, act, chunk, slabs, pp)
    pairs = [('mean', mean, want['mean']), ('invstd', invstd, want['invstd']), ('a', a, want['a']), ('dz', dz, wdz), ('dgamma', dgamma, wdg),
             ('dbeta', dbeta, wdb)]
    for name, got, w in pairs:
        print('bn_train %s %s: %d of %d elements differ in bits from the ordered restatement' % (what, name, int((_bits(got) != _bits(w)).sum()), w.size))
    if act != 'swish':
        _equal(what, pairs)
        return
    _equal(what, pairs[:2])
    r64 = ref.forward64(z, gamma, beta, eps, act)
    assert np.abs(r64['u']).max() < 87.0
    dz64, dg64, db64 = ref.backward64(da, z, gamma, beta, eps, act)
    r32 = ref.forward32(z, gamma, beta, eps, 0.9, act)
    dz32, dg32, db32 = ref.backward32(da, z, gamma, beta, r32['mean'], r32['invstd'], act)
    bad = []
    for name, got, w32, w64 in (('a', a, r32['a'], r64['a']), ('dz', dz, dz32, dz64), ('dgamma', dgamma, dg32, dg64), ('dbeta', dbeta, db32, db64)):
        e_dev, e_ref = ref.rel_err(got, w64), ref.rel_err(w32, w64)
        print('bn_train %s %s: device %.3e, sequential float32 restatement %.3e, bar %.3e' % (what, name, e_dev, e_ref, 4 * e_ref + EPS24))
        if not e_dev <= 4 * e_ref + EPS24:
            bad.append((name, e_dev, e_ref))
    assert not bad, bad


# ----------------------------------------------------------------------------- the binding under autograd
def test_autograd_gives_the_fenced_bytes(dev):
    """autograd.batchnorm_act on z [5, 58, 57, 64] (16530 pixels, 130 slabs) with gradients for z, gamma and beta: a, the moving
    statistics and the three gradients have the bytes of the fenced calls"""
    from yoloret_amd import autograd
    b, h, w, c = AUTOGRAD_SHAPE
    pixels = b * h * w
    assert geometry(pixels, c)[:2] == (128, 130)
    z, gamma, beta, da = rounding_case(pixels, c, seed=2)
    moving = (np.zeros(c, F32), np.ones(c, F32))
    a, mean, invstd, mm, mv = dev_forward(dev, z, gamma, beta, c, 1e-3, 0.9, 'relu6', c, moving=moving)
    dz, dgamma, dbeta = dev_backward(dev, da, z, gamma, beta, mean, invstd, c, 'relu6', c)
    tz = torch.from_numpy(z.reshape(b, h, w, c)).to(dev).requires_grad_(True)
    tg, tb = (torch.from_numpy(v).to(dev).requires_grad_(True) for v in (gamma, beta))
    tm, tv = torch.from_numpy(moving[0].copy()).to(dev), torch.from_numpy(moving[1].copy()).to(dev)
    ta = autograd.batchnorm_act(tz, tg, tb, tm, tv, 0.9, 1e-3, 'relu6')
    assert tuple(ta.shape) == AUTOGRAD_SHAPE
    gz, gg, gb = torch.autograd.grad(ta, (tz, tg, tb), torch.from_numpy(da.reshape(b, h, w, c)).to(dev))
    _equal('autograd', (('a', ta.detach().cpu().numpy().reshape(pixels, c), a), ('moving_mean', tm.cpu().numpy(), mm), ('moving_var', tv.cpu().numpy(), mv),
                        ('dz', gz.cpu().numpy().reshape(pixels, c), dz), ('dgamma', gg.cpu().numpy(), dgamma), ('dbeta', gb.cpu().numpy(), dbeta)))
