"""The fusing operators on the device (yoloret_amd/csrc/fusegrad.hip behind yr_maxpool_*, yr_upsample2_* and yr_wsum_*) against
tests/fusegrad_ref.py.

Every launch of a C entry runs between the guards of tests/fence.py, in CARRIERS as tests/test_gpu_bntrain.py builds them (`off` NaN
floats, the data, 63 NaN floats; off = 1 puts every base pointer 4 bytes past a 256-byte boundary), with outputs pre-filled with NaN,
rows of ld = C and ld = C + 5 floats whose pad columns are NaN and must keep their bits, and the workspace pre-filled with 0xFF.  The
two alignments and the two row forms alternate with the case number.

Max-pooling and the up-sampling forward only move values: bit-equal to the float32 restatement AND to float64 autograd.  The up-sampling
backward and d alpha of the weighted sum round: bit-equal to the restatement in the device's order, and
max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24 with E_ref the same figure of the float32 restatement; those cases print their
figures before they assert (run with -s)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import fence, fusegrad_ref as ref
from tests.test_gpu_bntrain import _bits, _carrier, _inner, _nan

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
YR_ERR_ARG = -1
NAN_BITS = np.float32(np.nan).view(np.uint32)
F32 = np.float32
PAD = 5

POOL_SHAPES = {2: [(2, 2), (3, 5), (5, 4), (7, 9), (26, 26)], 4: [(4, 4), (5, 7), (9, 11), (24, 24)]}
MAP_CHANNELS = [1, 3, 48, 75, 130]
BATCHES = [1, 3]
UP_SHAPES = [(1, 1), (2, 3), (7, 5), (13, 13)]
POOL_DATA = ['ints', 'const', 'relu6', 'normal']
WSUM_CHANNELS = [1, 3, 48, 75]
WSUM_MIN_ELEMS, WSUM_MAX_CHUNKS = 8192, 256          # WS_MIN_ELEMS, WS_MAX_CHUNKS of csrc/fusegrad.hip (tests/test_fusegrad_host.py reads them there)
WORKLOAD_LIKE = (33 * 2 * 26 * 26, 48)               # 2 * 26 * 26 pixels scaled until the slab cap sets the chunk: 44616 > 256 * 171


def wsum_min_chunk(c):
    return -(-WSUM_MIN_ELEMS // c)


def wsum_pixels(c):
    chunk = wsum_min_chunk(c)
    return [1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]


def _rt():
    from yoloret_amd import runtime
    return runtime


def _layout(n, c):
    """both alignments and dense / padded rows, alternating with the case number"""
    return n % 2, c + (n // 2) % 2 * PAD


def fenced(dev, off, launch, reads, writes, cols, ws_bytes=0, ws_fill=0xFF):
    """launch(read pointers, write pointers, workspace pointer) between the guards.  reads: arrays (None: a null pointer); writes: the
    initial contents of the written tensors; cols: per written tensor the columns the entry may write (the rest of each row must stay
    NaN); ws_fill: a byte, or 'random'.  -> the written tensors after the call."""
    rt = _rt()
    cr = [_carrier(a, dev, off) if a is not None else None for a in reads]
    cw = [_carrier(a, dev, off) for a in writes]
    if ws_fill == 'random':
        ws = torch.empty((ws_bytes + 16,), dtype=torch.uint8, device=dev).random_(0, 256)
    else:
        ws = torch.full((ws_bytes + 16,), ws_fill, dtype=torch.uint8, device=dev)

    def at(moved, c):
        return ctypes.c_void_p(moved(c[0]).data_ptr() + 4 * off) if c is not None else None

    def call(moved):
        launch([at(moved, c) for c in cr], [at(moved, c) for c in cw], rt._ptr(moved(ws)))
    with torch.cuda.device(dev):
        fence.run(call, writes=[c for c, _ in cw], reads=[c[0] for c in cr if c is not None], scratch=[ws])
    outs = []
    for (c, n), init, ncol in zip(cw, writes, cols):
        o = _inner(c, n, off, np.shape(init))
        assert np.all(_bits(o[..., ncol:]) == NAN_BITS), 'pad columns of an output were written'
        outs.append(o)
    return outs


# ----------------------------------------------------------------------------- the entries, fenced
def dev_maxpool(dev, x, c, k, ld, off=0):
    """x [B, H, W, x_ld] (pad columns NaN) -> y [B, OH, OW, ld]"""
    rt = _rt()
    b, h, w, x_ld = x.shape

    def launch(r, wr, ws):
        rt.check(rt.lib().yr_maxpool_forward(r[0], x_ld, b, h, w, c, k, wr[0], ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [x], [_nan(b, h // k, w // k, ld)], [c])[0]


def dev_maxpool_backward(dev, dy, x, c, k, ld, off=0):
    rt = _rt()
    b, h, w, x_ld = x.shape

    def launch(r, wr, ws):
        rt.check(rt.lib().yr_maxpool_backward(r[0], dy.shape[3], r[1], x_ld, b, h, w, c, k, wr[0], ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [dy, x], [_nan(b, h, w, ld)], [c])[0]


def dev_upsample(dev, x, c, ld, off=0):
    rt = _rt()
    b, h, w, x_ld = x.shape

    def launch(r, wr, ws):
        rt.check(rt.lib().yr_upsample2_forward(r[0], x_ld, b, h, w, c, wr[0], ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [x], [_nan(b, 2 * h, 2 * w, ld)], [c])[0]


def dev_upsample_backward(dev, dy, c, ld, off=0):
    rt = _rt()
    b, h2, w2, dy_ld = dy.shape

    def launch(r, wr, ws):
        rt.check(rt.lib().yr_upsample2_backward(r[0], dy_ld, b, h2 // 2, w2 // 2, c, wr[0], ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, [dy], [_nan(b, h2 // 2, w2 // 2, ld)], [c])[0]


def dev_wsum(dev, xs, alpha, c, ld, off=0):
    """xs four [P, x_ld] -> y [P, ld]"""
    rt = _rt()
    pixels = xs[0].shape[0]

    def launch(r, wr, ws):
        rt.check(rt.lib().yr_wsum_forward(r[0], xs[0].shape[1], r[1], xs[1].shape[1], r[2], xs[2].shape[1], r[3], xs[3].shape[1], r[4], pixels, c,
                                          wr[0], ld, rt.stream_ptr(dev)))
    return fenced(dev, off, launch, list(xs) + [alpha], [_nan(pixels, ld)], [c])[0]


def dev_wsum_backward(dev, dy, xs, alpha, c, ld, off=0, need=(True,) * 4, need_alpha=True, ws_fill=0xFF):
    """-> ([dx_i [P, ld] or None], dalpha [4] or None); without need_alpha the four maps and the workspace are null pointers"""
    rt = _rt()
    pixels = dy.shape[0]
    nbytes = rt.wsum_workspace_bytes(pixels, c)
    assert nbytes > 0
    which = [i for i in range(4) if need[i]]

    def launch(r, wr, ws):
        dx = [None] * 4
        for j, i in enumerate(which):
            dx[i] = wr[j]
        rt.check(rt.lib().yr_wsum_backward(r[0], dy.shape[1], r[2], ld, r[3], ld, r[4], ld, r[5], ld, r[1], pixels, c, dx[0], ld, dx[1], ld, dx[2], ld,
                                           dx[3], ld, wr[len(which)] if need_alpha else None, ws if need_alpha else None,
                                           nbytes if need_alpha else 0, rt.stream_ptr(dev)))
    reads = [dy, alpha] + ([ref.padded(x, ld) for x in xs] if need_alpha else [None] * 4)
    writes = [_nan(pixels, ld) for _ in which] + ([_nan(4)] if need_alpha else [])
    outs = fenced(dev, off, launch, reads, writes, [c] * len(which) + ([4] if need_alpha else []), nbytes, ws_fill)
    dxs = [None] * 4
    for j, i in enumerate(which):
        dxs[i] = outs[j]
    return dxs, (outs[len(which)] if need_alpha else None)


# ----------------------------------------------------------------------------- data
def pool_data(kind, shape, rng):
    if kind == 'ints':
        return rng.integers(-2, 3, shape).astype(F32)          # nearly every window ties
    if kind == 'const':
        return np.full(shape, F32(rng.choice([0.0, 6.0, -1.5])), F32)
    if kind == 'relu6':
        return np.clip(3 + 4 * rng.standard_normal(shape), 0, 6).astype(F32)          # exactly 0 or 6 over large areas
    assert kind == 'normal'
    return rng.standard_normal(shape).astype(F32)


def _same_bits(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), what


# ----------------------------------------------------------------------------- max-pooling
@pytest.mark.parametrize('kind', POOL_DATA)
@pytest.mark.parametrize('k', [2, 4])
def test_maxpool(dev, k, kind):
    n = 0
    for (h, w), c, b in itertools.product(POOL_SHAPES[k], MAP_CHANNELS, BATCHES):
        rng = np.random.default_rng(1000 * h + 10 * w + c + b)
        x = pool_data(kind, (b, h, w, c), rng)
        oh, ow = h // k, w // k
        dy = ref.ints(rng, (b, oh, ow, c)) if kind != 'normal' else rng.standard_normal((b, oh, ow, c)).astype(F32)
        off, ld = _layout(n, c)
        n += 1
        what = 'k=%d %s B=%d %dx%d C=%d ld=%d off=%d' % (k, kind, b, h, w, c, ld, off)
        y = dev_maxpool(dev, ref.padded(x, ld), c, k, ld, off)
        dx = dev_maxpool_backward(dev, ref.padded(dy, ld), ref.padded(x, ld), c, k, ld, off)
        _same_bits(y[..., :c], ref.maxpool32(x, k), 'forward ' + what)
        _same_bits(dx[..., :c], ref.maxpool_backward32(dy, x, k), 'backward ' + what)
        y64, dx64 = ref.maxpool_grads64(x, dy, k)
        _same_bits(y[..., :c], y64.astype(F32), 'forward against float64 ' + what)
        _same_bits(dx[..., :c], dx64.astype(F32), 'backward against float64 ' + what)
        strip = dx[..., :c].copy()
        strip[:, :oh * k, :ow * k] = 0
        assert not _bits(strip).any(), 'the trailing strip is +0 ' + what
        if kind != 'normal':
            assert dx[..., :c].astype(np.float64).sum() == dy.astype(np.float64).sum(), 'sum dx == sum dy ' + what


def test_maxpool_ties_and_zeros(dev):
    """2 x 2 windows by hand, one window a channel: the maximum at each of the four positions, all four tied, the last two tied,
    -0 against +0 both ways; the forward returns the first of the tied values, bits included"""
    x = np.array([[9, 1, 2, 3], [1, 9, 2, 3], [1, 2, 9, 3], [1, 2, 3, 9], [5, 5, 5, 5], [1, 2, 7, 7], [-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 0.0, -0.0]], F32)
    x = x.T.reshape(1, 2, 2, 8).copy()
    dy = np.arange(1, 9, dtype=F32).reshape(1, 1, 1, 8)
    y = dev_maxpool(dev, x, 8, 2, 8)
    dx = dev_maxpool_backward(dev, dy, x, 8, 2, 8)
    first = [0, 1, 2, 3, 0, 2, 0, 0]
    want = np.zeros((4, 8), F32)
    want[first, np.arange(8)] = dy.reshape(8)
    _same_bits(dx.reshape(4, 8), want, 'dx')
    _same_bits(y.reshape(8), np.array([9, 9, 9, 9, 5, 7, -0.0, 0.0], F32), 'y')


# ----------------------------------------------------------------------------- up-sampling
def test_upsample(dev):
    """Measured on an MI355X over the 40 cases: the backward equals the restatement bit for bit, so device = E_ref in every case,
    1.3e-08 .. 9.9e-08 (three additions), against bars of 1.1e-07 .. 4.6e-07."""
    bad, n = [], 0
    for (h, w), c, b in itertools.product(UP_SHAPES, MAP_CHANNELS, BATCHES):
        rng = np.random.default_rng(2000 * h + 10 * w + c + b)
        x = rng.standard_normal((b, h, w, c)).astype(F32)
        dy = rng.standard_normal((b, 2 * h, 2 * w, c)).astype(F32)
        off, ld = _layout(n, c)
        n += 1
        what = 'B=%d %dx%d C=%d ld=%d off=%d' % (b, h, w, c, ld, off)
        y = dev_upsample(dev, ref.padded(x, ld), c, ld, off)
        dx = dev_upsample_backward(dev, ref.padded(dy, ld), c, ld, off)
        y64, dx64 = ref.upsample_grads64(x, dy)
        _same_bits(y[..., :c], ref.upsample32(x), 'forward ' + what)
        _same_bits(y[..., :c], y64.astype(F32), 'forward against float64 ' + what)
        dx32 = ref.upsample_backward32(dy)
        _same_bits(dx[..., :c], dx32, 'backward ' + what)
        e_dev, e_ref = ref.rel_err(dx[..., :c], dx64), ref.rel_err(dx32, dx64)
        print('upsample2 backward %s: device %.3e, float32 restatement %.3e, bar %.3e' % (what, e_dev, e_ref, 4 * e_ref + EPS24))
        if not e_dev <= 4 * e_ref + EPS24:
            bad.append((what, e_dev, e_ref))
    assert not bad, bad


def test_upsample_backward_adds_in_the_stated_order(dev):
    """First block ((2^24 + 1) + 1) + 1: left to right every addition is absorbed (ties to even) and the block gives 2^24, where the ones
    paired first would give more.  Second block ((1 + 2^24) + -2^24) + 1 = 1, where 1 + (2^24 + (-2^24 + 1)) would give 2."""
    big = F32(2.0 ** 24)
    dy = np.array([[[big, 1, 1, big], [1, 1, -big, 1]]], F32).reshape(1, 2, 4, 1)
    dx = dev_upsample_backward(dev, dy, 1, 1)
    want = ref.upsample_backward32(dy)
    assert want.reshape(2).tolist() == [2.0 ** 24, 1.0]
    _same_bits(dx, want, 'dx')


# ----------------------------------------------------------------------------- the weighted sum
def wsum_case(pixels, c, exact, seed=0):
    """exact: integers in [-4, 4] everywhere (alpha too): every product and partial sum an integer; else normals"""
    rng = np.random.default_rng(400000 * seed + 1000 * c + pixels)
    if exact:
        xs = [ref.ints(rng, (pixels, c)) for _ in range(4)]
        return xs, ref.ints(rng, (pixels, c)), np.array([3, -2, 0, 1], F32)
    xs = [(rng.uniform(-1, 1) + rng.uniform(.5, 2) * rng.standard_normal((pixels, c))).astype(F32) for _ in range(4)]
    return xs, rng.standard_normal((pixels, c)).astype(F32), np.array([1.25, -0.7, 0.0, 0.33], F32) + F32(1e-3) * rng.standard_normal(4).astype(F32) * np.array([1, 1, 0, 1], F32)


def _check_wsum(dev, pixels, c, n, bad):
    rt = _rt()
    chunk = rt.wsum_chunk(pixels, c)
    off, ld = _layout(n, c)
    what = 'P=%d C=%d ld=%d off=%d chunk=%d' % (pixels, c, ld, off, chunk)
    # integers: everything exact in any order
    xs, dy, alpha = wsum_case(pixels, c, True)
    y = dev_wsum(dev, [ref.padded(x, ld) for x in xs], alpha, c, ld, off)
    _same_bits(y[:, :c], ref.wsum32(xs, alpha), 'forward, integers ' + what)
    dxs, dalpha = dev_wsum_backward(dev, ref.padded(dy, ld), xs, alpha, c, ld, off)
    for i, want in enumerate(ref.wsum_dx32(dy, alpha)):
        _same_bits(dxs[i][:, :c], want, 'dx%d, integers %s' % (i, what))
    exact = np.array([(dy.astype(np.float64) * x.astype(np.float64)).sum() for x in xs])
    assert max(np.abs(dy.astype(np.float64) * x.astype(np.float64)).sum() for x in xs) < 2 ** 24, 'every partial sum is an integer below 2^24'
    _same_bits(dalpha, exact.astype(F32), 'dalpha, integers ' + what)
    # normals: the device's order bit for bit, and the bar against float64
    xs, dy, alpha = wsum_case(pixels, c, False)
    y = dev_wsum(dev, [ref.padded(x, ld) for x in xs], alpha, c, ld, off)
    _same_bits(y[:, :c], ref.wsum32(xs, alpha), 'forward ' + what)
    dxs, dalpha = dev_wsum_backward(dev, ref.padded(dy, ld), xs, alpha, c, ld, off)
    for i, want in enumerate(ref.wsum_dx32(dy, alpha)):
        _same_bits(dxs[i][:, :c], want, 'dx%d %s' % (i, what))
    _same_bits(dalpha, np.array([ref.ordered_dot(dy, x, chunk) for x in xs], F32), 'dalpha in the device\'s order ' + what)
    _, _, da64 = ref.wsum_grads64(xs, alpha, dy)
    seq = np.array([ref.seq_dot(dy, x) for x in xs], F32)
    e_dev, e_ref = ref.rel_err(dalpha, da64), ref.rel_err(seq, da64)
    print('wsum dalpha %s: device %.3e, float32 restatement %.3e, bar %.3e' % (what, e_dev, e_ref, 4 * e_ref + EPS24))
    if not e_dev <= 4 * e_ref + EPS24:
        bad.append((what, e_dev, e_ref))


@pytest.mark.parametrize('c', WSUM_CHANNELS)
def test_wsum(dev, c):
    bad = []
    for n, pixels in enumerate(wsum_pixels(c)):
        _check_wsum(dev, pixels, c, n, bad)
    assert not bad, bad


def test_wsum_where_the_slab_cap_sets_the_chunk(dev):
    bad = []
    _check_wsum(dev, WORKLOAD_LIKE[0], WORKLOAD_LIKE[1], 0, bad)
    assert not bad, bad


@pytest.mark.parametrize('c', WSUM_CHANNELS)
def test_wsum_forward_equals_the_plan_op(dev, c):
    """YR_OP_WSUM through runtime.run_op on the same four maps as identity sources (its rows need a stride that is a multiple of 4 and
    16-byte alignment, so the maps are copied into rows of round_up(C, 4) floats): the same float32 bits"""
    rt = _rt()
    for pixels in (65, 2 * wsum_min_chunk(c) + 1):
        xs, _, alpha = wsum_case(pixels, c, False, seed=1)
        y = dev_wsum(dev, xs, alpha, c, c)
        ld4 = (c + 3) // 4 * 4
        ts = []
        for x in xs:
            t = torch.zeros((1, 1, pixels, ld4), dtype=torch.float32, device=dev)
            t[0, 0, :, :c] = torch.from_numpy(x).to(dev)
            ts.append(t)
        ad = torch.from_numpy(alpha).to(dev)
        out = torch.full((1, 1, pixels, ld4), float('nan'), dtype=torch.float32, device=dev)
        op = rt.new_op(rt.OP_WSUM)
        op.h, op.w, op.cin, op.cout, op.nsrc = 1, pixels, c, c, 4
        for i, t in enumerate(ts):
            op.src[i] = rt.make_src(t, c=c, xform='identity')
        op.wgt = ad.data_ptr()
        op.out, op.out_ld = out.data_ptr(), ld4
        rt.run_op(op, 1)
        torch.cuda.synchronize()
        _same_bits(y, out[0, 0, :, :c].cpu().numpy(), 'P=%d C=%d' % (pixels, c))


def test_wsum_backward_optional_outputs_and_workspace_contents(dev):
    """every combination of null dx_i / null dalpha leaves the other outputs bit-equal; 0xFF, 0x00 and random workspaces give the same bytes"""
    c = 3
    pixels = 2 * wsum_min_chunk(c) + 1
    xs, dy, alpha = wsum_case(pixels, c, False, seed=2)
    full_dx, full_da = dev_wsum_backward(dev, dy, xs, alpha, c, c)
    assert all(np.isfinite(v).all() for v in full_dx) and np.isfinite(full_da).all()
    for n, (need_alpha, n0, n1, n2, n3) in enumerate(itertools.product([True, False], repeat=5)):
        need = (n0, n1, n2, n3)
        dxs, da = dev_wsum_backward(dev, dy, xs, alpha, c, c, off=n % 2, need=need, need_alpha=need_alpha)
        for i in range(4):
            assert (dxs[i] is None) == (not need[i])
            if need[i]:
                _same_bits(dxs[i], full_dx[i], 'dx%d with %r, dalpha %r' % (i, need, need_alpha))
        assert (da is None) == (not need_alpha)
        if need_alpha:
            _same_bits(da, full_da, 'dalpha with %r' % (need,))
    for fill in (0x00, 'random'):
        dxs, da = dev_wsum_backward(dev, dy, xs, alpha, c, c, ws_fill=fill)
        _same_bits(da, full_da, 'dalpha from a workspace of %r' % (fill,))
        for i in range(4):
            _same_bits(dxs[i], full_dx[i], 'dx%d from a workspace of %r' % (i, fill))
    # the binding gives what the fenced calls gave
    rt = _rt()
    tx, tdy, ta = [torch.from_numpy(x).to(dev) for x in xs], torch.from_numpy(dy).to(dev), torch.from_numpy(alpha).to(dev)
    ws = torch.empty((rt.wsum_workspace_bytes(pixels, c) + 64,), dtype=torch.uint8, device=dev).random_(0, 256)
    tdx, tda = rt.wsum_backward(tdy, tx, ta, workspace=ws)
    _same_bits(tda.cpu().numpy(), full_da, 'binding dalpha')
    for i in range(4):
        _same_bits(tdx[i].cpu().numpy(), full_dx[i], 'binding dx%d' % i)
    tdx, tda = rt.wsum_backward(tdy, None, ta, need=(False, True, False, False), need_alpha=False)
    assert tda is None and tdx[0] is None and tdx[2] is None and tdx[3] is None
    _same_bits(tdx[1].cpu().numpy(), full_dx[1], 'binding dx1 alone')
    _same_bits(rt.wsum_forward(tx, ta).cpu().numpy(), ref.wsum32(xs, alpha), 'binding forward')


# ----------------------------------------------------------------------------- all three
def test_an_image_alone_equals_its_slice_of_the_batch(dev):
    rng = np.random.default_rng(5)
    b, c = 3, 75
    x = pool_data('relu6', (b, 9, 11, c), rng)
    for k in (2, 4):
        dy = rng.standard_normal((b, 9 // k, 11 // k, c)).astype(F32)
        y, dx = dev_maxpool(dev, x, c, k, c), dev_maxpool_backward(dev, dy, x, c, k, c)
        _same_bits(dev_maxpool(dev, x[1:2], c, k, c), y[1:2], 'maxpool %d' % k)
        _same_bits(dev_maxpool_backward(dev, dy[1:2], x[1:2], c, k, c), dx[1:2], 'maxpool %d backward' % k)
    dy = rng.standard_normal((b, 18, 22, c)).astype(F32)
    _same_bits(dev_upsample(dev, x[1:2], c, c), dev_upsample(dev, x, c, c)[1:2], 'upsample2')
    _same_bits(dev_upsample_backward(dev, dy[1:2], c, c), dev_upsample_backward(dev, dy, c, c)[1:2], 'upsample2 backward')
    xs, dyw, alpha = wsum_case(b * 99, c, False, seed=3)
    y = dev_wsum(dev, xs, alpha, c, c)
    dxs, _ = dev_wsum_backward(dev, dyw, xs, alpha, c, c)
    _same_bits(dev_wsum(dev, [v[99:198] for v in xs], alpha, c, c), y[99:198], 'wsum')
    one, _ = dev_wsum_backward(dev, dyw[99:198], [v[99:198] for v in xs], alpha, c, c)
    for i in range(4):
        _same_bits(one[i], dxs[i][99:198], 'wsum dx%d' % i)


def test_refusals_change_nothing(dev):
    rt = _rt()
    L = rt.lib()
    p, s = rt._ptr, rt.stream_ptr(dev)
    nan = float('nan')
    b, h, w, c = 2, 6, 8, 8
    big = torch.zeros((b, 2 * h, 2 * w, c), dtype=torch.float32, device=dev)
    mid = torch.zeros((b, h, w, c), dtype=torch.float32, device=dev)
    alpha = torch.ones((4,), dtype=torch.float32, device=dev)
    outs = {k: torch.full(shape, nan, dtype=torch.float32, device=dev)
            for k, shape in (('big', (b, 2 * h, 2 * w, c)), ('mid', (b, h, w, c)), ('small', (b, h // 2, w // 2, c)), ('dalpha', (4,)))}
    pixels = b * h * w
    need = rt.wsum_workspace_bytes(pixels, c)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)
    o = outs

    def order(g, keys, kw):
        g.update(kw)
        return tuple(g[k] for k in keys) + (s,)

    def mpf(**kw):
        return order(dict(x=p(mid), x_ld=c, B=b, H=h, W=w, C=c, k=2, y=p(o['small']), y_ld=c), ('x', 'x_ld', 'B', 'H', 'W', 'C', 'k', 'y', 'y_ld'), kw)

    def mpb(**kw):
        return order(dict(dy=p(mid), dy_ld=c, x=p(mid), x_ld=c, B=b, H=h, W=w, C=c, k=2, dx=p(o['mid']), dx_ld=c),
                     ('dy', 'dy_ld', 'x', 'x_ld', 'B', 'H', 'W', 'C', 'k', 'dx', 'dx_ld'), kw)

    def usf(**kw):
        return order(dict(x=p(mid), x_ld=c, B=b, H=h, W=w, C=c, y=p(o['big']), y_ld=c), ('x', 'x_ld', 'B', 'H', 'W', 'C', 'y', 'y_ld'), kw)

    def usb(**kw):
        return order(dict(dy=p(big), dy_ld=c, B=b, H=h, W=w, C=c, dx=p(o['mid']), dx_ld=c), ('dy', 'dy_ld', 'B', 'H', 'W', 'C', 'dx', 'dx_ld'), kw)

    def wsf(**kw):
        g = dict(alpha=p(alpha), pixels=pixels, C=c, y=p(o['mid']), y_ld=c)
        keys = []
        for i in range(4):
            g['x%d' % i], g['x%d_ld' % i] = p(mid), c
            keys += ['x%d' % i, 'x%d_ld' % i]
        return order(g, keys + ['alpha', 'pixels', 'C', 'y', 'y_ld'], kw)

    def wsb(**kw):
        g = dict(dy=p(mid), dy_ld=c, alpha=p(alpha), pixels=pixels, C=c, dalpha=p(o['dalpha']), ws=p(ws), ws_bytes=need)
        keys, dkeys = ['dy', 'dy_ld'], []
        for i in range(4):
            g['x%d' % i], g['x%d_ld' % i], g['dx%d' % i], g['dx%d_ld' % i] = p(mid), c, (p(o['mid']) if i == 0 else None), c
            keys += ['x%d' % i, 'x%d_ld' % i]
            dkeys += ['dx%d' % i, 'dx%d_ld' % i]
        return order(g, keys + ['alpha', 'pixels', 'C'] + dkeys + ['dalpha', 'ws', 'ws_bytes'], kw)
    odd = ctypes.c_void_p(o['mid'].data_ptr() + 2)
    misaligned = ctypes.c_void_p(ws.data_ptr() + 4)
    huge = dict(B=1 << 20, H=1 << 10, W=1 << 9)          # 2^39 pixels: rows of 2^30 floats put byte offsets beyond 2^63
    cases = [
        (L.yr_maxpool_forward, [('k 3', mpf(k=3)), ('k 1', mpf(k=1)), ('B 0', mpf(B=0)), ('H 0', mpf(H=0)), ('W 0', mpf(W=0)), ('C 0', mpf(C=0)), ('H < k', mpf(H=1)),
                                ('W < k', mpf(W=3, k=4)), ('x_ld < C', mpf(x_ld=c - 1)), ('y_ld < C', mpf(y_ld=c - 1)), ('null x', mpf(x=None)), ('null y', mpf(y=None)),
                                ('y not 4-byte aligned', mpf(y=odd)), ('2^40 pixels', mpf(B=1 << 20, H=1 << 10, W=1 << 10)),
                                ('row offsets', mpf(x_ld=1 << 30, y_ld=1 << 30, **huge))]),
        (L.yr_maxpool_backward, [('k 3', mpb(k=3)), ('B 0', mpb(B=0)), ('H -1', mpb(H=-1)), ('C 0', mpb(C=0)), ('W < k', mpb(W=1)), ('dy_ld < C', mpb(dy_ld=c - 1)),
                                 ('x_ld < C', mpb(x_ld=c - 1)), ('dx_ld < C', mpb(dx_ld=c - 1)), ('null dy', mpb(dy=None)), ('null x', mpb(x=None)),
                                 ('null dx', mpb(dx=None)), ('dx not 4-byte aligned', mpb(dx=odd)), ('row offsets', mpb(dx_ld=1 << 30, **huge))]),
        (L.yr_upsample2_forward, [('B 0', usf(B=0)), ('H 0', usf(H=0)), ('W 0', usf(W=0)), ('C 0', usf(C=0)), ('x_ld < C', usf(x_ld=c - 1)), ('y_ld < C', usf(y_ld=c - 1)),
                                  ('null x', usf(x=None)), ('null y', usf(y=None)), ('2^38 pixels', usf(B=1 << 18, H=1 << 10, W=1 << 10)),
                                  ('row offsets', usf(y_ld=1 << 30, B=1 << 17, H=1 << 10, W=1 << 10))]),
        (L.yr_upsample2_backward, [('B 0', usb(B=0)), ('H 0', usb(H=0)), ('W -2', usb(W=-2)), ('C 0', usb(C=0)), ('dy_ld < C', usb(dy_ld=c - 1)), ('dx_ld < C', usb(dx_ld=c - 1)),
                                   ('null dy', usb(dy=None)), ('null dx', usb(dx=None)), ('dx not 4-byte aligned', usb(dx=odd)),
                                   ('row offsets', usb(dy_ld=1 << 30, B=1 << 17, H=1 << 10, W=1 << 10))]),
        (L.yr_wsum_forward, [('pixels 0', wsf(pixels=0)), ('pixels 2^40', wsf(pixels=1 << 40)), ('C 0', wsf(C=0)), ('C 2^30 + 1', wsf(C=(1 << 30) + 1)),
                             ('x2_ld < C', wsf(x2_ld=c - 1)), ('y_ld < C', wsf(y_ld=c - 1)), ('null x3', wsf(x3=None)), ('null alpha', wsf(alpha=None)),
                             ('null y', wsf(y=None)), ('row offsets', wsf(pixels=1 << 39, y_ld=1 << 30))]),
        (L.yr_wsum_backward, [('pixels 0', wsb(pixels=0)), ('pixels -1', wsb(pixels=-1)), ('C 0', wsb(C=0)), ('dy_ld < C', wsb(dy_ld=c - 1)), ('x1_ld < C', wsb(x1_ld=c - 1)),
                              ('dx0_ld < C', wsb(dx0_ld=c - 1)), ('null dy', wsb(dy=None)), ('null alpha', wsb(alpha=None)), ('null x2 with dalpha', wsb(x2=None)),
                              ('null workspace', wsb(ws=None)), ('short workspace', wsb(ws_bytes=need - 1)), ('misaligned workspace', wsb(ws=misaligned)),
                              ('dx0 not 4-byte aligned', wsb(dx0=odd)), ('row offsets', wsb(pixels=1 << 39, dy_ld=1 << 30))]),
    ]
    with torch.cuda.device(dev):
        for entry, rows in cases:
            for what, args in rows:
                assert entry(*args) == YR_ERR_ARG, '%s: %s' % (entry.__name__, what)
                assert L.yr_last_error()
    torch.cuda.synchronize()
    for t in outs.values():
        assert np.all(_bits(t.cpu().numpy()) == NAN_BITS)
    assert bool((ws == 0xFF).all()) and not bool(mid.any()) and not bool(big.any()) and bool((alpha == 1).all())
    for bad in ((0, 8), (-1, 8), (1 << 40, 8), (40, 0), (40, -3), (40, (1 << 30) + 1)):
        assert rt.wsum_chunk(*bad) == 0 and rt.wsum_workspace_bytes(*bad) == 0
    # the binding's own checks
    for call in (lambda: rt.maxpool_forward(mid, 3), lambda: rt.maxpool_forward(mid.cpu(), 2), lambda: rt.maxpool_forward(mid[:, :1].contiguous(), 2),
                 lambda: rt.maxpool_backward(mid, mid, 2), lambda: rt.maxpool_forward(mid, 2, out=torch.empty_like(mid)),
                 lambda: rt.upsample2_forward(mid[0]), lambda: rt.upsample2_backward(mid[:, :5].contiguous()),
                 lambda: rt.wsum_forward([mid] * 3, alpha), lambda: rt.wsum_forward([mid] * 4, alpha[:3].contiguous()),
                 lambda: rt.wsum_forward([mid, mid, mid, big], alpha), lambda: rt.wsum_backward(mid, None, alpha),
                 lambda: rt.wsum_backward(mid, [mid] * 4, alpha, need=(True,) * 3),
                 lambda: rt.wsum_backward(mid, [mid] * 4, alpha, workspace=torch.empty(8, dtype=torch.uint8, device=dev)),
                 lambda: rt.wsum_backward(mid, [mid] * 4, alpha, need=(False,) * 4, out=[torch.empty_like(mid)] + [None] * 3)):
        with pytest.raises(ValueError):
            call()
