"""Every form of the inference depthwise convolution (YR_OP_DEPTHWISE) against the float64 definition, on EXACT data.

Three kernel families serve the op - dw_kernel (depthwise.hip), dwp_kernel (depthwise_lds.hip, a walker per run of tiles) and
dwq_kernel (depthwise_walk.hip, 5 x 5) - and host-side cost models pick the family, the template instantiation and the geometry
from the map's size.  tests/depthwise_geo.py restates those choices and builds the case tables (tests/test_depthwise_geo_host.py
pins both); here every case

  * asserts the kernel name the launch reports (yr_last_kernel) against the mirror's prediction - family and template arguments;
  * runs between red zones (tests/fence.py), output pre-filled with NaN, row strides alternately dense and wider than the padded
    width, pad channels poisoned as the other op tests poison them (16-bit: NaN; float32: zeros, whose products stay finite);
  * uses data on which the arithmetic is exact: inputs in -2 .. 2, taps in -2 .. 2, BatchNorm scale in {1, -1, 0.5, 2}, shift in
    -3 .. 3.  Every product, every partial sum in any order (an integer of magnitude <= 100), every value before and after the
    activation and every squeeze-excite sum is representable - the map values in bfloat16's 8 significant bits, asserted on the
    float64 reference before the launch.  Nothing is rounded anywhere, so for activations `none` and `relu6` the device must EQUAL
    oracle.nn.depthwise in float64 in float32, bfloat16 and float16 (as numbers: identical bits but for the sign of a zero), and
    each row of squeeze-excite sums must equal the sum of the stored values of its own region.
  * swish cases (not exact) keep the bars of the other op tests: assert_rounded_once for 16-bit maps, TOL for float32.

The 5 x 5 instances of dwp_kernel run only with YOLORET_DW_WALK=0, which the library reads once per process: not reachable here.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import nn
from tests import depthwise_geo as G
from tests import fence
from tests.util import assert_close, assert_rounded_once, from_dev16, q16, round_up, to_dev16

pytestmark = pytest.mark.gpu

DTYPES16 = ['bf16', 'f16']
DTYPES = ['f32', 'bf16', 'f16']
TOL = 2e-5          # the float32 bar of tests/test_gpu_ops.py
SCALES = np.array([1.0, -1.0, 0.5, 2.0])


def _rt():
    from yoloret_amd import runtime as rt
    return rt


def _act(x, act):
    return {'none': lambda v: v, 'relu6': nn.relu6, 'swish': nn.swish}[act](x)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=6)
def _exact_case(k, s, b, h, w, c, act):
    """(x, taps, scale, shift, float64 reference) - computed once per shape, shared by the element types and forms, read-only."""
    rng = np.random.default_rng([k, s, b, h, w, c])
    x = rng.integers(-2, 3, (b, h, w, c)).astype(np.float64)
    wk = rng.integers(-2, 3, (k, k, c)).astype(np.float64)
    scale = SCALES[rng.integers(0, 4, c)]
    shift = rng.integers(-3, 4, c).astype(np.float64)
    pre = nn.depthwise(x, wk, s, 'same') * scale + shift
    ref = _act(pre, act)
    # exactness, asserted and not assumed: any partial sum of the taps is an integer bounded by max|x| * sum|taps| <= 256 (the
    # integers bfloat16 holds), and the values before and after the activation survive a rounding to bfloat16 unchanged
    assert np.abs(x).max() * np.abs(wk).sum(axis=(0, 1)).max() <= 256
    assert np.array_equal(q16(pre, 'bf16'), pre)
    if act != 'swish':
        assert np.array_equal(q16(ref, 'bf16'), ref) and np.array_equal(q16(ref, 'f16'), ref)
    return _frozen(x, wk, scale, shift, ref)


def _to_dev(a, dev, dt, ld):
    """[B,H,W,C] -> device [B,H,W,ld]: 16-bit pad channels NaN; float32 pad channels up to the vector zero (they meet zero weights), the
    channels of a wider row NaN (no lane may read them)"""
    if dt != 'f32':
        return to_dev16(a, dev, dt, ld=ld)
    c = a.shape[-1]
    p = np.full(a.shape[:-1] + (ld,), np.nan, np.float32)
    p[..., :round_up(c, 4)] = 0.0
    p[..., :c] = a
    return torch.from_numpy(p).to(dev)


def _from_dev(t, dt, c):
    return (t.detach().cpu().numpy()[..., :c] if dt == 'f32' else from_dev16(t, dt, c)).astype(np.float64)


def _params(dev, dt, wk, scale, shift):
    rt = _rt()
    k, c = wk.shape[0], wk.shape[2]
    ldc = round_up(c, rt.VEC[rt.dtype_id(dt)])
    wp = np.zeros((k * k, ldc), np.float32)
    wp[:, :c] = wk.reshape(k * k, c)
    sc, sh = np.zeros(ldc, np.float32), np.zeros(ldc, np.float32)
    sc[:c], sh[:c] = scale, shift
    return [torch.from_numpy(v.ravel().copy()).to(dev) for v in (wp, sc, sh)]


def _launch(dev, dt, xd, c, keep, k, s, act, b, wide_out=False, se_rows=0):
    """One YR_OP_DEPTHWISE launch between red zones -> (out [b,ho,wo,ld_out], part [b,rows,ldc] | None, the kernel's name)."""
    rt = _rt()
    did = rt.dtype_id(dt)
    V = rt.VEC[did]
    ldc = round_up(c, V)
    h, w = xd.shape[1], xd.shape[2]
    ho, wo = -(-h // s), -(-w // s)
    out = torch.full((b, ho, wo, ldc + (2 * V if wide_out else 0)), float('nan'), dtype=rt.TORCH_DTYPE[did], device=dev)
    part = torch.full((b, se_rows, ldc), float('nan'), dtype=torch.float32, device=dev) if se_rows else None
    op = rt.new_op(rt.OP_DEPTHWISE, act)
    op.dtype = op.out_dtype = did
    op.h, op.w, op.cin, op.cout, op.k, op.stride, op.nsrc = ho, wo, c, c, k, s, 1
    op.src[0] = rt.make_src(xd, c=c)
    op.wgt, op.scale, op.shift = [t.data_ptr() for t in keep]
    op.out, op.out_ld = out.data_ptr(), out.shape[3]
    if part is not None:
        op.gate, op.gate_ld, op.se_reduced = part.data_ptr(), ldc, se_rows
    fence.run_op(op, b, writes=[out] + ([part] if part is not None else []), reads=[xd] + keep, cols=ldc)
    name = rt.lib().yr_last_kernel().decode()
    torch.cuda.synchronize()
    return out, part, name


def _check_map(got, ref, dt, act, what):
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    if act == 'swish':
        if dt == 'f32':
            assert_close(got, ref, TOL, what)
        else:
            assert_rounded_once(got, ref, dt, what)
        return
    bad = got != ref
    assert not bad.any(), '%s: %d of %d elements differ from the exact result, first at %s: %r != %r' % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref[bad][0])


def _check_rows(part, stored, regions, c, act, what):
    """Row i of `part` is the sum of the STORED values of region i: exactly on exact data (every sum a multiple of 1/2 far below 2^24),
    else within the error of a float32 sum of n terms in any order, (n - 1) * 2^-24 * sum |v|."""
    rows = part.detach().cpu().numpy()[..., :c].astype(np.float64)
    assert rows.shape[1] == len(regions), what
    assert np.isfinite(rows).all(), '%s: a row of sums was left unwritten' % what
    for i, (y0, y1, x0, x1) in enumerate(regions):
        v = stored[:, y0:y1, x0:x1]
        want = v.sum(axis=(1, 2))
        n = (y1 - y0) * (x1 - x0)
        if act == 'swish':
            assert (np.abs(rows[:, i] - want) <= n * 2.0 ** -24 * np.abs(v).sum(axis=(1, 2)) + 1e-30).all(), (what, i)
        else:
            assert n * np.abs(v).max() * 2 < 2 ** 24
            assert np.array_equal(rows[:, i], want), '%s: row %d (rows %d..%d, columns %d..%d) is not the sum of its region' % (what, i, y0, y1, x0, x1)


def _run_exact(dev, dt, k, s, b, h, w, c, act, se_rows=0, wide=False):
    x, wk, scale, shift, ref = _exact_case(k, s, b, h, w, c, act)
    rt = _rt()
    ldc = round_up(c, rt.VEC[rt.dtype_id(dt)])
    xd = _to_dev(x, dev, dt, ldc + (rt.VEC[rt.dtype_id(dt)] if not wide else 0))       # (source and output rows: one wide, one dense)
    out, part, name = _launch(dev, dt, xd, c, _params(dev, dt, wk, scale, shift), k, s, act, b, wide_out=wide, se_rows=se_rows)
    got = _from_dev(out, dt, c)
    return got, ref, part, name


# ------------------------------------------------------------------------------------------------ 1. every dwp class, 3 x 3
def _dwp_ids(se):
    return ['tw%d-th%d-R%d-nb%d-big%d' % cls for cls, _, _ in G.dwp_class_cases(se)]


def _dwp_class_case(dev, dt, se, cls, one, many):
    b = 2
    runs = [(one, 'none', False, G.DWP_C), (one, 'relu6', True, G.TAIL_C)]
    if many is not None:
        runs += [(many, 'relu6', False, G.DWP_C), (many, 'swish', True, G.TAIL_C)]
    for (h, w), act, wide, c in runs:
        g = G.dwp_geometry(h, w, 3, se)
        assert G.dwp_class(g) == cls
        what = 'dwp %s %dx%dx%d %s se=%d %s' % (dt, h, w, c, act, se, g)
        got, ref, part, name = _run_exact(dev, dt, 3, 1, b, h, w, c, act, se_rows=g.ntx * g.nty if se else 0, wide=wide)
        assert name == G.dwp_name(dt, 3, act, se, g.R), (what, name)
        _check_map(got, ref, dt, act, what)
        if se:
            _check_rows(part, got, G.dwp_tile_regions(h, w, g), c, act, what)


@pytest.mark.parametrize('dt', DTYPES16)
@pytest.mark.parametrize('cls,one,many', G.dwp_class_cases(False), ids=_dwp_ids(False))
def test_dwp_every_class_plain(dev, dt, cls, one, many):
    """Each of the 37 (tw, th, R, nband, nbig) classes of the plain 3 x 3 form: its smallest map (one tile) and, where the class has
    one, its smallest map of 2 x 2 tiles or more whose last tile is cut short along x and y.  72 channels: a whole 64-channel chunk
    and a chunk of one vector (the second run of each map: 76, the last vector half filled)."""
    _dwp_class_case(dev, dt, False, cls, one, many)


@pytest.mark.parametrize('dt', DTYPES16)
@pytest.mark.parametrize('cls,one,many', G.dwp_class_cases(True), ids=_dwp_ids(True))
def test_dwp_every_class_se(dev, dt, cls, one, many):
    """The 33 classes of the squeeze-excite 3 x 3 form; the sums row by row: each the exact sum of what its own tile stored."""
    _dwp_class_case(dev, dt, True, cls, one, many)


# ------------------------------------------------------------------------------------------------ 2. multi-tile walks
@pytest.mark.parametrize('dt', DTYPES16)
@pytest.mark.parametrize('se', [False, True], ids=['plain', 'se'])
@pytest.mark.parametrize('ci', range(len(G.WALK_CASES)), ids=['%dx%d-b%d' % v for v in G.WALK_CASES])
def test_dwp_multi_tile_walks(dev, dt, se, ci):
    """1024 channels leave 48 walkers per 64-channel chunk: each walks a run of one, two or three tiles (the prefetch of the next
    tile into the other LDS buffer, the wait count behind a tile's stores, the buffer flip, the squeeze-excite flush of the tile
    before; runs that end in either buffer, that pass into the next tile row and into the next image - asserted on the mirror).
    Every image against float64; the sums tile by tile."""
    h, w, b = G.WALK_CASES[ci]
    c = G.WALK_C
    g = G.dwp_geometry(h, w, 3, se)
    lengths, _, _ = G.dwp_run_facts(b, c, g)
    assert max(lengths) >= 2 and len(G.dwp_runs(b, c, g)) == 48
    act = ('none', 'relu6', 'none')[ci]
    what = 'dwp walk %s %dx%dx%d b%d se=%d runs %s' % (dt, h, w, c, b, se, sorted(lengths))
    got, ref, part, name = _run_exact(dev, dt, 3, 1, b, h, w, c, act, se_rows=g.ntx * g.nty if se else 0, wide=bool(ci & 1))
    assert name == G.dwp_name(dt, 3, act, se, g.R), (what, name)
    _check_map(got, ref, dt, act, what)
    if se:
        _check_rows(part, got, G.dwp_tile_regions(h, w, g), c, act, what)


# ------------------------------------------------------------------------------------------------ 4. (and 3.) dwq, every class
@pytest.mark.parametrize('dt', DTYPES16)
@pytest.mark.parametrize('se', [False, True], ids=['plain', 'se'])
@pytest.mark.parametrize('ci', range(len(G.DWQ_CASES)), ids=['%dx%d-b%d' % v for v in G.DWQ_CASES])
def test_dwq_every_class(dev, dt, se, ci):
    """The walking 5 x 5 form in every (strips per block, images and waves per workgroup, pixel groups per row) class, with last
    quanta of 1, 2, 3 and 4 rows, maps lower than the kernel, odd batches where a workgroup takes two images, several column
    blocks.  The sums row by row: each the exact sum of what its (column block, row quantum) stored."""
    from yoloret_amd.compiler import DW_LDS, DW_WALK
    assert DW_LDS and DW_WALK, 'the suite runs the default forms'
    h, w, b = G.DWQ_CASES[ci]
    c = (G.DWP_C, G.TAIL_C)[ci % 2]
    g = G.dwq_geometry(h, w, b, 5, se)
    for act, wide in ((('none', 'relu6')[ci & 1], bool(ci & 2)),) + ((('swish', True),) if ci % 4 == 0 else ()):
        what = 'dwq %s %dx%dx%d b%d %s se=%d %s' % (dt, h, w, c, b, act, se, g)
        got, ref, part, name = _run_exact(dev, dt, 5, 1, b, h, w, c, act, se_rows=g.nblk * g.nq if se else 0, wide=wide)
        assert name == G.dwq_name(dt, 5, act, se), (what, name)
        _check_map(got, ref, dt, act, what)
        if se:
            _check_rows(part, got, G.dwq_regions(h, w, g), c, act, what)


@pytest.mark.parametrize('dt', DTYPES16)
@pytest.mark.parametrize('se', [False, True], ids=['plain', 'se'])
@pytest.mark.parametrize('ci', range(len(G.DWQ_SEG_CASES)), ids=['%dx%d-b%d' % v for v in G.DWQ_SEG_CASES])
def test_dwq_segments_of_several_quanta(dev, dt, se, ci):
    """A workgroup that walks through several row quanta: no vertical halo between them, and the squeeze-excite sums of quantum
    qi leave in the middle of the walk (alternating halves of the LDS scratch, the row after a quantum's end already counted for
    the next one).  The launcher cuts segments longer than a quantum only when the workgroups outnumber the chip's slots - here 16
    chunks of 64 channels x 100 or 127 images of a one-strip map (the mirror's dwq_segments asserts the case)."""
    h, w, b = G.DWQ_SEG_CASES[ci]
    c = G.WALK_C
    g = G.dwq_geometry(h, w, b, 5, se)
    qps, nseg = G.dwq_segments(h, w, b, c, 5, se)
    assert qps >= 2 and g.nq > qps * (nseg - 1) and G.dwq_last_quantum(h, g) < g.Q
    act = ('relu6', 'none')[ci]
    what = 'dwq %s %dx%dx%d b%d %s se=%d %s segments of %d quanta' % (dt, h, w, c, b, act, se, g, qps)
    got, ref, part, name = _run_exact(dev, dt, 5, 1, b, h, w, c, act, se_rows=g.nblk * g.nq if se else 0, wide=bool(ci))
    assert name == G.dwq_name(dt, 5, act, se), (what, name)
    _check_map(got, ref, dt, act, what)
    if se:
        _check_rows(part, got, G.dwq_regions(h, w, g), c, act, what)


# ------------------------------------------------------------------------------------------------ 5. dw_kernel, every instantiation
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('ci', range(len(G.DW_SMALL_CASES)), ids=['k%d-s%d-%dx%d-b%d' % v for v in G.DW_SMALL_CASES])
def test_dw_kernel_small_instantiations(dev, dt, ci):
    """<3,1,4,1>, <3,2,2,1>, <5,1,4,1> and <5,2,2,1> (x patch, y patch) in the three element types: odd and even maps (the 'SAME'
    padding of a stride-2 map differs between them), a channel tail, several workgroups."""
    k, s, h, w, b = G.DW_SMALL_CASES[ci]
    c = G.DW_SMALL_C[dt]
    vec = 4 if dt == 'f32' else 8
    inst = G.dw_instance(k, s, b, h, w, c, vec)
    assert inst[3] == 1
    for act, wide in ((('none', 'relu6')[ci & 1], bool(ci & 2)),) + ((('swish', True),) if ci % 3 == 0 else ()):
        what = 'dw %s k%d s%d %dx%dx%d b%d %s' % (dt, k, s, h, w, c, b, act)
        got, ref, _, name = _run_exact(dev, dt, k, s, b, h, w, c, act, wide=wide)
        assert name == G.dw_name(dt, inst), (what, name)
        _check_map(got, ref, dt, act, what)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('which', ['big', 'below'])
def test_dw_kernel_big_branch(dev, dt, which):
    """dw_kernel<3,2,2,2>: the 2-row patches launch_depthwise_t picks from 2^21 lanes on - what the stride-2 maps of the workload run at
    bench batch.  129 x 131 -> 65 x 66 (odd Ho: the last row pair is half beyond the map; 'SAME' pads bottom / right only), three
    channel vectors with a tail, the smallest batch that reaches the threshold - and the batch below it, which must stay on
    <3,2,2,1>.  The batch repeats five distinct images round robin, so the reference stays five images."""
    rt = _rt()
    did = rt.dtype_id(dt)
    V = rt.VEC[did]
    h, w = G.DW_BIG_HW
    c = G.DW_BIG_C[dt]
    big, below = G.dw_big_batches()
    b = big if which == 'big' else below
    inst = G.dw_instance(3, 2, b, h, w, c, V)
    assert inst == ((3, 2, 2, 2) if which == 'big' else (3, 2, 2, 1))
    act = 'none' if which == 'big' else 'relu6'
    x, wk, scale, shift, ref = _exact_case(3, 2, G.DW_BIG_DISTINCT, h, w, c, act)
    idx = torch.arange(b, device=dev) % G.DW_BIG_DISTINCT
    xd = _to_dev(x, dev, dt, round_up(c, V))[idx].contiguous()
    assert xd.numel() * xd.element_size() <= G.MAX_BYTES_BIG
    out, _, name = _launch(dev, dt, xd, c, _params(dev, dt, wk, scale, shift), 3, 2, act, b, wide_out=True)
    assert name == G.dw_name(dt, inst), name
    want = torch.from_numpy(ref.copy()).to(dev)[idx]               # float64: holds every element type's values (a copy: `ref` is read-only)
    got = out[..., :c].double()
    bad = got != want                                              # (NaN != anything: an unwritten element shows)
    assert not bad.any(), 'dw_kernel<%d,%d,%d,%d> %s: %d elements differ, first at %s' % (inst + (dt, int(bad.sum()), tuple(bad.nonzero()[0].tolist())))


# ------------------------------------------------------------------------------------------------ 3. dw_kernel's squeeze-excite form
@pytest.mark.parametrize('dt,k,s,h,w,c,b', G.DW_SE_CASES, ids=['%s-k%d-s%d-%dx%dx%d-b%d' % v for v in G.DW_SE_CASES])
def test_dw_kernel_se_form_sums(dev, dt, k, s, h, w, c, b):
    """dw_kernel<K,S,XT,1,T,1>: all channel vectors of a strip in one workgroup (cw = C4, dividing 256 or not: the last lanes idle)
    and 32-vector blocks shared out over several workgroups with a ragged last block.  The map equals the exact result, no row of
    sums is left unwritten, and the rows of an image add up to exactly the sum of its stored values."""
    rt = _rt()
    vec = rt.VEC[rt.dtype_id(dt)]
    ho, wo = -(-h // s), -(-w // s)
    xt = 4 if s == 1 else 2
    cw, ncb, rows = G.dw_se_geometry(ho * -(-wo // xt), -(-c // vec))
    act = 'relu6' if k == 3 else 'none'
    what = 'dw se %s k%d s%d %dx%dx%d cw=%d ncb=%d rows=%d' % (dt, k, s, h, w, c, cw, ncb, rows)
    got, ref, part, name = _run_exact(dev, dt, k, s, b, h, w, c, act, se_rows=rows, wide=bool(k == 5))
    assert name == G.dw_name(dt, (k, s, xt, 1), se=True), (what, name)
    _check_map(got, ref, dt, act, what)
    sums = part.cpu().numpy()[..., :c].astype(np.float64)
    assert np.isfinite(sums).all(), '%s: a row of sums was left unwritten' % what
    assert np.array_equal(sums.sum(axis=1), got.sum(axis=(1, 2))), what
