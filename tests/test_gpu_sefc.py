"""The inference squeeze-excite ops on the device - SE_MEAN and SE_FC of yoloret_amd/csrc/elementwise.hip, in the three forms SE_FC
takes its input (a pooled vector, a map it pools itself, rows of partial channel sums), whose FC pair and row pooling are
yr_se_fc_pair<1024> and yr_se_mean_rows<1024, false> of yoloret_amd/csrc/se_tail.h - against tests/sefc_ref.py, at the edges of
their geometry: the case lists are tests/sefc_ref.py's, and tests/test_sefc_host.py holds what each list must reach.

Every launch runs through tests/fence.run_op (guards around every tensor, two alignments), outputs are pre-filled with NaN, the pad
columns of every input row and the pad rows and columns of the packed FC parameters are NaN, the batch is three different images,
and the columns an op may not write (SE_MEAN: those from 4 ceil(C / 4) on) must keep their bits; SE_FC writes its whole row, +0 from
column C on.  Every case asserts that the device equals the float32 restatement in the device's documented order bit for bit, and that
max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the same figure of that restatement; the figures are printed before they
assert (run with -s).

The cases the work was specified with name C = 33 and C = 75 for "a shorter last FC1 segment"; by the kernel's own rule (one segment per
16 inputs, ceil(C / segments) inputs each) those cut into 3 x 11 and 5 x 15, equal segments whose length is no multiple of the batch of
8.  They stay for that; C = 35 (12 + 12 + 11) and C = 77 (4 x 16 + 13) are the short last segments, and a kernel that drops the clamp of a
segment's end to C passes 33 and 75 and fails 35 and 77 (tried once on the device).

Measured on an MI355X over the 242 figures of the file (126 SE_MEAN, 40 pooled vector, 42 map, 34 partial-sum rows): the device equals the
restatement bit for bit in every case, so device = E_ref in every figure: median 8.9e-08, none above 1e-06; the largest is the pooled
vector at C 4100, R 4, 9.7e-07 for device and restatement alike against a bar of 3.9e-06.  At the shipped widths: 512 / 128 3.0e-07
(bar 1.3e-06), 1152 / 48 4.4e-07 (bar 1.8e-06), 2304 / 96 5.2e-07 (bar 2.1e-06).  No kernel was changed: the never-run paths (second j0,
q0 and c0 passes, the empty last segment, PL = 1 and 2) returned the restatement's bits at the first run."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fence, sefc_ref as ref
from tests.util import q16, round_up, to_dev, to_dev16

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
YR_ERR_ARG = -1
F32 = np.float32
NAN_BITS = np.float32(np.nan).view(np.uint32)
B = ref.BATCH
DTYPES = ['f32', 'bf16', 'f16']
VEC = {'f32': 4, 'bf16': 8, 'f16': 8}          # elements of 16 bytes: the granule of a map's ld
WIDER = 8                                      # what a wider row adds to its ld (a multiple of every granule)


def _rt():
    from yoloret_amd import runtime
    return runtime


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    d = _bits(got) != _bits(want)
    assert not d.any(), '%s: %d of %d differ, first at %s: device %r, restatement %r' % (
        what, d.sum(), d.size, np.argwhere(d)[0], got[tuple(np.argwhere(d)[0])], want[tuple(np.argwhere(d)[0])])


def _within_bar(what, got, r32, r64, bad):
    e_dev, e_ref = ref.rel_err(got, r64), ref.rel_err(r32, r64)
    print('sefc %s: device %.3e, float32 restatement %.3e, bar %.3e' % (what, e_dev, e_ref, 4 * e_ref + EPS24))
    if not e_dev <= 4 * e_ref + EPS24:
        bad.append((what, e_dev, e_ref))


def _values(x, dt):
    """what the device sees of float32 data stored as dt"""
    return np.ascontiguousarray(x, F32) if dt == 'f32' else q16(x, dt)


def _rows_dev(x, dev, dt, wide):
    """x [B, n, C] (representable in dt) -> device tensor [B, n, 1, ld] of dt, pad columns NaN"""
    b, n, c = x.shape
    ld = round_up(c, VEC[dt]) + (WIDER if wide else 0)
    x = x.reshape(b, n, 1, c)
    return to_dev(x, dev, ld) if dt == 'f32' else to_dev16(x, dev, dt, ld)


def _nan_out(dev, ld, b=B):
    return torch.full((b, ld), float('nan'), dtype=torch.float32, device=dev)


_params = {}


def _fc_params(dev, c, r):
    """(w1, b1, w2, b2) and their packed device tensors, once per (C, R) and left unchanged"""
    if (c, r) not in _params:
        host = ref.fc_params(c, r)
        for a in host:
            a.setflags(write=False)
        _params[c, r] = host, [torch.from_numpy(a).to(dev) for a in ref.pack_params(*host)]
    return _params[c, r]


# ----------------------------------------------------------------------------- the two ops, fenced
def dev_mean(dev, x, dt, wide_in, out_ld):
    """SE_MEAN of x [B, HW, C] stored as dt -> [B, out_ld] float32 as the device left it (NaN where it wrote nothing)"""
    rt = _rt()
    b, hw, c = x.shape
    xd = _rows_dev(x, dev, dt, wide_in)
    out = _nan_out(dev, out_ld, b)
    op = rt.new_op(rt.OP_SE_MEAN)
    op.dtype, op.out_dtype = rt.dtype_id(dt), 0
    op.h = op.w = 1
    op.cin = op.cout = c
    op.nsrc = 1
    op.src[0] = rt.make_src(xd, c=c)
    op.out, op.out_ld = out.data_ptr(), out_ld
    fence.run_op(op, b, writes=[out], reads=[xd], cols=round_up(c, 4))
    return out.cpu().numpy()


def fc_op(src, c, r, keep, gate, dt='f32', k=0):
    rt = _rt()
    op = rt.new_op(rt.OP_SE_FC)
    op.dtype, op.out_dtype = rt.dtype_id(dt), 0
    op.h = op.w = 1
    op.cin = op.cout = c
    op.se_reduced, op.nsrc, op.k = r, 1, k
    op.src[0] = rt.make_src(src, c=c)
    op.wgt, op.b1, op.wgt2, op.b2 = [t.data_ptr() for t in keep]
    op.out, op.out_ld = gate.data_ptr(), gate.shape[1]
    return op


def dev_fc(dev, src, c, r, ld_gate, dt='f32', k=0):
    """SE_FC on src [B, n, 1, ld]: n == 1 and k == 0 a pooled vector, n > 1 a map of dt to pool, k > 0 rows of partial sums of k
    pixels -> [B, ld_gate]"""
    _, keep = _fc_params(dev, c, r)
    gate = _nan_out(dev, ld_gate, src.shape[0])
    fence.run_op(fc_op(src, c, r, keep, gate, dt, k), src.shape[0], writes=[gate], reads=[src] + keep)
    return gate.cpu().numpy()


def _check_gate(what, got, c, g32, g64, bad):
    _same_bits(got[:, :c], g32, 'the gate in the device\'s order, ' + what)
    assert not _bits(got[:, c:]).any(), 'columns from C on are +0, ' + what
    _within_bar(what, got[:, :c], g32, g64, bad)


def _gate_lds(c):
    return sorted({round_up(c, 4), round_up(c, 8)})


# ----------------------------------------------------------------------------- SE_MEAN
@pytest.mark.parametrize('dt', DTYPES)
def test_se_mean(dev, dt):
    """every HW x C of the lists; the input row and the output row are the narrowest and a wider one in turn"""
    bad = []
    for n, (hw, c) in enumerate((hw, c) for hw in ref.MEAN_HW for c in ref.MEAN_C):
        x = _values(ref.maps(B, hw, c), dt)
        ldc = round_up(c, 4)
        out_ld = ldc + (WIDER if (n + n // len(ref.MEAN_C)) % 2 else 0)
        what = 'SE_MEAN %s HW=%d C=%d out_ld=%d' % (dt, hw, c, out_ld)
        got = dev_mean(dev, x, dt, n % 3 == 1, out_ld)
        m32 = ref.mean_op32(x)
        _same_bits(got[:, :c], m32, 'the mean in the device\'s order, ' + what)
        assert not _bits(got[:, c:ldc]).any(), 'the pad lanes of the last quad are +0, ' + what
        assert np.all(_bits(got[:, ldc:]) == NAN_BITS), what
        _within_bar(what, got[:, :c], m32, ref.mean64(x), bad)
    assert not bad, bad


# ----------------------------------------------------------------------------- SE_FC on a pooled vector
@pytest.mark.parametrize('c,r', ref.FC_CASES, ids=['C%d-R%d' % cr for cr in ref.FC_CASES])
def test_se_fc_pooled_vector(dev, c, r):
    """gate rows of round_up(C, 4) and of round_up(C, 8) floats; the pooled vector in rows of round_up(C, 4) floats and wider ones"""
    (w1, b1, w2, b2), _ = _fc_params(dev, c, r)
    mean = ref.maps(B, 1, c, seed=1)
    g32, g64 = ref.fc_pair32(mean[:, 0], w1, b1, w2, b2), ref.fc_pair64(mean[:, 0], w1, b1, w2, b2)
    bad = []
    for n, ld_gate in enumerate(_gate_lds(c)):
        src = _rows_dev(mean, dev, 'f32', (n + c) % 2 == 1)
        what = 'pooled vector C=%d R=%d ld=%d ld_gate=%d' % (c, r, src.shape[3], ld_gate)
        _check_gate(what, dev_fc(dev, src, c, r, ld_gate), c, g32, g64, bad)
    assert not bad, bad


# ----------------------------------------------------------------------------- SE_FC pooling a map
@pytest.mark.parametrize('dt', DTYPES)
def test_se_fc_pools_a_map(dev, dt):
    bad = []
    for c, r, hw, wide in ref.MAP_CASES:
        (w1, b1, w2, b2), _ = _fc_params(dev, c, r)
        x = _values(ref.maps(B, hw, c, seed=2), dt)
        src = _rows_dev(x, dev, dt, wide)
        what = 'map %s C=%d R=%d HW=%d ld=%d PL=%d' % (dt, c, r, hw, src.shape[3], ref.map_split(c)['PL'])
        got = dev_fc(dev, src, c, r, _gate_lds(c)[-1], dt)
        _check_gate(what, got, c, ref.fc_pair32(ref.mean_map32(x), w1, b1, w2, b2), ref.fc_pair64(ref.mean64(x), w1, b1, w2, b2), bad)
    assert not bad, bad


# ----------------------------------------------------------------------------- SE_FC on rows of partial sums
ROWS_C = sorted({case[0] for case in ref.ROWS_CASES})


@pytest.mark.parametrize('c', ROWS_C)
def test_se_fc_partial_sum_rows(dev, c):
    """op.k is the true pixel count (4 rows + 3), not the row count; the plan's dtype does not matter (the rows are float32)"""
    bad = []
    for n, (_, r, rows, wide) in enumerate(case for case in ref.ROWS_CASES if case[0] == c):
        (w1, b1, w2, b2), _ = _fc_params(dev, c, r)
        x = ref.maps(B, rows, c, seed=3) * F32(4)
        k = ref.rows_pixels(rows)
        src = _rows_dev(x, dev, 'f32', wide)
        what = 'rows C=%d R=%d rows=%d k=%d ld=%d' % (c, r, rows, k, src.shape[3])
        got = dev_fc(dev, src, c, r, _gate_lds(c)[n % len(_gate_lds(c))], DTYPES[n % 3], k)
        _check_gate(what, got, c, ref.fc_pair32(ref.mean_rows32(x, k), w1, b1, w2, b2), ref.fc_pair64(ref.mean64(x, k), w1, b1, w2, b2), bad)
    assert not bad, bad


# ----------------------------------------------------------------------------- an image alone
def test_an_image_alone_equals_its_slice_of_the_batch(dev):
    """image 1 of 3 alone gives the bits of its slice: SE_MEAN, and SE_FC in each of its three forms"""
    x = ref.maps(B, 169, 75, seed=4)
    for dt in DTYPES:
        v = _values(x, dt)
        _same_bits(dev_mean(dev, v[1:2], dt, True, 76), dev_mean(dev, v, dt, True, 76)[1:2], 'SE_MEAN ' + dt)
        _same_bits(dev_fc(dev, _rows_dev(v[1:2], dev, dt, True), 75, 5, 80, dt), dev_fc(dev, _rows_dev(v, dev, dt, True), 75, 5, 80, dt)[1:2], 'map ' + dt)
    for c, r, n in ((75, 5, 1), (520, 128, 1)):
        v = ref.maps(B, n, c, seed=5)
        _same_bits(dev_fc(dev, _rows_dev(v[1:2], dev, 'f32', True), c, r, round_up(c, 8)), dev_fc(dev, _rows_dev(v, dev, 'f32', True), c, r, round_up(c, 8))[1:2],
                   'pooled vector C=%d' % c)
    for c, r, n in ((64, 8, 17), (1030, 4, 130)):
        v = ref.maps(B, n, c, seed=6)
        k = ref.rows_pixels(n)
        _same_bits(dev_fc(dev, _rows_dev(v[1:2], dev, 'f32', True), c, r, round_up(c, 8), k=k),
                   dev_fc(dev, _rows_dev(v, dev, 'f32', True), c, r, round_up(c, 8), k=k)[1:2], 'rows C=%d' % c)


# ----------------------------------------------------------------------------- refusals
def _refused(dev, op, gate, reads, what, b=2):
    """the launch returns YR_ERR_ARG with a message in both variants of the fence and writes nothing"""
    rt = _rt()
    L = rt.lib()
    seen = []

    def launch(op, batch):
        with torch.cuda.device(dev):
            seen.append((L.yr_op_run(ctypes.byref(op), int(batch), rt.stream_ptr(dev)), L.yr_last_error()))
    fence.run_op(op, b, writes=[gate], reads=reads, launch=launch)
    torch.cuda.synchronize()
    assert len(seen) == len(fence.VARIANTS) and all(rc == YR_ERR_ARG and b'se_fc' in msg for rc, msg in seen), (what, seen)
    assert np.all(_bits(gate.cpu().numpy()) == NAN_BITS), what


def test_refusals_change_nothing(dev):
    b, c, r = 2, 8, 2
    _, keep = _fc_params(dev, c, r)
    vec = torch.zeros((b, 1, 1, c), dtype=torch.float32, device=dev)
    rows = torch.zeros((b, 5, 1, c), dtype=torch.float32, device=dev)

    def gate(ld=c):
        return _nan_out(dev, ld, b)

    def case(what, src=vec, dt='f32', k=0, ld=c, keep=keep, reads=None, **fields):
        g = gate(ld)
        op = fc_op(src, c, r, keep, g, dt, k)
        for f, v in fields.items():
            setattr(op, f, v)
        _refused(dev, op, g, [src] + list(keep if reads is None else reads), what)

    case('in.c != cout', cout=c + 4)
    case('in.c != cout, rows', src=rows, k=20, cout=c - 4)
    case('a 16-bit gate', out_dtype=1)
    case('se_reduced 0', se_reduced=0)
    case('out_ld below round_up(C, 4)', out_ld=c - 4)
    case('out_ld no multiple of 4', ld=c + 4, out_ld=c + 2)
    for i, name in enumerate(('wgt', 'b1', 'wgt2', 'b2')):          # each parameter 4 bytes past a 16-byte boundary
        longer = torch.zeros((keep[i].numel() + 4,), dtype=torch.float32, device=dev)
        moved = list(keep)
        moved[i] = longer
        case(name + ' 4 bytes off', reads=moved, **{name: longer.data_ptr() + 4})
    # a map to pool whose ld is no multiple of the type's vector width (4 floats, 8 16-bit elements)
    m32 = torch.zeros((b, 3, 1, c + 2), dtype=torch.float32, device=dev)
    g = gate()
    op = fc_op(m32, c, r, keep, g)
    op.src[0].c = c
    _refused(dev, op, g, [m32] + keep, 'float32 map of ld 10')
    for dt, tdt in (('bf16', torch.bfloat16), ('f16', torch.float16)):
        m16 = torch.zeros((b, 3, 1, c + 4), dtype=tdt, device=dev)
        g = gate()
        op = fc_op(m16, c, r, keep, g, dt)
        op.src[0].c = c
        _refused(dev, op, g, [m16] + keep, dt + ' map of ld 12')
    # more LDS than 64 KiB: the widths are one quad past what fits, for a vector / rows and (16 KiB less) for a map to pool
    for c2, r2, n, k in ((12288, 4, 1, 0), (12288, 4, 3, 15), (8192, 4, 2, 0)):
        pool = 2 if k else 1 if n > 1 else 0
        assert ref.lds_bytes(c2, r2, pool) > ref.LDS_LIMIT >= ref.lds_bytes(c2 - 4, r2, pool) and (pool != 1 or ref.lds_bytes(c2, r2, 0) <= ref.LDS_LIMIT)
        _, keep2 = _fc_params(dev, c2, r2)
        src = torch.zeros((b, n, 1, c2), dtype=torch.float32, device=dev)
        g = gate(c2)
        _refused(dev, fc_op(src, c2, r2, keep2, g, 'f32', k), g, [src] + keep2, 'LDS: C=%d R=%d pool=%d' % (c2, r2, pool))
