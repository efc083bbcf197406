"""The definition of the inference squeeze-excite ops - SE_MEAN and SE_FC of yoloret_amd/csrc/elementwise.hip, whose FC pair and
partial-sum pooling are yr_se_fc_pair<1024> and yr_se_mean_rows<1024, false> of yoloret_amd/csrc/se_tail.h (reference
yolo3/efficientnet.py:406-438: Mean over H, W -> 1x1 + bias -> Swish -> 1x1 + bias -> sigmoid) - written from the prose of those two
files, not from the kernels.

* ``fma32``: fmaf in NumPy.  The product of two float32 values is exact in float64; the addend is added with a TwoSum residual, and
  where that residual is not zero and the float64 sum's last mantissa bit is even the sum moves one float64 ulp toward the residual
  (round to odd: 53 >= 24 + 2 bits, so the cast to float32 rounds as one rounding of the exact value would).  The plain
  float32(float64(a) * b + c) rounds twice and differs on float32 ties (tests/test_sefc_host.py compares both with libm's fmaf).
* the geometry the launches derive from (C, R), the row count and the map size: ``segments``, ``fc1_split``, ``fc2_split``,
  ``rows_split``, ``map_split``, ``lds_bytes``.  The case lists at the end are built for classes of that geometry, and
  tests/test_sefc_host.py checks through these functions that every class is still in them.
* float32 restatements in the device's documented order - what the device must return bit for bit on arbitrary data, and whose
  deviation from float64 is E_ref in  max |device - ref64| / max |ref64| <= 4 E_ref + 2^-24  (tests/test_gpu_sefc.py):
    ``mean_op32``    SE_MEAN: 64 pixel lanes, lane pl adds pixels pl, pl + 64, ... in order from +0; lanes 8 g .. 8 g + 7 are added in
                     order from lane 8 g's own sum, the 8 group sums in order from group 0's own, then / float(HW);
    ``mean_map32``   SE_FC pooling a map: PL = 1024 / c4p pixel lanes (c4p: the power of two >= ceil(C / 4), 1024 at most), lane pl adds
                     pixels pl, pl + PL, ...; the lanes are added in order from lane 0's own sum, then / float(HW);
    ``mean_rows32``  SE_FC on rows of partial sums: per pass of <= 1024 channels the rows are cut into nrs segments of rps rows, a
                     segment is added in row order from +0, the segments in order from segment 0's own sum, then / count;
    ``fc_pair32``    each stage cuts its inputs into segments; a segment is an fmaf chain from +0 in input order; bias + the segments in
                     segment order with plain float32 adds (an empty segment adds +0); swish (hidden units) and sigmoid (gate) are the
                     library's pinned ones (tests/segrad_ref.sigmoid32 / swish32).
  16-bit maps enter as their widened float32 values.
* float64 versions of the same formulas (``mean64``, ``fc_pair64``)."""
import numpy as np

from tests.convgrad_ref import rel_err      # noqa: F401  (shared helper: nothing mutable)
from tests.segrad_ref import sigmoid32, swish32

F32 = np.float32
SE_FC_THREADS = 1024          # lanes of se_fc_kernel's workgroup                       } tests/test_sefc_host.py reads all of these
SE_MEAN_PL = 64               # pixel lanes of se_mean_kernel                            } in the two source files
SE_MEAN_QUADS = 16            # channel quads of one se_mean_kernel workgroup
FC_BATCH, ROWS_BATCH = 8, 16  # weight rows / partial-sum rows loaded together, the tail of a segment clamped to its last row
LDS_LIMIT = 64 * 1024


def round_up(v, m):
    return (v + m - 1) // m * m


# ----------------------------------------------------------------------------- fmaf
def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, element by element (broadcasting), as fmaf gives it"""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * b                                    # exact: 48 bits
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)                # TwoSum: p + c == s + err exactly
        s = np.asarray(s)
        even = (s.view(np.int64) & 1) == 0
        fix = (err != 0) & even & np.isfinite(s)
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(F32)


def fma32_plain(a, b, c):
    """two roundings: what fma32 must NOT be (kept for tests/test_sefc_host.py, which shows the difference)"""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    return (a * b + c).astype(F32)


# ----------------------------------------------------------------------------- geometry
def segments(n, most):
    """segments a stage cuts n inputs into: as many as give a lane two batches of 8 (one per 16 inputs), 1 at least, `most` at most"""
    return max(1, min((n + 15) // 16, most))


def seg_ranges(n, nseg, per):
    """[(a, b)] of the nseg segments of `per` inputs over n: b is clamped to n, so a trailing segment may be short, empty (a == b) or
    begin past the end (a > b)"""
    return [(s * per, min(s * per + per, n)) for s in range(nseg)]


def _stage_split(n_in, n_out, first, count, per):
    quads = round_up(n_out, 4) // 4
    out = []
    for q0 in range(0, quads, SE_FC_THREADS):
        qn = min(quads - q0, SE_FC_THREADS)
        nseg = segments(n_in, SE_FC_THREADS // qn)
        out.append({first: q0, count: qn, 'nseg': nseg, per: -(-n_in // nseg)})
    return out


def fc1_split(c, r):
    """FC1 (C inputs, R outputs): per outer pass of <= 1024 quads of hidden units {j0, jq, nseg, cps}"""
    return _stage_split(c, r, 'j0', 'jq', 'cps')


def fc2_split(c, r):
    """FC2 (R inputs, C outputs): per outer pass of <= 1024 channel quads {q0, qp, nseg, jps}"""
    return _stage_split(r, c, 'q0', 'qp', 'jps')


def rows_split(rows, c):
    """yr_se_mean_rows<1024>: per pass of <= 1024 of the round_up(C, 4) channels {c0, cn, nrs, rps}"""
    ldc = round_up(c, 4)
    out = []
    for c0 in range(0, ldc, SE_FC_THREADS):
        cn = min(ldc - c0, SE_FC_THREADS)
        nrs = SE_FC_THREADS // cn
        out.append({'c0': c0, 'cn': cn, 'nrs': nrs, 'rps': -(-rows // nrs)})
    return out


def map_split(c):
    """SE_FC pooling a map: {c4p, PL, passes (the first quad of each)}"""
    c4 = -(-c // 4)
    c4p = 1
    while c4p < c4 and c4p < SE_FC_THREADS:
        c4p *= 2
    return {'c4p': c4p, 'PL': SE_FC_THREADS // c4p, 'passes': list(range(0, c4, c4p))}


def lds_bytes(c, r, pool):
    """dynamic LDS of an SE_FC launch: mean | hidden | 1024 partial quads, and 1024 more quads where a map is pooled (pool == 1)"""
    floats = round_up(round_up(c, 4) + round_up(r, 4) + 4 * SE_FC_THREADS, 4)
    return 4 * floats + (16 * SE_FC_THREADS if pool == 1 else 0)


# ----------------------------------------------------------------------------- float32, the device's order
def _seq(rows):
    """[n, ...] -> [...]: added one after the other from +0 (n == 0: +0)"""
    s = np.zeros(rows.shape[1:], F32)
    for row in rows:
        s = s + row
    return s


def _from_first(terms):
    """[n, ...] -> [...]: added in order, the first term its own"""
    s = terms[0].copy()
    for t in terms[1:]:
        s = s + t
    return s


def _lanes(x, nl):
    """x [B, HW, C] -> [nl, B, C]: lane l adds pixels l, l + nl, ... in order from +0"""
    b, hw, c = x.shape
    steps = -(-hw // nl)
    pad = np.zeros((b, steps * nl, c), F32)          # (a lane's sum starts at +0 and adding +0 changes no bit of it)
    pad[:, :hw] = x
    return _seq(pad.reshape(b, steps, nl, c).transpose(1, 2, 0, 3))


def mean_op32(x):
    """SE_MEAN: x [B, HW, C] float32 (widened) -> [B, C]"""
    x = np.ascontiguousarray(x, F32)
    lanes = _lanes(x, SE_MEAN_PL)
    groups = np.stack([_from_first(lanes[8 * g:8 * g + 8]) for g in range(SE_MEAN_PL // 8)])
    out = _from_first(groups) / F32(x.shape[1])
    assert out.dtype == F32
    return out


def mean_map32(x):
    """SE_FC pooling a map (pool == 1): x [B, HW, C] float32 (widened) -> [B, C]"""
    x = np.ascontiguousarray(x, F32)
    out = _from_first(_lanes(x, map_split(x.shape[2])['PL'])) / F32(x.shape[1])
    assert out.dtype == F32
    return out


def mean_rows32(rows, count):
    """SE_FC on partial-sum rows (pool == 2): rows [B, n, C] float32, count the true pixel count -> [B, C]"""
    rows = np.ascontiguousarray(rows, F32)
    b, n, c = rows.shape
    out = np.empty((b, c), F32)
    for p in rows_split(n, c):
        lo, hi = p['c0'], min(p['c0'] + p['cn'], c)
        segs = [_seq(rows[:, ra:rb, lo:hi].transpose(1, 0, 2)) for ra, rb in seg_ranges(n, p['nrs'], p['rps'])]
        out[:, lo:hi] = _from_first(segs) / F32(count)
    return out


def _chain32(x, w):
    """x [B, n], w [n, O] -> [B, O]: s = fmaf(w[i], x[i], s) for i in order from +0"""
    s = np.zeros((x.shape[0], w.shape[1]), F32)
    for i in range(x.shape[1]):
        s = fma32(w[i][None, :], x[:, i:i + 1], s)
    return s


def _stage32(x, w, bias, passes, first, count, per):
    n_in, n_out = w.shape
    out = np.empty((x.shape[0], n_out), F32)
    for p in passes:
        lo, hi = 4 * p[first], min(4 * (p[first] + p[count]), n_out)
        v = np.broadcast_to(bias[lo:hi], (x.shape[0], hi - lo)).astype(F32)
        for a, b in seg_ranges(n_in, p['nseg'], p[per]):
            v = v + _chain32(x[:, a:b], w[a:b, lo:hi])
        out[:, lo:hi] = v
    assert out.dtype == F32
    return out


def fc_pair32(mean, w1, b1, w2, b2):
    """mean [B, C], w1 [C, R], b1 [R], w2 [R, C], b2 [C] -> the gate [B, C] (what follows it in a row, pad lanes, is +0)"""
    mean, w1, b1, w2, b2 = (np.ascontiguousarray(a, F32) for a in (mean, w1, b1, w2, b2))
    c, r = w1.shape
    hid = swish32(_stage32(mean, w1, b1, fc1_split(c, r), 'j0', 'jq', 'cps'))
    return sigmoid32(_stage32(hid, w2, b2, fc2_split(c, r), 'q0', 'qp', 'jps'))


# ----------------------------------------------------------------------------- float64 by the same formulas
def mean64(x, count=None):
    x = np.asarray(x, np.float64)
    return x.sum(axis=1) / (x.shape[1] if count is None else count)


def _sig64(u):
    return 1.0 / (1.0 + np.exp(-u))


def fc_pair64(mean, w1, b1, w2, b2):
    mean, w1, b1, w2, b2 = (np.asarray(a, np.float64) for a in (mean, w1, b1, w2, b2))
    z1 = b1 + mean @ w1
    return _sig64(b2 + (z1 * _sig64(z1)) @ w2)


# ----------------------------------------------------------------------------- data
def fc_params(c, r, seed=0):
    """-> (w1 [C, R], b1 [R], w2 [R, C], b2 [C]) float32, scaled like trained kernels (1 / sqrt(fan-in))"""
    rng = np.random.default_rng(1000003 * seed + 7919 * c + 131 * r)
    w1 = (rng.standard_normal((c, r)) / np.sqrt(c)).astype(F32) * F32(2)
    w2 = (rng.standard_normal((r, c)) / np.sqrt(r)).astype(F32) * F32(2)
    return w1, rng.uniform(-1, 1, r).astype(F32), w2, rng.uniform(-1, 1, c).astype(F32)


def pack_params(w1, b1, w2, b2, fill=np.nan):
    """-> W1 [ldc][R4], b1 [R4], W2 [R][ldc], b2 [ldc] as the op takes them (include/yoloret_hip.h), pad rows and columns `fill`: no
    output may depend on them"""
    c, r = w1.shape
    ldc, r4 = round_up(c, 4), round_up(r, 4)
    out = [np.full(s, fill, F32) for s in ((ldc, r4), (r4,), (r, ldc), (ldc,))]
    out[0][:c, :r], out[1][:r], out[2][:, :c], out[3][:c] = w1, b1, w2, b2
    return out


def maps(b, hw, c, seed=0):
    """[B, HW, C] float32: normals around a per-channel offset, three different images"""
    rng = np.random.default_rng(1000003 * seed + 7919 * c + 17 * hw + 100000 * b)
    return (rng.uniform(-.5, .5, (1, 1, c)) + rng.standard_normal((b, hw, c))).astype(F32)


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_sefc.py
BATCH = 3
MEAN_HW = [1, 63, 64, 65, 169, 600]          # 600 > 512: the lanes of an 8-group hold 9 or 10 pixels each
MEAN_C = [1, 3, 4, 61, 64, 75, 260]          # C % 4 != 0; ceil(C / 4) no multiple of 16; more than one workgroup along x

# SE_FC on a pooled vector: (C, R).  What each is for is what tests/test_sefc_host.py asks of the list.
FC_SHIPPED = [(512, 128), (32, 8), (96, 4), (144, 6), (240, 10), (480, 20), (672, 28), (1152, 48), (1392, 58), (2304, 96)]
FC_CASES = FC_SHIPPED + [
    (16, 4), (5, 1), (16, 2), (13, 6),       # one FC1 segment; R in {1, 2, 4, 6}: the pad lanes of a quad of hidden units
    (64, 16),                                # several equal FC1 segments
    (33, 8), (75, 5),                        # cps = 11, 15: no multiple of 8 (3 x 11 and 5 x 15: the segments are equal)
    (35, 8), (77, 8),                        # a shorter last FC1 segment: 12 + 12 + 11, 4 x 16 + 13
    (520, 128),                              # an empty last FC1 segment: 32 of 17, 31 x 17 = 527
    (48, 12),                                # jq = 3 does not divide 1024: lane 1023 idles
    (8, 4100),                               # a second j0 pass of one quad
    (16, 64), (16, 35),                      # FC2: several equal segments; a shorter last one
    (512, 130),                              # FC2: the cap 1024 / qp = 8, segments of 17
    (128, 520),                              # FC2: an empty last segment
    (12, 48),                                # qp = 3
    (1, 4), (2, 4), (3, 1), (6, 8),          # C in {1, 2, 3, 6}: the pad lanes of a channel quad
    (4100, 4),                               # a second q0 pass with a single quad in it
]

# SE_FC pooling a map: (C, R, HW, map ld wider than the type's round-up of C)
def _map_cases():
    out = []
    for c, r in ((64, 8), (75, 5)):
        pl = map_split(c)['PL']
        out += [(c, r, hw, n % 2 == 1) for n, hw in enumerate((2, pl - 1, pl, pl + 1, 3 * pl + 1))]
    out += [(1152, 48, 2, False), (1152, 48, 3, True), (1152, 48, 7, False)]          # c4p = 512, PL = 2 (PL - 1 = 1 pixel is no map)
    out += [(4100, 4, 3, False)]                                                      # a second q0 pass, PL = 1
    return out


MAP_CASES = _map_cases()

# SE_FC on partial-sum rows: (C, R, rows, row ld wider than round_up(C, 4)); op.k = rows_pixels(rows)
def _rows_cases():
    out = []
    for c, r in ((64, 8), (75, 5), (200, 10)):
        nrs = rows_split(1, c)[0]['nrs']
        for n, rows in enumerate(sorted({1, 15, 16, 17, nrs - 1, nrs, nrs + 1, 5 * nrs + 3})):
            out.append((c, r, rows, n % 2 == 1))
    out += [(200, 10, 100, True)]                                                     # rps = 20: a batch of 16 and a clamped tail of 4
    out += [(1030, 4, rows, rows % 2 == 0) for rows in (1, 17, 127, 128, 129, 130)]   # passes of 1024 and 8 channels: nrs = 1 and 128
    out += [(1392, 58, rows, rows % 2 == 0) for rows in (1, 2, 3, 35)]                # passes of 1024 and 368: nrs = 1 and 2
    out += [(2304, 96, 5, False), (2304, 96, 23, True)]                               # passes of 1024, 1024 and 256: nrs = 1, 1, 4
    return out


ROWS_CASES = _rows_cases()


def rows_pixels(rows):
    """the true pixel count a case divides by: not the row count"""
    return 4 * rows + 3
