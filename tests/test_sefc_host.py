"""Host side of the inference squeeze-excite ops (no GPU): tests/sefc_ref.py's fmaf against libm's, its float32 restatements against
literal lane-by-lane ones, against float64 and among themselves, the constants it restates against the two source files, and - through
its geometry functions - that the case lists of tests/test_gpu_sefc.py still hold every class of the geometry they were built for."""
import ctypes
import os
import re

import numpy as np

from tests import sefc_ref as ref
from tests.segrad_ref import sigmoid32

F32 = np.float32
U = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ----------------------------------------------------------------------------- fmaf
def _triples(n=400000):
    """half arbitrary, half products exactly on a float32 tie (13 x 12 odd mantissa bits: 25 significant bits when the product carries)
    with an addend far below the product's last float64 bit: fmaf rounds by the addend's sign, two roundings to even"""
    rng = np.random.default_rng(0)
    h = n // 2
    a = np.concatenate([rng.standard_normal(h), (rng.integers(2 ** 12, 2 ** 13, h) | 1) * 2.0 ** rng.integers(-20, 20, h)]).astype(F32)
    b = np.concatenate([rng.standard_normal(h), (rng.integers(2 ** 11, 2 ** 12, h) | 1) * 2.0 ** rng.integers(-20, 20, h)]).astype(F32)
    tiny = a[h:].astype(np.float64) * b[h:] * 2.0 ** -70 * rng.choice([-1.0, 1.0], h)
    c = np.concatenate([rng.standard_normal(h), tiny]).astype(F32)
    return a, b, c


def test_fma32_is_libm_fmaf():
    libm = ctypes.CDLL('libm.so.6')
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    a, b, c = _triples()
    want = np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], F32)
    assert int(np.sum(_bits(ref.fma32(a, b, c)) != _bits(want))) == 0
    # the triples tell one rounding from two: a definition by the plain float64 cast fails here
    plain = int(np.sum(_bits(ref.fma32_plain(a, b, c)) != _bits(want)))
    print('fma32: 0 of %d differ from libm; the plain float64 cast differs in %d' % (a.size, plain))
    assert plain > 10000
    # broadcasting, and a few by hand: 1 + 2^-24 is a tie of the sum itself
    assert ref.fma32(F32(1), F32(1), F32(2.0 ** -24)) == F32(1) and ref.fma32(F32(1 + 2.0 ** -23), F32(1), F32(2.0 ** -24)) == F32(1 + 2.0 ** -22)
    assert ref.fma32(np.ones((2, 1), F32), np.ones((1, 3), F32), F32(0)).shape == (2, 3)


# ----------------------------------------------------------------------------- the documented orders, literally
def _mean_op_literal(img):
    hw, c = img.shape
    lanes = np.zeros((64, c), F32)
    for i in range(hw):
        lanes[i % 64] = lanes[i % 64] + img[i]
    groups = []
    for g in range(8):
        t = lanes[8 * g].copy()
        for i in range(1, 8):
            t = t + lanes[8 * g + i]
        groups.append(t)
    t = groups[0]
    for g in groups[1:]:
        t = t + g
    return t / F32(hw)


def _mean_map_literal(img):
    hw, c = img.shape
    pl = ref.map_split(c)['PL']
    lanes = np.zeros((pl, c), F32)
    for i in range(hw):
        lanes[i % pl] = lanes[i % pl] + img[i]
    t = lanes[0].copy()
    for i in range(1, pl):
        t = t + lanes[i]
    return t / F32(hw)


def _mean_rows_literal(rows, count):
    n, c = rows.shape
    out = np.empty(c, F32)
    for ch in range(c):
        cn = min(ref.round_up(c, 4) - ch // 1024 * 1024, 1024)
        nrs = 1024 // cn
        rps = -(-n // nrs)
        m = None
        for seg in range(nrs):
            s = F32(0)
            for r in range(seg * rps, min(seg * rps + rps, n)):
                s = F32(s + rows[r, ch])
            m = s if m is None else F32(m + s)
        out[ch] = F32(m / F32(count))
    return out


def _stage_literal(x, w, bias):
    """one stage of the FC pair for one image: output o belongs to quad o // 4, pass (o // 4) // 1024"""
    n_in, n_out = w.shape
    quads = -(-n_out // 4)
    out = np.empty(n_out, F32)
    for o in range(n_out):
        qn = min(quads - (o // 4) // 1024 * 1024, 1024)
        nseg = ref.segments(n_in, 1024 // qn)
        per = -(-n_in // nseg)
        v = bias[o]
        for seg in range(nseg):
            s = F32(0)
            for i in range(seg * per, min(seg * per + per, n_in)):
                s = ref.fma32(w[i, o], x[i], s)
            v = F32(v + s)
        out[o] = v
    return out


def test_means_are_the_stated_orders():
    rng = np.random.default_rng(1)
    for hw, c in ((1, 1), (63, 3), (65, 5), (169, 4), (600, 2)):
        x = (1 + rng.standard_normal((2, hw, c))).astype(F32)
        for b in range(2):
            assert np.array_equal(_bits(ref.mean_op32(x)[b]), _bits(_mean_op_literal(x[b]))), ('SE_MEAN', hw, c)
    for hw, c in ((2, 64), (31, 75), (33, 75), (97, 75), (7, 1152), (3, 4100), (700, 5)):
        x = (1 + rng.standard_normal((2, hw, c))).astype(F32)
        for b in range(2):
            assert np.array_equal(_bits(ref.mean_map32(x)[b]), _bits(_mean_map_literal(x[b]))), ('map', hw, c)
    for n, c in ((1, 1), (17, 64), (83, 64), (14, 75), (100, 200), (35, 1030), (3, 1392)):
        rows = (1 + rng.standard_normal((2, n, c))).astype(F32)
        for b in range(2):
            assert np.array_equal(_bits(ref.mean_rows32(rows, 4 * n + 3)[b]), _bits(_mean_rows_literal(rows[b], 4 * n + 3))), ('rows', n, c)
    # 2^24 + 1 + 1 stays at 2^24 in one segment of rows; ones of other segments are added among themselves first
    rows = np.ones((1, 4, 1024), F32)
    rows[0, 0] = 2.0 ** 24
    assert ref.mean_rows32(rows, 1)[0, 0] == 2.0 ** 24          # 1024 channels: one segment of 4 rows
    assert ref.mean_rows32(rows[:, :, :512], 1)[0, 0] == 2.0 ** 24 + 2          # 512: two segments of 2 rows, (2^24 + 1) + (1 + 1)


def test_fc_pair_is_the_stated_order():
    rng = np.random.default_rng(2)
    for c, r in ((1, 1), (16, 4), (33, 8), (35, 6), (75, 5), (12, 48), (130, 35)):
        w1, b1, w2, b2 = ref.fc_params(c, r)
        mean = rng.standard_normal((2, c)).astype(F32)
        got = ref.fc_pair32(mean, w1, b1, w2, b2)
        for b in range(2):
            hid = _stage_literal(mean[b], w1, b1)
            hid = hid * sigmoid32(hid)
            assert np.array_equal(_bits(got[b]), _bits(sigmoid32(_stage_literal(hid, w2, b2)))), (c, r)


def test_restatements_agree_where_they_must():
    """one lane, one segment and one pass each reduce to a plain sequential chain"""
    rng = np.random.default_rng(3)
    x = (1 + rng.standard_normal((2, 9, 4100))).astype(F32)          # PL = 1: the pixels in order
    seq = x[:, 0].copy()
    for i in range(1, 9):
        seq = seq + x[:, i]
    assert np.array_equal(_bits(ref.mean_map32(x)), _bits(seq / F32(9)))
    rows = x[:, :, :600]                                             # 600 channels: nrs = 1, the rows in order; count = the row count
    assert np.array_equal(_bits(ref.mean_rows32(rows, 9)), _bits(seq[:, :600] / F32(9)))
    one = x[:, :1, :75]                                              # one pixel: every order returns it
    for f in (ref.mean_op32, ref.mean_map32, lambda v: ref.mean_rows32(v, 1)):
        assert np.array_equal(_bits(f(one)), _bits(one[:, 0]))
    # SE_MEAN and the map pooling of C = 64 (PL = 64) differ only in how the 64 lanes are combined: on integers they agree
    ints = rng.integers(-4, 5, (2, 169, 64)).astype(F32)
    assert np.array_equal(_bits(ref.mean_op32(ints)), _bits(ref.mean_map32(ints)))
    # C <= 16 and R <= 16: one segment a stage, the gate is bias + one fmaf chain
    c, r = 13, 6
    w1, b1, w2, b2 = ref.fc_params(c, r)
    mean = rng.standard_normal((2, c)).astype(F32)
    assert [p['nseg'] for p in ref.fc1_split(c, r) + ref.fc2_split(c, r)] == [1, 1]
    s = np.zeros((2, r), F32)
    for i in range(c):
        s = ref.fma32(w1[i][None], mean[:, i:i + 1], s)
    hid = b1 + s
    hid = hid * sigmoid32(hid)
    s = np.zeros((2, c), F32)
    for j in range(r):
        s = ref.fma32(w2[j][None], hid[:, j:j + 1], s)
    assert np.array_equal(_bits(ref.fc_pair32(mean, w1, b1, w2, b2)), _bits(sigmoid32(b2 + s)))


# ----------------------------------------------------------------------------- against float64
def test_pinned_sigmoid_is_within_four_ulps():
    """what the bound on the gate below takes for granted"""
    u = np.linspace(-20, 20, 4001).astype(F32)
    want = 1.0 / (1.0 + np.exp(-u.astype(np.float64)))
    assert np.max(np.abs(sigmoid32(u) - want) / want) <= 8 * U          # 4 ulp = 8 half-ulps


def _sum_bound(x, depth, count):
    """|float32 sum of `depth` dependent additions / count - exact| <= 1.01 (depth u sum |x| / count + u |mean|), against max |mean|"""
    x = np.abs(np.asarray(x, np.float64))
    m = np.abs(ref.mean64(x, count))          # (of |x|: at least |mean|)
    return 1.01 * U * (depth * x.sum(axis=1) / count + m)


def test_means_against_float64():
    for hw, c in ((1, 3), (65, 61), (169, 75), (600, 64)):
        x = ref.maps(3, hw, c)
        assert np.all(np.abs(ref.mean_op32(x) - ref.mean64(x)) <= _sum_bound(x, -(-hw // 64) + 14, hw)), ('SE_MEAN', hw, c)
    for hw, c in ((2, 64), (97, 75), (7, 1152), (3, 4100)):
        x = ref.maps(3, hw, c)
        pl = ref.map_split(c)['PL']
        assert np.all(np.abs(ref.mean_map32(x) - ref.mean64(x)) <= _sum_bound(x, -(-hw // pl) + pl - 1, hw)), ('map', hw, c)
    for n, c in ((17, 64), (68, 75), (100, 200), (130, 1030)):
        rows = ref.maps(3, n, c) * F32(4)
        k = ref.rows_pixels(n)
        depth = max(p['rps'] + p['nrs'] - 1 for p in ref.rows_split(n, c))
        assert np.all(np.abs(ref.mean_rows32(rows, k) - ref.mean64(rows, k)) <= _sum_bound(rows, depth, k)), ('rows', n, c)


def _gate_bound(mean, w1, b1, w2, b2):
    """first-order bound on |gate32 - gate64|, element by element: a stage is `cps + nseg` dependent roundings a unit over
    |bias| + sum |x| |w|; swish has slope <= 1.1 and costs the pinned sigmoid (4 ulp) and a product; the sigmoid has slope 1 / 4"""
    a = [np.abs(np.asarray(v, np.float64)) for v in (mean, w1, b1, w2, b2)]
    c, r = w1.shape
    d1 = max(p['cps'] + p['nseg'] for p in ref.fc1_split(c, r))
    d2 = max(p['jps'] + p['nseg'] for p in ref.fc2_split(c, r))
    z1 = np.asarray(b1, np.float64) + np.asarray(mean, np.float64) @ np.asarray(w1, np.float64)
    h = np.abs(z1 / (1.0 + np.exp(-z1)))
    dz1 = d1 * U * (a[2] + a[0] @ a[1])
    dh = 1.1 * dz1 + 5 * U * h
    dz2 = dh @ a[3] + d2 * U * (a[4] + h @ a[3])
    return 1.01 * (0.25 * dz2 + 4.5 * U)


def test_fc_pair_against_float64():
    for c, r in ((16, 4), (75, 5), (520, 128), (512, 130), (128, 520), (1152, 48)):
        w1, b1, w2, b2 = ref.fc_params(c, r)
        mean = ref.mean64(ref.maps(3, 5, c)).astype(F32)
        g32, g64 = ref.fc_pair32(mean, w1, b1, w2, b2), ref.fc_pair64(mean, w1, b1, w2, b2)
        assert np.all(np.abs(g32 - g64) <= _gate_bound(mean, w1, b1, w2, b2)), (c, r)
        assert ref.rel_err(g32, g64) < 1e-6, (c, r, ref.rel_err(g32, g64))


# ----------------------------------------------------------------------------- the constants, read where they are defined
def _csrc(name):
    from yoloret_amd import build
    return open(os.path.join(build.CSRC, name)).read()


def test_constants_are_those_of_the_sources():
    el, tail = _csrc('elementwise.hip'), _csrc('se_tail.h')
    assert int(re.search(r'#define SE_FC_THREADS (\d+)\s', el).group(1)) == ref.SE_FC_THREADS
    assert int(re.search(r'#define SE_MEAN_PL (\d+)\s', el).group(1)) == ref.SE_MEAN_PL
    assert re.search(r'float4 part\[SE_MEAN_PL\]\[(\d+)\]', el).group(1) == str(ref.SE_MEAN_QUADS)
    assert 'yr_se_fc_pair<SE_FC_THREADS>' in el and 'yr_se_mean_rows<SE_FC_THREADS, false>' in el
    # the batches: weight rows of a stage and partial-sum rows are loaded w8[8] / v[16] at a time
    assert set(re.findall(r'se_f4 w8\[(\d+)\];', tail)) == {str(ref.FC_BATCH)} and len(re.findall(r'se_f4 w8\[8\];', tail)) == 2
    assert re.findall(r'float v\[(\d+)\];', tail) == [str(ref.ROWS_BATCH)]
    assert re.search(r'const int want = \(n \+ 15\) >> 4;', tail)
    assert re.search(r'YR_REQUIRE\(lds <= 64 \* 1024,', el) and ref.LDS_LIMIT == 64 * 1024
    # LDS of the launches: yr_se_fc_floats and the extra quads of a pooled map
    assert ref.lds_bytes(512, 128, 0) == 4 * (512 + 128 + 4096) and ref.lds_bytes(75, 5, 1) == 4 * (76 + 8 + 4096) + 16384
    assert ref.lds_bytes(4100, 4, 1) == 49184 and ref.lds_bytes(8192, 4100, 0) > ref.LDS_LIMIT >= ref.lds_bytes(8192, 4096, 0)


# ----------------------------------------------------------------------------- what the case lists reach
def test_geometry_by_hand():
    assert [ref.segments(n, 1000) for n in (1, 16, 17, 32, 33, 2304)] == [1, 1, 2, 2, 3, 144] and ref.segments(2304, 42) == 42
    assert ref.fc1_split(512, 128) == [{'j0': 0, 'jq': 32, 'nseg': 32, 'cps': 16}]
    assert ref.fc2_split(512, 128) == [{'q0': 0, 'qp': 128, 'nseg': 8, 'jps': 16}]
    assert ref.fc1_split(520, 128)[0]['cps'] == 17 and ref.seg_ranges(520, 32, 17)[-1] == (527, 520)
    assert ref.fc1_split(2304, 96) == [{'j0': 0, 'jq': 24, 'nseg': 42, 'cps': 55}]
    assert ref.fc2_split(512, 130) == [{'q0': 0, 'qp': 128, 'nseg': 8, 'jps': 17}]
    assert [p['jq'] for p in ref.fc1_split(8, 4100)] == [1024, 1] and [p['qp'] for p in ref.fc2_split(4100, 4)] == [1024, 1]
    assert ref.rows_split(17, 64) == [{'c0': 0, 'cn': 64, 'nrs': 16, 'rps': 2}]
    assert [(p['cn'], p['nrs']) for p in ref.rows_split(5, 2304)] == [(1024, 1), (1024, 1), (256, 4)]
    assert [(p['cn'], p['nrs']) for p in ref.rows_split(5, 1030)] == [(1024, 1), (8, 128)] and ref.rows_split(1, 75)[0]['nrs'] == 13
    assert ref.map_split(75) == {'c4p': 32, 'PL': 32, 'passes': [0]} and ref.map_split(1152) == {'c4p': 512, 'PL': 2, 'passes': [0]}
    assert ref.map_split(4100) == {'c4p': 1024, 'PL': 1, 'passes': [0, 1024]} and ref.map_split(1)['PL'] == 1024


def _stage_classes(n_in, passes, count, per):
    """the classes one stage of one case is in"""
    out = set()
    if len(passes) > 1:
        out.add('second pass')
        if passes[-1][count] == 1:
            out.add('second pass of one quad')
    for p in passes:
        rng = ref.seg_ranges(n_in, p['nseg'], p[per])
        lens = [b - a for a, b in rng]
        most = ref.SE_FC_THREADS // p[count]
        if p['nseg'] == 1:
            out.add('one segment')
        elif all(n == lens[0] for n in lens):
            out.add('equal segments')
        if p['nseg'] > 1 and 0 < lens[-1] < p[per]:
            out.add('short last segment')
        if lens[-1] <= 0:
            out.add('empty last segment')
        if p[per] % ref.FC_BATCH:
            out.add('batch tail')
        if p['nseg'] == most < (n_in + 15) // 16:
            out.add('cap reached')
        if ref.SE_FC_THREADS % p[count]:
            out.add('idle lanes')
    return out


STAGE_CLASSES = {'second pass', 'second pass of one quad', 'one segment', 'equal segments', 'short last segment', 'empty last segment', 'batch tail',
                 'cap reached', 'idle lanes'}


def test_fc_cases_hold_every_class():
    fc1, fc2 = set(), set()
    for c, r in ref.FC_CASES:
        assert ref.lds_bytes(c, r, 0) <= ref.LDS_LIMIT, (c, r)
        fc1 |= _stage_classes(c, ref.fc1_split(c, r), 'jq', 'cps')
        fc2 |= _stage_classes(r, ref.fc2_split(c, r), 'qp', 'jps')
    assert fc1 == STAGE_CLASSES, STAGE_CLASSES - fc1
    assert fc2 == STAGE_CLASSES, STAGE_CLASSES - fc2
    cases = set(ref.FC_CASES)
    assert len(cases) == len(ref.FC_CASES)
    # the cases the work was specified with, by name
    assert {(33, 8), (75, 5), (2304, 96), (520, 128), (8, 4100), (512, 130), (4100, 4)} <= cases
    assert {(512, 128), (32, 8), (96, 4), (144, 6), (240, 10), (480, 20), (672, 28), (1152, 48), (1392, 58), (2304, 96)} == set(ref.FC_SHIPPED) <= cases
    assert {1, 2, 4, 6} <= {r for _, r in cases} and {1, 2, 3, 6} <= {c for c, _ in cases}          # pad lanes of a quad, either stage
    assert any(c <= 16 for c, _ in cases)
    assert [b - a for a, b in ref.seg_ranges(130, 8, 17)] == [17] * 7 + [11]


def test_mean_cases_hold_every_class():
    assert {1, 63, 64, 65, 169} <= set(ref.MEAN_HW) and any(hw > 8 * ref.SE_MEAN_PL for hw in ref.MEAN_HW)
    assert {1, 3, 4, 61, 64, 75, 260} <= set(ref.MEAN_C)
    c4 = [-(-c // 4) for c in ref.MEAN_C]
    assert any(c % 4 for c in ref.MEAN_C) and any(q % ref.SE_MEAN_QUADS for q in c4) and any(q > ref.SE_MEAN_QUADS for q in c4)
    assert any(q > ref.SE_MEAN_QUADS and q % ref.SE_MEAN_QUADS for q in c4), 'a last workgroup along x with idle quads'


def test_map_cases_hold_every_class():
    by_c = {}
    for c, r, hw, wide in ref.MAP_CASES:
        assert hw > 1 and ref.lds_bytes(c, r, 1) <= ref.LDS_LIMIT, (c, r, hw)
        by_c.setdefault(c, []).append((hw, wide))
    splits = {c: ref.map_split(c) for c in by_c}
    assert any(s['c4p'] == -(-c // 4) for c, s in splits.items()), 'ceil(C / 4) a power of two'
    assert splits[75] == {'c4p': 32, 'PL': 32, 'passes': [0]} and -(-75 // 4) == 19, 'C = 75: 13 idle quads'
    for c, s in splits.items():
        pl = s['PL']
        if 3 < pl:
            assert {2, pl - 1, pl, pl + 1, 3 * pl + 1} <= {hw for hw, _ in by_c[c]}, c
            assert any(hw < pl for hw, _ in by_c[c])
    assert splits[1152]['c4p'] == 512 and splits[1152]['PL'] == 2 and {2, 3} <= {hw for hw, _ in by_c[1152]}
    assert (3, False) in by_c[4100] and len(splits[4100]['passes']) == 2 and splits[4100]['PL'] == 1
    assert any(wide for v in by_c.values() for _, wide in v) and any(not wide for v in by_c.values() for _, wide in v)


def test_rows_cases_hold_every_class():
    by_c = {}
    for c, r, rows, wide in ref.ROWS_CASES:
        assert ref.lds_bytes(c, r, 2) <= ref.LDS_LIMIT and ref.rows_pixels(rows) != rows
        by_c.setdefault(c, []).append((rows, wide))
    one_pass = [c for c in by_c if len(ref.rows_split(1, c)) == 1]
    assert len(one_pass) >= 3
    for c in one_pass:
        nrs = ref.rows_split(1, c)[0]['nrs']
        assert {1, 15, 16, 17, nrs - 1, nrs, nrs + 1, 5 * nrs + 3} <= {rows for rows, _ in by_c[c]}, c
    assert (17, True) in by_c[64] or (17, False) in by_c[64]
    p = ref.rows_split(17, 64)[0]
    assert [b - a for a, b in ref.seg_ranges(17, p['nrs'], p['rps'])][8:] == [1, -1, -3, -5, -7, -9, -11, -13], 'trailing empty row segments'
    assert ref.SE_FC_THREADS % ref.rows_split(1, 75)[0]['cn'], 'C = 75: cn = 76 does not divide 1024'
    assert {1030, 1392, 2304} <= set(by_c)
    assert [len(ref.rows_split(1, c)) for c in (1030, 1392, 2304)] == [2, 2, 3] and ref.rows_split(1, 1030)[1]['cn'] == 8
    # a segment longer than a batch of 16 with a clamped tail, in a one-pass and in a several-pass case; and one of exactly 16 and 32
    tails = [(c, rows) for c, v in by_c.items() for rows, _ in v for p in ref.rows_split(rows, c) if p['rps'] > ref.ROWS_BATCH and p['rps'] % ref.ROWS_BATCH]
    assert any(c in one_pass for c, _ in tails) and any(c not in one_pass for c, _ in tails)
    for c in (1030, 1392):          # the narrow last pass at nrs - 1, nrs, nrs + 1 rows
        nrs = ref.rows_split(1, c)[-1]['nrs']
        assert {nrs - 1, nrs, nrs + 1} <= {rows for rows, _ in by_c[c]}, c
    for c, v in by_c.items():
        assert {wide for _, wide in v} == {False, True}, c
