"""Host side of the fusing operators (no GPU): the restatements of tests/fusegrad_ref.py against hand-derived answers, the new entries
of the library, and what the case lists of tests/test_gpu_fusegrad.py reach."""
import ctypes
import os
import re

import numpy as np

from tests import fusegrad_ref as ref

F32 = np.float32
NEW_ENTRIES = ('yr_maxpool_forward', 'yr_maxpool_backward', 'yr_upsample2_forward', 'yr_upsample2_backward', 'yr_wsum_chunk',
               'yr_wsum_workspace_bytes', 'yr_wsum_forward', 'yr_wsum_backward')


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _window(values):
    """four values -> x [1, 2, 2, 1], row-major"""
    return np.array(values, F32).reshape(1, 2, 2, 1)


# ----------------------------------------------------------------------------- hand-derived answers
def test_maxpool_window_by_hand():
    """a 2 x 2 window, dy = 7: the maximum at each of the four positions; all four tied: the first; the last two tied: the third
    (the first of the two); float64 autograd agrees"""
    dy = np.full((1, 1, 1, 1), 7, F32)
    cases = [([9, 1, 2, 3], 0), ([1, 9, 2, 3], 1), ([1, 2, 9, 3], 2), ([1, 2, 3, 9], 3), ([5, 5, 5, 5], 0), ([1, 2, 6, 6], 2)]
    for values, first in cases:
        x = _window(values)
        want = np.zeros(4, F32)
        want[first] = 7
        assert ref.maxpool32(x, 2).reshape(()) == max(values)
        dx = ref.maxpool_backward32(dy, x, 2)
        assert np.array_equal(_bits(dx.reshape(4)), _bits(want)), values
        y64, dx64 = ref.maxpool_grads64(x, dy, 2)
        assert y64.reshape(()) == max(values) and np.array_equal(dx64.reshape(4), want), values


def test_maxpool_signed_zeros():
    """-0 and +0 compare equal, so the first of them wins, and the forward returns ITS bits"""
    dy = np.full((1, 1, 1, 1), 3, F32)
    for values, y_bits in (([-0.0, 0.0, 0.0, -0.0], 0x80000000), ([0.0, -0.0, -0.0, 0.0], 0), ([-1.0, -0.0, 0.0, -2.0], 0x80000000)):
        x = _window(values)
        first = 1 if values[0] == -1.0 else 0
        assert _bits(ref.maxpool32(x, 2)).reshape(()) == y_bits
        dx = ref.maxpool_backward32(dy, x, 2).reshape(4)
        want = np.zeros(4, F32)
        want[first] = 3
        assert np.array_equal(_bits(dx), _bits(want)), values          # the other three are +0, never -0


def test_maxpool_trailing_strip():
    """a 5 x 5 map at k = 2: four windows; row 4 and column 4 are read by nothing and their gradient is +0"""
    x = np.arange(25, dtype=F32).reshape(1, 5, 5, 1)          # increasing: every window's maximum is its last element
    x[0, 4, :, 0] = 1000          # the strip holds the largest values of the map: they must not matter
    x[0, :, 4, 0] = 1000
    dy = np.array([[1, 2], [3, 4]], F32).reshape(1, 2, 2, 1)
    assert np.array_equal(ref.maxpool32(x, 2).reshape(2, 2), [[6, 8], [16, 18]])
    dx = ref.maxpool_backward32(dy, x, 2).reshape(5, 5)
    want = np.zeros((5, 5), F32)
    want[1, 1], want[1, 3], want[3, 1], want[3, 3] = 1, 2, 3, 4
    assert np.array_equal(_bits(dx), _bits(want))
    y64, dx64 = ref.maxpool_grads64(x, dy, 2)
    assert np.array_equal(dx64.reshape(5, 5), want) and np.array_equal(y64.reshape(2, 2), [[6, 8], [16, 18]])
    # k = 4 on 5 x 7: one window, the strip is a row and three columns
    x = np.zeros((1, 5, 7, 1), F32)
    x[0, 2, 3, 0] = 2
    x[0, 4, 6, 0] = 9
    dx = ref.maxpool_backward32(np.full((1, 1, 1, 1), 5, F32), x, 4).reshape(5, 7)
    want = np.zeros((5, 7), F32)
    want[2, 3] = 5
    assert np.array_equal(_bits(dx), _bits(want))


def test_upsample_by_hand():
    """one element becomes a 2 x 2 block; the gradient adds the block in row-major order: ((2^24 + 1) + 1) + 1 = 2^24 in float32 (each
    1 is absorbed: ties to even), where (2^24 + 1) + (1 + 1) would be 2^24 + 2 and the exact sum is 2^24 + 3"""
    x = np.array([[1, 2], [3, 4]], F32).reshape(1, 2, 2, 1)
    assert np.array_equal(ref.upsample32(x).reshape(4, 4), [[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]])
    big = F32(2.0 ** 24)
    dy = np.array([[big, 1], [1, 1]], F32).reshape(1, 2, 2, 1)
    assert ref.upsample_backward32(dy).reshape(()) == big
    assert F32(F32(big + F32(1)) + F32(F32(1) + F32(1))) == big + 2
    _, dx64 = ref.upsample_grads64(np.zeros((1, 1, 1, 1)), dy)
    assert dx64.reshape(()) == 2.0 ** 24 + 3
    # ((1 + 2^24) + -2^24) + 1 = 1: the first 1 is lost, the last survives
    dy = np.array([[1, big], [-big, 1]], F32).reshape(1, 2, 2, 1)
    assert ref.upsample_backward32(dy).reshape(()) == 1
    dy = np.arange(16, dtype=F32).reshape(1, 4, 4, 1)
    assert np.array_equal(ref.upsample_backward32(dy).reshape(2, 2), [[0 + 1 + 4 + 5, 2 + 3 + 6 + 7], [8 + 9 + 12 + 13, 10 + 11 + 14 + 15]])


def test_weighted_sum_by_hand():
    """alpha = (2, -3, 0, 0.5) on x = (1, 2, 100, 4), dy = 3: y = 2 - 6 + 0 + 2 = -2; dx = alpha dy = (6, -9, 0, 1.5); dalpha = dy x =
    (3, 6, 300, 12) - the map behind a zero alpha still has a gradient for its alpha"""
    alpha = np.array([2, -3, 0, 0.5], F32)
    xs = [np.full((1, 1), v, F32) for v in (1, 2, 100, 4)]
    dy = np.full((1, 1), 3, F32)
    assert ref.wsum32(xs, alpha).reshape(()) == -2
    assert [float(v.reshape(())) for v in ref.wsum_dx32(dy, alpha)] == [6, -9, 0, 1.5]
    assert [float(ref.seq_dot(dy, x)) for x in xs] == [3, 6, 300, 12] == [float(ref.ordered_dot(dy, x, 5)) for x in xs]
    y64, dx64, da64 = ref.wsum_grads64(xs, alpha, dy)
    assert y64.reshape(()) == -2 and [float(v.reshape(())) for v in dx64] == [6, -9, 0, 1.5] and da64.tolist() == [3, 6, 300, 12]
    # the order: each product rounded, then left to right.  (2^24 + 1) + 1 is absorbed twice
    xs = [np.full((1, 1), v, F32) for v in (2.0 ** 24, 1, 1, 0)]
    assert ref.wsum32(xs, np.ones(4, F32)).reshape(()) == 2.0 ** 24


def test_ordered_dot_is_the_stated_order():
    """against a literal restatement of fusegrad.hip's header, lane by lane, and against the sequential sum where they must agree"""
    def literal(dy, x, chunk, threads):
        p, c = dy.shape
        total = None
        for p0 in range(0, p, chunk):
            lanes, e = np.zeros(threads, F32), 0
            for q in range(p0, min(p0 + chunk, p)):
                for cc in range(c):
                    lanes[e % threads] = F32(lanes[e % threads] + F32(dy[q, cc] * x[q, cc]))
                    e += 1
            waves = []
            for w in range(threads // 64):
                v = lanes[64 * w:64 * w + 64].copy()
                for off in (32, 16, 8, 4, 2, 1):
                    v = np.array([F32(v[lane] + v[lane ^ off]) for lane in range(64)], F32)
                assert np.all(_bits(v) == _bits(v)[0]), 'every lane of the butterfly holds the same bits'
                waves.append(v[0])
            s = waves[0]
            for t in waves[1:]:
                s = F32(s + t)
            total = s if total is None else F32(total + s)
        return total
    rng = np.random.default_rng(0)
    for p, c, chunk, threads in ((1, 1, 5, 1024), (700, 3, 300, 1024), (50, 48, 22, 1024), (129, 75, 110, 1024), (40, 7, 13, 128)):
        dy, x = (1 + rng.standard_normal((p, c))).astype(F32), (1 + rng.standard_normal((p, c))).astype(F32)
        assert _bits(ref.ordered_dot(dy, x, chunk, threads)) == _bits(literal(dy, x, chunk, threads)), (p, c, chunk)
    dy, x = rng.standard_normal((30, 2)).astype(F32), rng.standard_normal((30, 2)).astype(F32)          # 60 pairs: one a lane, lanes 60.. +0
    pairs = (dy * x).reshape(-1)
    v = np.concatenate([pairs, np.zeros(4, F32)])
    n = 64
    while n > 1:
        n //= 2
        v = v[:n] + v[n:2 * n]
    assert _bits(ref.ordered_dot(dy, x, 100)) == _bits(v[0])
    # 2^24 + 1 + 1 + ... sequentially stays at 2^24
    dy = np.ones((9, 1), F32)
    x = np.ones((9, 1), F32)
    x[0] = 2.0 ** 24
    assert ref.seq_dot(dy, x) == 2.0 ** 24


# ----------------------------------------------------------------------------- the library
def _lib():
    from yoloret_amd import runtime as rt
    return ctypes.CDLL(rt.LIB_PATH)


def _source():
    from yoloret_amd import build
    return open(os.path.join(build.CSRC, 'fusegrad.hip')).read()


def _define(src, name):
    return int(re.search(r'#define %s (\d+) ' % name, src).group(1))


def test_entries_are_exported_and_bound():
    from yoloret_amd import build, runtime as rt
    lib = _lib()
    header = open(os.path.join(build.HERE, '..', 'include', 'yoloret_hip.h')).read()
    for name in NEW_ENTRIES:
        assert getattr(lib, name) is not None and name in rt.EXPORTS and re.search(r'\b%s\(' % name, header), name
    assert 'fusegrad.hip' in build.SOURCES and lib.yr_abi_version() == 9 == rt.ABI_VERSION
    for name in ('maxpool_forward', 'maxpool_backward', 'upsample2_forward', 'upsample2_backward', 'wsum_forward', 'wsum_backward', 'wsum_chunk',
                 'wsum_workspace_bytes'):
        assert callable(getattr(rt, name)) and getattr(rt, name).__doc__


def test_no_kernel_of_the_file_uses_scratch():
    from yoloret_amd import build
    rows = build.kernel_resources()['fusegrad.hip']
    assert len(rows) == 9 and all(scratch == 0 for _, _, scratch, _, _ in rows), rows


def test_chunk_rule_and_refusals():
    from yoloret_amd import runtime as rt
    src = _source()
    min_elems, most, threads = _define(src, 'WS_MIN_ELEMS'), _define(src, 'WS_MAX_CHUNKS'), _define(src, 'WS_THREADS')
    assert (min_elems, most, threads) == (8192, 256, 1024) and threads == ref.WS_THREADS
    assert most <= 1024, 'at or below what yr_launch_slab_sum is used with elsewhere (CG_DW_MAX_CHUNKS 1024, HT_MAX_CHUNKS 2048)'
    for c in (1, 3, 48, 75, 1024, 5000, 8192, 8193):
        minimum = -(-min_elems // c)
        for p in (1, minimum, minimum + 1, most * minimum, most * minimum + 1, 10 * most * minimum + 7):
            chunk = rt.wsum_chunk(p, c)
            assert chunk == max(minimum, -(-p // most)), (p, c)
            slabs = -(-p // chunk)
            assert slabs <= most and rt.wsum_workspace_bytes(p, c) == 16 * slabs
    # from 2^38 pixels on the cap is 1024, so that the chunk fits an int
    assert rt.wsum_chunk((1 << 38) - 1, 48) == -(-((1 << 38) - 1) // 256) and rt.wsum_chunk(1 << 38, 48) == 1 << 28 and rt.wsum_chunk((1 << 40) - 1, 1) == 1 << 30
    for bad in ((0, 8), (-1, 8), (1 << 40, 8), (40, 0), (40, -3), (40, (1 << 30) + 1)):
        assert rt.wsum_chunk(*bad) == 0 and rt.wsum_workspace_bytes(*bad) == 0, bad


def test_gpu_case_lists_reach_what_they_claim():
    from tests import test_gpu_fusegrad as g
    from yoloret_amd import runtime as rt
    src = _source()
    assert (g.WSUM_MIN_ELEMS, g.WSUM_MAX_CHUNKS) == (_define(src, 'WS_MIN_ELEMS'), _define(src, 'WS_MAX_CHUNKS'))
    for c in g.WSUM_CHANNELS:
        minimum = g.wsum_min_chunk(c)
        counts = g.wsum_pixels(c)
        assert counts == [1, 2, 63, 64, 65, minimum - 1, minimum, minimum + 1, 2 * minimum + 1] and minimum > 65
        chunks = [rt.wsum_chunk(p, c) for p in counts]
        assert chunks == [minimum] * len(counts), 'the minimum sets every chunk of the list'
        slabs = [-(-p // minimum) for p in counts]
        assert slabs == [1, 1, 1, 1, 1, 1, 1, 2, 3], 'one slab, exactly one full slab, two, three'
        assert counts[-1] - 2 * minimum == 1 and counts[-2] - minimum == 1, 'a last range of one pixel'
        assert rt.wsum_workspace_bytes(counts[-1], c) == 48
        # lanes: fewer pairs than lanes (idle lanes), exactly the lanes, more than one step
        assert counts[0] * c < 1024 < counts[-1] * c
    # the branch where the slab cap sets the chunk
    p, c = g.WORKLOAD_LIKE
    minimum = g.wsum_min_chunk(c)
    assert c == 48 and p % (2 * 26 * 26) == 0 and p > g.WSUM_MAX_CHUNKS * minimum > p - 2 * 26 * 26, 'the first multiple of 2 * 26 * 26 in that branch'
    chunk = rt.wsum_chunk(p, c)
    assert chunk == -(-p // g.WSUM_MAX_CHUNKS) == 175 > minimum == 171 and -(-p // chunk) == 255 and p - 254 * chunk == 166
    assert chunk * c % 1024 and 1024 % c, 'neither the range nor the lanes divide evenly: a lane\'s channel changes from step to step'
    # integers stay exact at the largest size: every partial sum of |dy x| below 2^24
    xs, dy, alpha = g.wsum_case(p, c, True)
    assert max(np.abs(dy.astype(np.float64) * x.astype(np.float64)).sum() for x in xs) < 2 ** 24
    assert (alpha < 0).any() and (alpha == 0).any()
    _, _, alpha = g.wsum_case(p, c, False)
    assert (alpha < 0).any() and (alpha == 0).any(), 'a negative and a zero alpha'
    # max-pooling: one window, multiples of k, a remainder in rows and columns; the trailing strip up to k - 1 wide
    for k, shapes in g.POOL_SHAPES.items():
        rem = {(h % k, w % k) for h, w in shapes}
        assert (0, 0) in rem and any(a and b for a, b in rem)
        assert max(max(h % k, w % k) for h, w in shapes) == k - 1 and min(min(h, w) for h, w in shapes) == k
    assert g.POOL_SHAPES == {2: [(2, 2), (3, 5), (5, 4), (7, 9), (26, 26)], 4: [(4, 4), (5, 7), (9, 11), (24, 24)]}
    assert g.MAP_CHANNELS == [1, 3, 48, 75, 130] and g.BATCHES == [1, 3] and g.UP_SHAPES == [(1, 1), (2, 3), (7, 5), (13, 13)]
    # more than one workgroup of 256 lanes, and a last one that is not full
    assert 3 * 13 * 13 * 130 > 256 and 3 * 13 * 13 * 130 % 256 and 3 * 12 * 12 * 130 > 256
    rng = np.random.default_rng(0)
    x = g.pool_data('ints', (3, 26, 26, 48), rng)
    gap, top, _ = ref.top_two_gap(x, 2)
    assert (gap == 0).mean() > 0.3 and (ref.top_two_gap(x[:, :24, :24], 4)[0] == 0).mean() > 0.8, 'a third of the 2 x 2 windows tie at the maximum, most 4 x 4 ones'
    x = g.pool_data('relu6', (3, 26, 26, 48), rng)
    gap, top, _ = ref.top_two_gap(x, 2)
    assert ((gap == 0) & ((top == 0) | (top == 6))).mean() > 0.05
