"""Host side of BatchNorm in training mode (no GPU): the restatements of tests/bntrain_ref.py against hand-derived answers, the new
entries of the library, and what the case lists of tests/test_gpu_bntrain.py reach."""
import ctypes
import os
import re

import numpy as np

from tests import bntrain_ref as ref

F32 = np.float32
NEW_ENTRIES = ('yr_bn_train_chunk', 'yr_bn_train_workspace_bytes', 'yr_bn_train_forward', 'yr_bn_train_backward')


# ----------------------------------------------------------------------------- hand-derived answers
def test_two_pixels_by_hand():
    """z = [[1], [3]], eps = 0: mean 2, var ((-1)^2 + 1^2) / 2 = 1, invstd 1, xhat = (-1, +1).  gamma 2, beta 1: u = (-1, 3).
    da = (1, 3): dbeta = 4, dgamma = -1 + 3 = 2; dz = ((g - 4 / 2) - xhat 2 / 2) gamma invstd = ((-1 + 1) 2, (1 - 1) 2) = (0, 0): with two
    pixels every gradient lies in the span of (1, 1) and xhat, which the batch statistics remove.
    ReLU6 masks the first pixel (u = -1): g = (0, 3), dbeta = 3, dgamma = 3, dz = ((0 - 1.5) + 1.5, (3 - 1.5) - 1.5) 2 = (0, 0)."""
    z, gamma, beta, da = [[1.0], [3.0]], [2.0], [1.0], [[1.0], [3.0]]
    f64, f32 = ref.forward64(z, gamma, beta, 0.0), ref.forward32(z, gamma, beta, 0.0)
    for f in (f64, f32):
        assert f['mean'][0] == 2 and f['var'][0] == 1 and f['invstd'][0] == 1
        assert np.array_equal(f['xhat'][:, 0], [-1, 1]) and np.array_equal(f['u'][:, 0], [-1, 3]) and np.array_equal(f['a'], f['u'])
    assert np.array_equal(ref.forward32(z, gamma, beta, 0.0, act='relu6')['a'][:, 0], [0, 3])
    for act, want in ((None, (4, 2)), ('relu6', (3, 3))):
        dz, dgamma, dbeta = ref.backward32(da, z, gamma, beta, f32['mean'], f32['invstd'], act)
        assert dbeta[0] == want[0] and dgamma[0] == want[1] and np.array_equal(dz[:, 0], [0, 0])
        dz, dgamma, dbeta = ref.backward64(da, z, gamma, beta, 0.0, act)
        assert abs(dbeta[0] - want[0]) < 1e-12 and abs(dgamma[0] - want[1]) < 1e-12 and np.abs(dz).max() < 1e-12


def test_four_pixels_by_hand():
    """z = (0, 0, 4, 4), eps = 0: mean 2, var 4, invstd 1 / 2, xhat = (-1, -1, 1, 1).  gamma 3, beta 0, da = (1, 0, 0, 0): dbeta = 1,
    dgamma = -1; dz = ((g - 1 / 4) - xhat (-1 / 4)) 3 / 2: g - 1/4 = (3/4, -1/4, -1/4, -1/4), xhat / 4 = (-1/4, -1/4, 1/4, 1/4), the sum
    (1/2, -1/2, 0, 0), times 3/2: (3/4, -3/4, 0, 0)."""
    z, da = [[0.0], [0.0], [4.0], [4.0]], [[1.0], [0.0], [0.0], [0.0]]
    f = ref.forward32(z, [3.0], [0.0], 0.0)
    assert f['mean'][0] == 2 and f['var'][0] == 4 and f['invstd'][0] == 0.5 and np.array_equal(f['xhat'][:, 0], [-1, -1, 1, 1])
    dz, dgamma, dbeta = ref.backward32(da, z, [3.0], [0.0], f['mean'], f['invstd'])
    assert dbeta[0] == 1 and dgamma[0] == -1 and np.array_equal(dz[:, 0], [0.75, -0.75, 0, 0])
    dz64, dg64, db64 = ref.backward64(da, z, [3.0], [0.0], 0.0)
    assert np.allclose(dz64[:, 0], [0.75, -0.75, 0, 0], rtol=0, atol=1e-12) and abs(dg64[0] + 1) < 1e-12 and abs(db64[0] - 1) < 1e-12


def test_relu6_ties_pass_nothing():
    """u exactly 0 and exactly 6 are masked (both comparisons strict), and what is masked is +0"""
    g = ref.act_grad32(np.full((5, 1), 5.0, F32), np.array([[0.0], [3.0], [6.0], [-1.0], [7.0]], F32), 'relu6')
    assert np.array_equal(g[:, 0], [0, 5, 0, 0, 0]) and not np.signbit(g).any()
    z = np.array([[1.0], [3.0]])          # xhat = (-1, 1); gamma 3, beta 3: u = (0, 6)
    dz, dgamma, dbeta = ref.backward64([[1.0], [1.0]], z, [3.0], [3.0], 0.0, 'relu6')
    assert dgamma[0] == 0 and dbeta[0] == 0 and not dz.any()


def test_bessel_factor_and_moving_update():
    """N = 1: max(N - 1, 1) = 1, the factor is 1 (the variance of one pixel is 0 either way); N = 2: 2."""
    assert ref.bessel(1) == 1 and ref.bessel(2) == 2 and ref.bessel(4) == F32(4 / 3) and ref.bessel(1 << 30) == 1
    # z = (1, 3): mean 2, biased variance 1, unbiased 2; momentum 0.5 from (0, 1): mean 0 - (0 - 2) / 2 = 1, var 1 - (1 - 2) / 2 = 1.5
    f = ref.forward32([[1.0], [3.0]], [1.0], [0.0], 0.0, 0.5, None, [0.0], [1.0])
    assert f['moving_mean'][0] == 1 and f['moving_var'][0] == 1.5
    mm, mv = ref.moving64([0.0], [1.0], [2.0], [1.0], 2, 0.5)
    assert mm[0] == 1 and mv[0] == 1.5
    # momentum 1 freezes them, momentum 0 replaces them
    f = ref.forward32([[1.0], [3.0]], [1.0], [0.0], 0.0, 1.0, None, [7.0], [9.0])
    assert f['moving_mean'][0] == 7 and f['moving_var'][0] == 9
    f = ref.forward32([[1.0], [3.0]], [1.0], [0.0], 0.0, 0.0, None, [7.0], [9.0])
    assert f['moving_mean'][0] == 2 and f['moving_var'][0] == 2
    # one pixel: var +0, invstd = 1 / sqrt(eps), a = beta
    f = ref.forward32([[5.0, -2.0]], [1.5, 2.0], [0.25, -1.0], 1e-3)
    assert np.array_equal(f['mean'], [5, -2]) and not f['var'].any() and np.array_equal(f['a'], [[0.25, -1.0]])
    assert np.array_equal(f['invstd'], np.full(2, F32(1) / np.sqrt(F32(1e-3)), F32))


def test_sequential_sum_is_sequential():
    """2^24 + 1 + 1 + ... stays at 2^24 when added one by one in float32 (a pairwise sum would not), and starts from +0"""
    x = np.ones((9, 1), F32)
    x[0] = 2.0 ** 24
    assert ref.seq_sum(x)[0] == 2.0 ** 24 and float(np.sum(x.astype(np.float64))) == 2.0 ** 24 + 8
    assert not np.signbit(ref.seq_sum(np.full((3, 2), -0.0, F32))).any()


def test_the_two_restatements_agree():
    rng = np.random.default_rng(0)
    z = 10 + 3 * rng.standard_normal((50, 7))
    gamma, beta, da = rng.uniform(-2, 2, 7), rng.standard_normal(7), rng.standard_normal((50, 7))
    for act in (None, 'relu6', 'swish'):
        f64, f32 = ref.forward64(z, gamma, beta, 1e-3, act), ref.forward32(z, gamma, beta, 1e-3, 0.9, act)
        for k in ('a', 'mean', 'var', 'invstd'):
            assert ref.rel_err(f32[k], f64[k]) < 1e-5, (act, k)
        g64 = ref.backward64(da, z, gamma, beta, 1e-3, act)
        g32 = ref.backward32(da, z.astype(F32), gamma, beta, f32['mean'], f32['invstd'], act)
        for a, b in zip(g32, g64):
            assert ref.rel_err(a, b) < 1e-4, act
    s, b = ref.fold64([2.0], [1.0], [3.0], [4.0], 0.0)
    assert s[0] == 1 and b[0] == -2


# ----------------------------------------------------------------------------- the library
def _source():
    from yoloret_amd import build
    return open(os.path.join(os.path.dirname(build.__file__), 'csrc', 'bntrain.hip')).read()


def test_new_entries_are_exported_under_abi_9():
    """fails on the parent commit: the symbols are missing there"""
    from yoloret_amd import autograd, build, runtime
    L = ctypes.CDLL(build.LIB)
    L.yr_abi_version.restype = ctypes.c_int
    assert L.yr_abi_version() == 9 == runtime.ABI_VERSION
    for sym in NEW_ENTRIES:
        getattr(L, sym)
        assert sym in runtime.EXPORTS
    assert 'bntrain.hip' in build.SOURCES
    for name in ('bn_train_chunk', 'bn_train_workspace_bytes', 'bn_train_forward', 'bn_train_backward'):
        assert callable(getattr(runtime, name))
    assert callable(autograd.batchnorm_act) and callable(autograd.fold_batchnorm)
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'yoloret_hip.h')).read()
    assert all(sym + '(' in header for sym in NEW_ENTRIES)
    assert 'UNBIASED' in header and 'define YR_ABI_VERSION 9' in re.sub(r'\s+', ' ', header)


def test_kernels_use_no_scratch():
    from yoloret_amd import build
    rows = build.kernel_resources()['bntrain.hip']
    assert len(rows) == 6          # sums, squared deviations, apply; backward sums, backward apply, the slab sum of dz == null
    assert all(scratch == 0 for _, _, scratch, _, _ in rows)


def test_launch_counts_are_as_the_header_says():
    """forward 3, backward 2 (the elementwise pass or, with dz == null, the slab sum): the entry bodies hold that many launches"""
    from yoloret_amd import build
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'yoloret_hip.h')).read()
    text = header[header.index('BatchNorm (+ activation) in training mode'):]
    assert '3 launches.' in text and '2 launches either way.' in text
    src = _source()
    fwd = src[src.index('extern "C" int yr_bn_train_forward'):src.index('extern "C" int yr_bn_train_backward')]
    bwd = src[src.index('extern "C" int yr_bn_train_backward'):]
    assert fwd.count('hipLaunchKernelGGL(') == 3 and 'else' not in fwd
    assert bwd.count('hipLaunchKernelGGL(') == 3 and bwd.count('else') == 1 and re.search(r'if \(dz\)\s+hipLaunchKernelGGL\(bt_bwd_apply_kernel', bwd)
    assert 'atomic' not in src.lower().replace('no float atomics', '')
    from yoloret_amd import runtime
    assert 'Three launches' in runtime.bn_train_forward.__doc__ and 'Two launches' in runtime.bn_train_backward.__doc__


def test_chunk_is_a_function_of_the_sizes_only():
    from yoloret_amd import runtime as rt
    src = _source()
    assert '#define BT_MIN_ELEMS 8192 ' in src and '#define BT_MAX_CHUNKS 256 ' in src and '#define BT_CB 64 ' in src
    for pixels, c in ((1, 1), (1, 256), (2, 75), (1030, 3), (64 * 13 * 13, 512), (64 * 26 * 26, 256), (64 * 52 * 52, 128), (64 * 208 * 208, 16), (1 << 30, 7)):
        chunk = rt.bn_train_chunk(pixels, c)
        assert chunk >= 1 and chunk * min(c, 64) >= 8192 and chunk == rt.bn_train_chunk(pixels, c)
        slabs = -(-pixels // chunk)
        assert slabs <= 256
        assert rt.bn_train_workspace_bytes(pixels, c) == 2 * slabs * c * 4
    assert rt.bn_train_chunk(5000, 64) == 128 and rt.bn_train_chunk(5000, 3) == 2731 and rt.bn_train_chunk(5000, 1) == 8192
    assert rt.bn_train_chunk(64 * 52 * 52, 128) == 676          # 173056 pixels: more than 256 chunks of 128
    assert rt.bn_train_chunk((1 << 40) - 1, 8) == 1 << 30 and rt.bn_train_workspace_bytes((1 << 40) - 1, 8) == 2 * 1024 * 8 * 4
    for bad in ((0, 8), (-1, 8), (1 << 40, 8), (40, 0), (40, -3)):
        assert rt.bn_train_chunk(*bad) == 0 and rt.bn_train_workspace_bytes(*bad) == 0


# ----------------------------------------------------------------------------- what tests/test_gpu_bntrain.py reaches
def test_gpu_cases_reach_what_they_claim():
    from tests import test_gpu_bntrain as g
    from yoloret_amd import runtime as rt
    assert g.BN_CHANNELS == [1, 3, 63, 64, 75, 130, 256] and g.BN_PIXELS == [1, 2, 63, 64, 65, 66, 258, 1030] and g.PAD == 5
    # the flat form (C < 64: 1024 // C pixels a step, with and without idle lanes), one whole channel block, a partial second and third one
    assert '#define BT_THREADS 1024 ' in _source()
    assert any(1024 % c == 0 for c in g.BN_CHANNELS if c < 64) and any(1024 % c for c in g.BN_CHANNELS if c < 64) and 64 in g.BN_CHANNELS
    assert any(64 < c < 128 for c in g.BN_CHANNELS) and any(128 < c and c % 64 for c in g.BN_CHANNELS)
    # pixel counts below and above what the 1024 lanes cover in one step, with a partial last step, for every channel count
    for c in g.BN_CHANNELS:
        step = 1024 // min(c, 64)
        assert any(p < step for p in g.BN_PIXELS) and any(p > step and p % step for p in g.BN_PIXELS)
    # the exact forward data: per-channel sums of exactly m N, integer squared deviations, a constant channel, odd counts
    for pixels in g.BN_PIXELS + g.chunk_pixels(3)[1]:
        for c in (1, 3, 75):
            z, m, gamma, beta, moving = g.exact_forward_case(pixels, c)
            assert np.array_equal(z, np.round(z)) and np.abs(z).max() <= 7
            assert np.array_equal(z.astype(np.float64).sum(0), m.astype(np.float64) * pixels)
            assert np.abs(z).sum(0).max() < 2 ** 24 and ((z - m[None, :]) ** 2).sum(0).max() < 2 ** 24
            if c >= 3:
                assert not (z[:, 2] - m[2]).any()
            if pixels > 8:
                assert (z[:, 0] != m[0]).any()
    # the exact backward data: var 4, xhat -1 / +1 in equal numbers, u exact with ties at 0 and at 6, inside, below and above
    for pixels in g.BN_EVEN_PIXELS:
        for c in (1, 3, 75):
            z, gamma, beta, da = g.exact_backward_case(pixels, c)
            f = ref.forward32(z, gamma, beta, 0.0)
            assert np.all(f['var'] == 4) and np.all(f['invstd'] == 0.5) and np.all(f['xhat'].sum(0) == 0) and np.all(np.abs(f['xhat']) == 1)
            u = f['u'].astype(np.float64)
            assert np.array_equal(u, ref.forward64(z, gamma, beta, 0.0)['u']), 'u is exact in float32'
            assert (u == 0).any()
            if c >= 8:
                assert (u == 6).any() and ((u > 0) & (u < 6)).any() and (u < 0).any() and (u > 6).any()
                assert any(((u[:, ch] == 0) | (u[:, ch] == 6)).all() for ch in range(c)), 'a channel with both values masked'
            assert np.array_equal(da, np.round(da)) and np.abs(da).max() <= 4
    assert all(p % 2 == 0 for p in g.BN_EVEN_PIXELS) and len(g.BN_EVEN_PIXELS) == 5
    # da at one pixel a channel
    rng = np.random.default_rng(0)
    for where in ('first', 'last', 'random'):
        da = g.one_hot_da(65, 75, where, rng)
        assert ((da != 0).sum(0) <= 1).all() and (da != 0).sum() >= 70
    assert g.one_hot_da(65, 3, 'first', rng)[0].all() and g.one_hot_da(65, 3, 'last', rng)[-1].all()
    # the chunk edges ask the library: one slab, exactly one, two and three
    for c in g.BN_CHUNK_CHANNELS:
        chunk, counts = g.chunk_pixels(c)
        assert chunk == -(-8192 // min(c, 64)) and counts == [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
        assert [-(-p // chunk) for p in counts] == [1, 1, 2, 3] and max(counts) < 6000
        assert [rt.bn_train_workspace_bytes(p, c) for p in counts] == [2 * n * c * 4 for n in (1, 1, 2, 3)]
    assert any(c < 64 for c in g.BN_CHUNK_CHANNELS) and any(c > 64 for c in g.BN_CHUNK_CHANNELS)
    # the rounding cases: large offsets next to small spreads, several slabs, all three forms
    assert any(-(-p // rt.bn_train_chunk(p, c)) >= 3 for p, c in g.ROUNDING_SHAPES) and any(c < 64 for _, c in g.ROUNDING_SHAPES)
    z, gamma, beta, da = g.rounding_case(1030, 75)
    assert np.abs(z.mean(0)).max() > 45 and (z.std(0) / np.abs(z.mean(0))).min() < 0.01 and (gamma < 0).any() and (gamma > 0).any()
    for pixels, c in g.ROUNDING_SHAPES:
        z, gamma, beta, da = g.rounding_case(pixels, c)
        u = ref.forward64(z, gamma, beta, 1e-3)['u']
        assert min(np.abs(u).min(), np.abs(u - 6).min()) > 1e-6 and np.abs(u).max() < 87


# ----------------------------------------------------------------------------- the device-order restatement
def test_ordered_sum_by_hand():
    """5 pixels, chunk 3, pp 2: slab 0 = pixels 0..2, lane 0 takes pixels 0 and 2, lane 1 pixel 1; slab 1 = pixels 3, 4, a lane each.
    x = (2^24, 1, 1, 1, 1): lane 0 of slab 0 = 2^24 + 1 -> 2^24 (the tie goes to even), + lane 1's 1 -> 2^24 again; slab 1 = 1 + 1 = 2;
    total 2^24 + 2.  The sequential sum stays at 2^24 (four times + 1, each lost), float64 gives 2^24 + 4.
    x = (1, 2^24, 1, 1, -2^24) in channel 1: lane 0 = 1 + 1 = 2, lane 1 = 2^24; slab 0 = 2 + 2^24 = 2^24 + 2; slab 1 = 1 - 2^24;
    1 - 2^24 is exact (2^24 - 1 fits), the total (2^24 + 2) + (1 - 2^24) = 3, as in float64.  In sequence: 1 + 2^24 -> 2^24, + 1 and + 1
    lost, - 2^24: 0."""
    big = 2.0 ** 24
    x = np.array([[big, 1], [1, big], [1, 1], [1, 1], [1, -big]], F32)
    got = ref.ordered_sum(x, 3, 2)
    assert got.dtype == F32 and got[0] == big + 2 and got[1] == 3
    seq = ref.seq_sum(x)
    assert seq[0] == big and seq[1] == 0
    assert float(x[:, 0].astype(np.float64).sum()) == big + 4 and float(x[:, 1].astype(np.float64).sum()) == 3
    # one lane, one slab: the sequential sum; starts from +0
    assert np.array_equal(ref.ordered_sum(x, 5, 1), seq) and np.array_equal(ref.ordered_sum(x, 9, 1), seq)
    assert not np.signbit(ref.ordered_sum(np.full((5, 2), -0.0, F32), 3, 2)).any()
    # chunk = 1: every slab one pixel, the slabs in index order: sequential again, whatever pp
    assert np.array_equal(ref.ordered_sum(x, 1, 4), seq)


def test_ordered_sum_equals_the_literal_loops():
    """the vectorised form against the three loops as the header words them, one float32 addition at a time"""
    def literal(x, chunk, pp):
        p, c = x.shape
        total = np.zeros(c, F32)
        for j in range(-(-p // chunk)):
            lo, hi = j * chunk, min((j + 1) * chunk, p)
            lanes = np.zeros((pp, c), F32)
            for q in range(lo, hi):
                lanes[(q - lo) % pp] = lanes[(q - lo) % pp] + x[q]
            slab = np.zeros(c, F32)
            for po in range(pp):
                slab = slab + lanes[po]
            total = total + slab
        return total
    rng = np.random.default_rng(0)
    for p, c, chunk, pp in ((1, 1, 5, 3), (17, 3, 5, 2), (100, 4, 7, 16), (1000, 5, 129, 16), (999, 2, 37, 341), (50, 3, 50, 4), (64, 2, 16, 16), (33, 1, 8, 1024)):
        x = (50 + rng.standard_normal((p, c))).astype(F32)
        assert np.array_equal(ref.ordered_sum(x, chunk, pp).view(np.uint32), literal(x, chunk, pp).view(np.uint32)), (p, c, chunk, pp)


def test_ordered_sum_against_the_other_sums():
    from tests import test_gpu_bntrain as g
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1000, 7)).astype(F32)
    for chunk in (1000, 1001, 5000):
        assert np.array_equal(ref.ordered_sum(x, chunk, 1).view(np.uint32), ref.seq_sum(x).view(np.uint32))
    # exact data: any order gives the float64 sum
    z, m, _, _, _ = g.exact_forward_case(18437, 75)
    for chunk, pp in ((128, 16), (129, 16), (2731, 341), (18437, 1)):
        s = ref.ordered_sum(z, chunk, pp)
        assert np.array_equal(s.astype(np.float64), z.astype(np.float64).sum(0)) and np.array_equal(s, m * F32(18437))
    z, _, _, da = g.exact_backward_case(1030, 3)
    assert np.array_equal(ref.ordered_sum(da, 100, 341).astype(np.float64), da.astype(np.float64).sum(0))
    # arbitrary data at a workload size: other bits than the sequential sum, and closer to float64
    from yoloret_amd import runtime as rt
    pixels, c = 43264, 75
    chunk = rt.bn_train_chunk(pixels, c)
    assert chunk == 169
    z = g.rounding_case(pixels, c)[0]
    o, s, r64 = ref.device_order(c, chunk)(z), ref.seq_sum(z), z.astype(np.float64).sum(0)
    assert np.array_equal(o.view(np.uint32), ref.ordered_sum(z, 169, 16).view(np.uint32))
    assert (o.view(np.uint32) != s.view(np.uint32)).any()
    e_o, e_s = ref.rel_err(o, r64), ref.rel_err(s, r64)
    assert e_o < e_s, (e_o, e_s)
    # the restatements with the ordered sums: the same text, another summation
    gamma, beta, da = g.rounding_case(pixels, c)[1:]
    fo, fs = ref.forward32(z, gamma, beta, sums=ref.device_order(c, chunk)), ref.forward32(z, gamma, beta)
    assert np.array_equal(fo['mean'], o / F32(pixels)) and np.array_equal(fs['mean'], s / F32(pixels))
    bo = ref.backward32(da, z, gamma, beta, fs['mean'], fs['invstd'], 'relu6', sums=ref.device_order(c, chunk))
    bs = ref.backward32(da, z, gamma, beta, fs['mean'], fs['invstd'], 'relu6')
    g32 = ref.act_grad32(da, fs['u'], 'relu6')
    assert np.array_equal(bo[2], ref.ordered_sum(g32, chunk, 16)) and np.array_equal(bs[2], ref.seq_sum(g32))
    assert ref.rel_err(bo[0], bs[0]) < 1e-4 and (bo[0].view(np.uint32) != bs[0].view(np.uint32)).any()


# ----------------------------------------------------------------------------- what tests/test_gpu_bntrain_slabs.py reaches
def _define(src, name):
    return int(re.search(r'#define %s (\d+) ' % name, src).group(1))


def test_gpu_slab_cases_reach_what_they_claim():
    from tests import test_gpu_bntrain as g, test_gpu_bntrain_slabs as s
    from yoloret_amd import runtime as rt
    src = _source()
    tile, most, min_elems, cb_max, threads = (_define(src, n) for n in ('BT_TILE', 'BT_MAX_CHUNKS', 'BT_MIN_ELEMS', 'BT_CB', 'BT_THREADS'))
    assert (tile, most, min_elems, cb_max, threads) == (128, 256, 8192, 64, 1024)
    # the table of the file, number for number
    assert s.SLAB_ROWS == [(16385, 64, 128, 129), (18437, 75, 128, 145), (32768, 64, 128, 256), (32769, 130, 129, 255), (349569, 3, 2731, 129),
                           (699137, 3, 2732, 256), (1048577, 1, 8192, 129)]
    for pixels, c, chunk, slabs in s.SLAB_ROWS:
        cb = min(c, cb_max)
        minimum = -(-min_elems // cb)
        for p in (pixels, s.next_even(pixels)):          # the exact backward runs at the next even P: the same chunk and slab count
            assert rt.bn_train_chunk(p, c) == chunk == max(minimum, -(-p // most))
            assert -(-p // chunk) == slabs and rt.bn_train_workspace_bytes(p, c) == 2 * slabs * c * 4
        assert tile < slabs <= most, 'the second BT_TILE pass of bt_slab_sum'
    rows = s.SLAB_ROWS
    pp = [threads // min(c, cb_max) for _, c, _, _ in rows]
    assert pp == [16, 16, 16, 16, 341, 341, 1024]
    assert sum(slabs == most for _, _, _, slabs in rows) >= 2 and rows[2][3] == most and rows[2][2] == min_elems // cb_max      # both tiles full
    assert rows[0][3] - tile == 1 and rows[0][0] - (rows[0][3] - 1) * rows[0][2] == 1          # one slab in the second tile; the last range one pixel
    assert rows[1][3] - tile == 17 and rows[1][1] - cb_max == 11                               # a group of 16 and a tail; a second block of 11
    p, c, chunk, slabs = rows[3]
    assert chunk > min_elems // cb_max and chunk % pp[3] and p - (slabs - 1) * chunk == 3 and c - 2 * cb_max == 2
    assert rows[2][0] + 1 == p, 'the first pixel count whose chunk is not the minimum'
    assert any(chunk % q for (_, _, chunk, _), q in zip(rows, pp))
    assert rows[4][1] < cb_max and 1024 % rows[4][1] and rows[4][2] == -(-min_elems // 3)      # the flat form with idle lanes, its minimum chunk
    assert rows[5][2] == rows[4][2] + 1 and rows[5][0] == most * rows[4][2] + 1                # the first flat count above the minimum
    assert rows[6][1] == 1 and rows[6][2] == min_elems
    assert [r[:2] for r in s.SAME_BYTES_ROWS] == [(32769, 130), (699137, 3)]
    # the exact data at these sizes: every partial sum below 2^24, the mean m exactly (the three largest rows and the widest)
    for pixels, c, _, _ in (rows[3], rows[4], rows[5], rows[6]):
        z, m, gamma, beta, moving = g.exact_forward_case(pixels, c)
        z64 = z.astype(np.float64)
        assert np.array_equal(z64.sum(0), m.astype(np.float64) * pixels) and np.abs(z64).sum(0).max() < 2 ** 24
        assert ((z64 - m[None, :]) ** 2).sum(0).max() < 2 ** 24
        assert np.array_equal(ref.forward32(z, gamma, beta)['mean'], m)
    for pixels, c in ((32770, 130), (699138, 3)):
        assert (pixels, c) in [(s.next_even(p), cc) for p, cc, _, _ in rows]
        z, gamma, beta, da = g.exact_backward_case(pixels, c)
        f = ref.forward32(z, gamma, beta, 0.0)
        assert np.all(f['var'] == 4) and np.all(f['invstd'] == 0.5) and np.all(np.abs(f['xhat']) == 1)
        for act in (None, 'relu6'):
            grad = ref.act_grad32(da, f['u'], act).astype(np.float64)
            assert np.abs(grad).sum(0).max() < 2 ** 24          # |g| <= 4, |g xhat| = |g|: every partial sum an integer below 2^24
            dz, dgamma, dbeta = ref.backward32(da, z, gamma, beta, f['mean'], f['invstd'], act)
            assert np.array_equal(dbeta.astype(np.float64), grad.sum(0)) and np.array_equal(dgamma.astype(np.float64), (grad * f['xhat']).sum(0))
    # the ordered cases: the six rounding shapes, table rows 2, 4 and 6 (counted from 1), two workload-like shapes
    assert s.ORDERED_SHAPES == g.ROUNDING_SHAPES + [(18437, 75), (32769, 130), (699137, 3), (43264, 75), (173056, 24)]
    assert s.WORKLOAD_LIKE == [(64 * 26 * 26, 75), (64 * 52 * 52, 24)]
    assert rt.bn_train_chunk(43264, 75) == 169 and -(-43264 // 169) == 256
    assert rt.bn_train_chunk(173056, 24) == 676 and -(-173056 // 676) == 256 and threads // 24 == 42 and threads - 42 * 24 == 16 and 676 % 42
    # the autograd case
    b, h, w, c = s.AUTOGRAD_SHAPE
    assert b * h * w == 16530 and c == 64 and rt.bn_train_chunk(16530, 64) == 128 and -(-16530 // 128) == 130 > tile
