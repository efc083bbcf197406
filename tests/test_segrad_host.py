"""Host side of the squeeze-excite block (no GPU): the restatements of tests/segrad_ref.py against literal lane-by-lane ones and against
torch's float64 autograd, the new entries of the library and their two size functions, what the case lists of tests/test_gpu_segrad.py
reach, and what the cases of tests/test_gpu_segrad_autograd.py and tests/test_gpu_head_block.py rest on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import layers_ref as lr, segrad_ref as ref, selayers_ref as sl

F32 = np.float32
EPS24 = 2.0 ** -24
NEW_ENTRIES = ('yr_se_chunk', 'yr_se_workspace_bytes', 'yr_se_forward', 'yr_se_backward')


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ----------------------------------------------------------------------------- the documented orders, literally
def test_pixel_sum_is_the_stated_order():
    """a range's pixels dealt to PP lanes a channel in turn, a lane's terms from +0 in pixel order, the lanes in order from +0, the
    ranges in order from +0 - lane by lane"""
    def literal(img, chunk, pp):
        n, c = img.shape
        total = np.zeros(c, F32)
        for p0 in range(0, n, chunk):
            lanes = np.zeros((pp, c), F32)
            for p in range(p0, min(p0 + chunk, n)):
                lanes[(p - p0) % pp] = lanes[(p - p0) % pp] + img[p]
            slab = np.zeros(c, F32)
            for po in range(pp):
                slab = slab + lanes[po]
            total = total + slab
        return total
    rng = np.random.default_rng(0)
    for b, n, c, chunk in ((1, 1, 1, 4096), (2, 35, 3, 1366), (2, 300, 75, 108), (3, 250, 130, 94), (1, 700, 32, 128), (2, 169, 96, 86)):
        t = (1 + rng.standard_normal((b, n, c))).astype(F32)
        want = np.stack([literal(img, chunk, ref.pp_of(c)) for img in t])
        assert np.array_equal(_bits(ref.pixel_sum32(t, chunk)), _bits(want)), (b, n, c, chunk)
    assert [ref.cb_of(c) for c in (1, 3, 64, 65, 75, 96, 128, 130, 512, 672)] == [1, 3, 64, 33, 38, 48, 64, 44, 64, 62]
    assert [ref.pp_of(c) for c in (1, 3, 64, 75, 96, 130)] == [256, 85, 4, 6, 5, 5]
    # 2^24 + 1 + 1 + ... stays at 2^24 sequentially and within a range (the lanes are added in order); the ones of a second range are
    # added among themselves first
    t = np.ones((1, 9, 1), F32)
    t[0, 0, 0] = 2.0 ** 24
    assert ref.pixel_sum32(t, None)[0, 0] == 2.0 ** 24 == ref.pixel_sum32(t, 4096)[0, 0] and ref.pixel_sum32(t, 5)[0, 0] == 2.0 ** 24 + 4


def test_fc_and_fct_are_the_stated_orders():
    def fc_literal(v, w, bias, threads=1024):
        i_n, o_n = w.shape
        ol = min(o_n, threads)
        ks = threads // ol
        sl_ = -(-i_n // ks)
        out = np.empty(o_n, F32)
        for o in range(o_n):
            parts = []
            for k in range(ks):
                acc = F32(0)
                for i in range(k * sl_, min((k + 1) * sl_, i_n)):
                    acc = F32(acc + F32(v[i] * w[i, o]))
                parts.append(acc)
            s = bias[o]
            for part in parts:
                s = F32(s + part)
            out[o] = s
        return out

    def fct_literal(v, w):
        o_n, i_n = w.shape
        out = np.empty(o_n, F32)
        for o in range(o_n):
            lanes = np.zeros(64, F32)
            for i in range(i_n):
                lanes[i % 64] = F32(lanes[i % 64] + F32(v[i] * w[o, i]))
            for off in (32, 16, 8, 4, 2, 1):
                lanes = np.array([F32(lanes[lane] + lanes[lane ^ off]) for lane in range(64)], F32)
            assert np.all(_bits(lanes) == _bits(lanes)[0]), 'every lane of the butterfly holds the same bits'
            out[o] = lanes[0]
        return out
    rng = np.random.default_rng(1)
    for i_n, o_n in ((1, 1), (3, 1), (75, 33), (130, 4), (33, 130), (200, 300), (7, 1100)):
        v, w, bias = (rng.standard_normal(s).astype(F32) for s in ((2, i_n), (i_n, o_n), (o_n,)))
        got = ref.fc32(v, w, bias)
        for b in range(2):
            assert np.array_equal(_bits(got[b]), _bits(fc_literal(v[b], w, bias))), ('fc', i_n, o_n)
        got = ref.fct32(v, w.T.copy())
        for b in range(2):
            assert np.array_equal(_bits(got[b]), _bits(fct_literal(v[b], w.T))), ('fct', i_n, o_n)
    # the batch sums: the first term image 0's own, so a sum of -0 alone stays -0
    assert _bits(ref.batch_sum32(np.full((1, 1), -0.0, F32)))[0] == 0x80000000 and ref.batch_sum32(np.array([[2.0 ** 24], [1], [1]], F32))[0] == 2.0 ** 24


def test_float64_version_equals_torch_autograd():
    """forward64 / backward64 (the header's formulas) against torch-CPU float64 autograd of mean -> matmul + bias -> x sigmoid(x) ->
    matmul + bias -> sigmoid -> multiply, for y and all five gradients"""
    for b, h, w, c, r in ((1, 1, 1, 1, 1), (2, 2, 3, 3, 4), (3, 7, 5, 75, 33), (2, 13, 13, 130, 4)):
        x, dy, w1, b1, w2, b2 = ref.se_case(b, h, w, c, r)
        f = ref.forward64(x, w1, b1, w2, b2)
        g = ref.backward64(dy, x, w1, w2, f['m'], f['z1'], f['g'])
        t = ref.grads_torch(x, w1, b1, w2, b2, dy)
        assert ref.rel_err(f['y'], t['y']) < 1e-14
        for k in ('dx', 'dw1', 'db1', 'dw2', 'db2'):
            assert g[k].shape == t[k].shape and ref.rel_err(g[k], t[k]) < 1e-13, (k, ref.rel_err(g[k], t[k]))
        # and the float32 restatements, in either order, stay within a few float32 roundings of it
        f32 = ref.forward32(x, w1, b1, w2, b2)
        g32 = ref.backward32(dy, x, w1, w2, f32['m'], f32['z1'], f32['g'])
        fd = ref.forward32(x, w1, b1, w2, b2, 64)
        gd = ref.backward32(dy, x, w1, w2, fd['m'], fd['z1'], fd['g'], 64)
        for k in ('dx', 'dw1', 'db1', 'dw2', 'db2'):
            assert ref.rel_err(g32[k], t[k]) < 2e-6 and ref.rel_err(gd[k], t[k]) < 2e-6, k


def test_pinned_sigmoid_is_within_two_ulp_of_libm():
    u = np.linspace(-30, 30, 2001).astype(F32)
    s = ref.sigmoid32(u)
    assert s.dtype == F32 and np.max(np.abs(s.astype(np.float64) - 1 / (1 + np.exp(-u.astype(np.float64)))) / np.spacing(s)) < 2.5


# ----------------------------------------------------------------------------- the library
def _lib():
    from yoloret_amd import runtime as rt
    return ctypes.CDLL(rt.LIB_PATH)


def _source():
    from yoloret_amd import build
    return open(os.path.join(build.CSRC, 'segrad.hip')).read()


def _define(src, name):
    return int(re.search(r'#define %s (\d+) ' % name, src).group(1))


def test_entries_are_exported_and_bound():
    from yoloret_amd import autograd, build, runtime as rt
    lib = _lib()
    header = open(os.path.join(build.HERE, '..', 'include', 'yoloret_hip.h')).read()
    for name in NEW_ENTRIES:
        assert getattr(lib, name) is not None and name in rt.EXPORTS and re.search(r'\b%s\(' % name, header), name
    assert 'segrad.hip' in build.SOURCES and lib.yr_abi_version() == 9 == rt.ABI_VERSION
    for name in ('se_forward', 'se_backward', 'se_chunk', 'se_workspace_bytes'):
        assert callable(getattr(rt, name)) and getattr(rt, name).__doc__
    for name in ('squeeze_excite', 'head_block', 'head_block_parameters'):
        assert callable(getattr(autograd, name)) and getattr(autograd, name).__doc__
    assert autograd.HEAD_BLOCKS == ('td1', 'td2', 'td3', 'bu3', 'bu2', 'bu1') and (autograd.HEAD_BN_MOMENTUM, autograd.HEAD_BN_EPS) == (0.99, 1e-3)


def test_no_kernel_of_the_file_uses_scratch():
    from yoloret_amd import build
    build.build()
    rows = build.kernel_resources()['segrad.hip']
    assert len(rows) == 7 and all(scratch == 0 for _, _, scratch, _, _ in rows), rows


def test_chunk_rule_slab_cap_workspace_and_refusals():
    from yoloret_amd import runtime as rt
    src = _source()
    min_elems, most, threads, cb, fc_threads = (_define(src, n) for n in ('SE_MIN_ELEMS', 'SE_MAX_CHUNKS', 'SE_THREADS', 'SE_CB', 'SE_FC_THREADS'))
    assert (min_elems, most, threads, cb, fc_threads) == (4096, 16, 256, 64, 1024)
    assert (threads, cb, fc_threads) == (ref.SE_THREADS, ref.SE_CB, ref.SE_FC_THREADS)
    assert (_define(src, 'SE_MAX_C'), _define(src, 'SE_MAX_R')) == (4096, 1024)
    for c in (1, 3, 32, 64, 65, 75, 96, 130, 512, 672, 3840, 4096):
        minimum = -(-min_elems // ref.cb_of(c))
        for n in (1, minimum - 1, minimum, minimum + 1, 2 * minimum + 1, most * minimum, most * minimum + 1, 10 * most * minimum + 7):
            if n < 1:
                continue
            chunk = rt.se_chunk(1, n, c)
            assert chunk == max(minimum, -(-n // most)) == rt.se_chunk(64, n, c), (n, c)          # (the batch is checked, not used)
            slabs = -(-n // chunk)
            assert slabs <= most
            for b, r in ((1, 1), (3, 33), (64, 1024)):
                assert rt.se_workspace_bytes(b, n, c, r) == 4 * (b * slabs * c + 2 * b * c + 2 * b * r), (b, n, c, r)
    # the two shapes the constants were chosen at, 64 images: 8 x 3 x 64 and 2 x 16 x 64 workgroups
    assert rt.se_chunk(64, 13 * 13, 512) == 64 and rt.se_chunk(64, 52 * 52, 128) == 169 and rt.se_chunk(64, 104 * 104, 96) == 676
    assert rt.se_chunk(1, (1 << 40) - 1, 1) == -(-((1 << 40) - 1) // 16) and rt.se_chunk((1 << 31) - 1, 1, 8) == 512
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, -5, 8), (1, 8, 0), (1, 8, -3), (1, 8, 4097), (1, 1 << 40, 8), (1 << 20, 1 << 20, 8), (3, (1 << 39), 8)):
        assert rt.se_chunk(*bad) == 0 and rt.se_workspace_bytes(*bad, 2) == 0, bad
    for r in (0, -1, 1025):
        assert rt.se_workspace_bytes(2, 48, 8, r) == 0 and rt.se_chunk(2, 48, 8) == 512


def test_gpu_case_lists_reach_what_they_claim():
    from tests import test_gpu_segrad as g
    from yoloret_amd import runtime as rt
    src = _source()
    assert (g.SE_MIN_ELEMS, g.SE_MAX_CHUNKS) == (_define(src, 'SE_MIN_ELEMS'), _define(src, 'SE_MAX_CHUNKS'))
    assert g.SE_SHAPES == [(1, 1), (2, 3), (7, 5), (13, 13)] and g.SE_CHANNELS == [1, 3, 32, 75, 130] and g.SE_REDUCED == [1, 4, 33] and g.SE_BATCHES == [1, 3]
    for c in g.SE_CHANNELS:
        minimum = g.se_min_chunk(c)
        counts = g.se_pixels(c)
        assert counts == [minimum - 1, minimum, minimum + 1, 2 * minimum + 1]
        assert [rt.se_chunk(2, p, c) for p in counts] == [minimum] * 4, 'the minimum sets every chunk of the list'
        assert [-(-p // minimum) for p in counts] == [1, 1, 2, 3] and counts[-1] - 2 * minimum == 1, 'one range, one full range, two, three with a last range of one pixel'
    assert [g.se_min_chunk(c) for c in g.SE_CHANNELS] == [4096, 1366, 128, 108, 94]
    # the shape list at 13 x 13: one range for C = 1 and 3, two for the others; one, two and three channel blocks; fewer pixels than lanes a channel (C = 1, 3)
    assert [-(-169 // g.se_min_chunk(c)) for c in g.SE_CHANNELS] == [1, 1, 2, 2, 2] and [-(-c // 64) for c in g.SE_CHANNELS] == [1, 1, 1, 2, 3]
    assert ref.pp_of(1) > 169 > ref.pp_of(3) > 35 and rt.se_chunk(3, 13 * 13, 130) == 94
    # the branch where the slab cap sets the chunk
    b, h, w, c, r = g.WORKLOAD_LIKE
    assert rt.se_chunk(b, h * w, c) == -(-h * w // g.SE_MAX_CHUNKS) == 69 > g.se_min_chunk(c) == 64 and -(-h * w // 69) == 16 and h * w - 15 * 69 == 54
    assert h * w > g.SE_MAX_CHUNKS * g.se_min_chunk(c) >= 32 * 32, 'the first square map in that branch'
    # the model's widths: several channel blocks, the fc kernels' tiles and slices
    assert g.MODEL_WIDTHS == [(2, 13, 13, 512, 128), (2, 13, 13, 672, 28)]
    assert [ref.cb_of(c) for c in (512, 672)] == [64, 62] and [rt.se_chunk(2, 169, c) for c in (512, 672)] == [64, 67]
    # integers stay exact at the largest sizes: every partial sum below 2^24
    for shape in [g.WORKLOAD_LIKE, (2, 1, g.se_pixels(1)[-1], 1, 4)] + g.MODEL_WIDTHS:
        x, dy = ref.se_case(*shape, exact=True)[:2]
        assert np.abs(x).sum(axis=(1, 2)).max() < 2 ** 24 and np.abs(dy.astype(np.float64) * x).sum(axis=(1, 2)).max() < 2 ** 24


# ----------------------------------------------------------------------------- what the layer cases rest on
def _bar(what, got, r32, r64):
    e_dev, e_ref = ref.rel_err(got, r64), ref.rel_err(r32, r64)
    print('%s: float32 chain %.3e, float32 oracle %.3e, bar %.3e' % (what, e_dev, e_ref, 4 * e_ref + EPS24))
    return e_dev <= 4 * e_ref + EPS24


@pytest.mark.parametrize('case', sl.SE_BLOCKS, ids=sl.SE_BLOCK_IDS)
def test_se_block_cases_rest_on_agreeing_oracles(case):
    """EfficientNet's block with se_ratio 0.25 and Swish: the NumPy and the torch oracle agree in float64, and no Swish or sigmoid sees
    |u| >= 87 (the clamp of the pinned exp)"""
    name, k, s, e, cin, cout = case[:6]
    x, f = lr.block_inputs(case)
    P = lr.fresh_store()
    y64 = sl.numpy_se_block(P, case, x, np.float64)
    t64 = sl.torch_se_block(P, case, x, torch.float64, f)
    assert ref.rel_err(t64['y'], y64) < 1e-12
    c, r = cin * e, sl.reduced(cin)
    assert (c, r) in ((32, 8), (96, 4), (144, 6)) and t64['_se_reduce'].shape == (1, 1, c, r) and t64['_se_expand/bias'].shape == (c,)
    us = sl.preacts(P, name, x, k, s, e, cin, np.float64)
    assert len(us) == (4 if e != 1 else 3) and max(float(np.abs(u).max()) for _, u in us) < 87.0
    assert all(np.abs(t64[key]).max() > 0 for key in ('x', '_dw', '_se_reduce', '_se_reduce/bias', '_se_expand', '_se_expand/bias', '_project'))


@pytest.mark.parametrize('case', sl.HEAD_CASES, ids=sl.HEAD_IDS)
def test_head_block_cases_rest_on_agreeing_oracles(case):
    """the head block on 2 images at 12 x 12: the two oracles agree in float64; a float32 chain on the CPU meets the bar the device is
    held to; the ReLU6 inputs stay off their kinks by ``layers_ref.relu6_margins``; |u| < 87 before every Swish and sigmoid"""
    model_name, name, cin, _ = case
    x, f1, f2 = sl.head_inputs(case)
    P = sl.head_store(case)
    assert P.values[name + '_conv/kernel'].shape == (1, 1, cin, sl.HEAD_F) and sl.HEAD_O == 75
    n64 = sl.numpy_head(P, name, x, np.float64)
    t64, t32 = sl.torch_head(P, name, x, torch.float64, f1, f2), sl.torch_head(P, name, x, torch.float32, f1, f2)
    assert ref.rel_err(t64['x_out'], n64[0]) < 1e-12 and ref.rel_err(t64['y'], n64[1]) < 1e-12
    xo, y = sl.host_head(P.values, name, x)
    assert _bar('%s %s x_out' % case[:2], xo, t32['x_out'], t64['x_out']) and _bar('%s %s y' % case[:2], y, t32['y'], t64['y'])
    us64, us32 = sl.head_preacts(P, name, x, np.float64), sl.head_preacts(P, name, x, np.float32)
    assert [w.split(' ')[0] for w, _ in us64] == ['ReLU6', 'Swish', 'Swish', 'sigmoid']
    for where, distance, margin in lr.relu6_margins([(w.split(' of ')[1], u) for w, u in us64[:1]], [(w.split(' of ')[1], u) for w, u in us32[:1]]):
        print('%s %s %s: smallest distance %.3e, margin %.3e' % (case[0], name, where, distance, margin))
        assert distance > margin, 'a kink lies too close - choose another seed'
    assert max(float(np.abs(u).max()) for _, u in us64[1:]) < 87.0
    assert all(np.abs(t64[key]).max() > 0 for key in sl.head_kernels(name) + ('x',))
    assert ('_y' in sl.head_kernels(name)) == (name + '_y/kernel' in lr.product_net(model_name, P.values).get_weights()) == (name == 'bu3')


def test_training_case_rests_on_its_margins():
    """bu3 of MobileNetV2 x0.75 with BatchNorm on the statistics of the batch (tests/selayers_ref.train_head on the parameters of
    ``autograd.head_block_parameters``, here on the CPU): ReLU6's inputs stay off the kinks by the rule of ``relu6_margins``, |u| < 87
    before the Swish, every trained tensor has a gradient, the pad columns' is 0"""
    from yoloret_amd import autograd as ag
    case = sl.HEAD_TRAIN_CASE
    x, f1, f2 = sl.head_inputs(case)
    par = ag.head_block_parameters(lr.product_net(case[0], sl.head_store(case).values), case[1], 'cpu')
    assert sorted(k for k, v in par.items() if k != 'name' and v.requires_grad) == sorted(sl.HEAD_TRAINED)
    host = {k: v.detach().numpy() for k, v in par.items() if k != 'name'}
    t64, t32 = sl.train_head(host, x, f1, f2, 'float64'), sl.train_head(host, x, f1, f2, 'float32')
    for where, distance, margin in lr.relu6_margins([('_conv_BN', t64['u']['_conv_BN'])], [('_conv_BN', t32['u']['_conv_BN'])]):
        print('training %s: smallest distance %.3e, margin %.3e' % (where, distance, margin))
        assert distance > margin, 'a kink lies too close - choose another seed'
    assert float(np.abs(t64['u']['_mb_dw_BN']).max()) < 87.0
    for key in sl.HEAD_TRAINED:
        assert np.abs(t64[key]).max() > 0 and ref.rel_err(t32[key], t64[key]) < 1e-5, key
    assert not t64['_conv'][:, 75:].any() and host['_conv'].shape == (128, 76)
