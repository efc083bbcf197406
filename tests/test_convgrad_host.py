"""Host side of the backward operators (no GPU): the restatement of tests/convgrad_ref.py against hand-derived answers, the new entries
of the library, and what the case lists of tests/test_gpu_convgrad.py reach."""
import ctypes
import os

import numpy as np

from tests import convgrad_ref as ref

SOBEL = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], np.float64)      # taps [ty][tx]; a cross-correlation, as Keras computes it
X23 = np.array([[1, 2, 3], [4, 5, 6]], np.float64)


def _map(a):
    return np.asarray(a, np.float64)[None, :, :, None]


# ----------------------------------------------------------------------------- hand-derived answers
def test_linear_on_two_pixels():
    """x = [[1, 2], [3, 4]], w[co][ci] = [[1, -1], [2, 0], [0, 3]]: y = x w^T = [[-1, 2, 6], [-1, 6, 12]].  With dy = [[1, 0, 2], [0, 1, -1]]:
    dx = dy w = [1 (1, -1) + 2 (0, 3), (2, 0) - (0, 3)] = [[1, 5], [2, -3]]; dw = dy^T x = [(1, 2), (3, 4), 2 (1, 2) - (3, 4)] = [[1, 2], [3, 4], [-1, 0]]."""
    x, w, dy = [[1, 2], [3, 4]], [[1, -1], [2, 0], [0, 3]], [[1, 0, 2], [0, 1, -1]]
    for dt in (np.float64, np.float32):
        assert np.array_equal(ref.linear(x, w, dt), [[-1, 2, 6], [-1, 6, 12]])
        dx, dw = ref.linear_grads(x, w, dy, dt)
        assert np.array_equal(dx, [[1, 5], [2, -3]]) and np.array_equal(dw, [[1, 2], [3, 4], [-1, 0]])
    assert np.array_equal(ref.pack_wt(w), [[1, -1, 0, 0], [2, 0, 0, 0], [0, 3, 0, 0]])


def test_depthwise_3x3_stride_1_on_a_2x3_map():
    """'same' at stride 1: one row / column of zeros on every side, y[oy][ox] = sum x[oy - 1 + ty][ox - 1 + tx] w[ty][tx].
    x = [[1, 2, 3], [4, 5, 6]], w = [[1, 0, -1], [2, 0, -2], [1, 0, -1]]:
      y[0][0] = x01 w12 + x11 w22 = -4 - 5 = -9;  y[0][1] = (2 - 6) + (4 - 6) = -6;  y[0][2] = x01 w10 + x11 w20 = 4 + 5 = 9
      y[1][0] = x01 w02 + x11 w12 = -2 - 10 = -12;  y[1][1] = (1 - 3) + (8 - 12) = -6;  y[1][2] = 2 + 10 = 12
    dy = ones: dw[ty][tx] is the sum of the x that tap meets: [[1 + 2, 6, 2 + 3], [12, 21, 16], [4 + 5, 15, 5 + 6]];
    dx[iy][ix] is the sum of the taps that meet x[iy][ix]: rows {0, 1} (iy = 0) or {1, 2} (iy = 1) of w, both with column sums
    (3, 0, -3); columns {0, 1} at ix = 0, all at ix = 1, {1, 2} at ix = 2: dx = [[3, 0, -3], [3, 0, -3]]."""
    assert ref.geometry(2, 3, 3, 1, 'same') == ((1, 1, 1, 1), (2, 3))
    taps = SOBEL.reshape(9, 1)
    for dt in (np.float64, np.float32):
        assert np.array_equal(ref.depthwise(_map(X23), taps, 3, 1, 'same', dt)[0, :, :, 0], [[-9, -6, 9], [-12, -6, 12]])
        dx, dw = ref.depthwise_grads(_map(X23), taps, np.ones((1, 2, 3, 1)), 3, 1, 'same', dt)
        assert np.array_equal(dx[0, :, :, 0], [[3, 0, -3], [3, 0, -3]])
        assert np.array_equal(dw.reshape(3, 3), [[3, 6, 5], [12, 21, 16], [9, 15, 11]])


def test_depthwise_3x3_stride_2_on_a_2x3_map():
    """Keras 'same' at stride 2: out = ceil(n / 2) = 1 x 2.  Rows: total pad max(0 * 2 + 3 - 2, 0) = 1 -> 0 above, 1 below; columns:
    max(1 * 2 + 3 - 3, 0) = 2 -> 1 left, 1 right.  y[0][ox] = sum x[ty][2 ox - 1 + tx] w[ty][tx] (ty = 2 falls below the map):
      y[0][0] = x01 w02 + x11 w12 = -2 - 10 = -12;  y[0][1] = x01 w00 + x11 w10 = 2 + 10 = 12
    dy = [[1, 2]]: dx[iy][ix] = sum_ox dy[ox] w[iy][ix + 1 - 2 ox]: ix = 0 meets only w[iy][1] = 0; ix = 1 meets w[iy][2] (ox = 0) and
    w[iy][0] (ox = 1): (-1 + 2, -2 + 4); ix = 2 meets 2 w[iy][1] = 0: dx = [[0, 1, 0], [0, 2, 0]].
    dw[ty][tx] = sum_ox dy[ox] x[ty][2 ox - 1 + tx]: [[2 x01, x00 + 2 x02, x01], [2 x11, x10 + 2 x12, x11], 0] = [[4, 7, 2], [10, 16, 5], [0, 0, 0]].
    MobileNetV2's explicit pad gives the same geometry (that is what correct_pad is for): k // 2 - (1 - n % 2) in front, k // 2 behind."""
    assert ref.geometry(2, 3, 3, 2, 'same') == ((0, 1, 1, 1), (1, 2))
    assert ref.geometry(2, 3, 3, 2, 'mobilenet') == ((0, 1, 1, 1), (1, 2))
    assert ref.geometry(2, 3, 3, 2, (0, 1, 1, 1)) == ((0, 1, 1, 1), (1, 2))
    assert ref.mobilenet_pads(4, 5) == (1, 2, 2) and ref.same_pads(4, 5, 2) == (1, 2, 2) and ref.same_pads(5, 5, 2) == (2, 2, 3)
    taps = SOBEL.reshape(9, 1)
    dy = np.array([[1, 2]], np.float64)[None, :, :, None]
    for dt in (np.float64, np.float32):
        assert np.array_equal(ref.depthwise(_map(X23), taps, 3, 2, 'same', dt)[0, :, :, 0], [[-12, 12]])
        dx, dw = ref.depthwise_grads(_map(X23), taps, dy, 3, 2, 'mobilenet', dt)
        assert np.array_equal(dx[0, :, :, 0], [[0, 1, 0], [0, 2, 0]])
        assert np.array_equal(dw.reshape(3, 3), [[4, 7, 2], [10, 16, 5], [0, 0, 0]])


def test_geometry_matches_the_binding():
    from yoloret_amd import runtime as rt
    for h in range(1, 9):
        for w in (1, 2, 3, 7, 16, 17):
            for k in (3, 5):
                for stride in (1, 2):
                    pads, out = ref.geometry(h, w, k, stride, 'same')
                    assert rt.depthwise_geometry(h, w, k, stride, 'same') == (pads[0], pads[1]) + out
                    assert rt.depthwise_geometry(h, w, k, stride, pads) == (pads[0], pads[1]) + out
                pads, out = ref.geometry(h, w, k, 2, 'mobilenet')
                assert rt.depthwise_geometry(h, w, k, 2, pads) == (pads[0], pads[1]) + out


def test_relu6_derivative_is_zero_at_0_and_6():
    """TensorFlow's Relu6Grad passes the gradient where 0 < u < 6, both strict: at u = 0 and u = 6 exactly it is 0.  z = (0, 3, 6, -1, 7),
    scale 2, shift 0 would move them; scale 1, shift 0 keeps u = z: dz = da (0, 1, 0, 0, 0)."""
    z = np.array([[0.0], [3.0], [6.0], [-1.0], [7.0]])
    for dt in (np.float64, np.float32):
        a, u = ref.bn_act(z, [1.0], [0.0], 'relu6', dt)
        assert np.array_equal(u, z) and np.array_equal(a[:, 0], [0, 3, 6, 0, 6])
        dz = ref.bn_act_backward(np.full((5, 1), 5.0), u, [1.0], 'relu6', dt)
        assert np.array_equal(dz[:, 0], [0, 5, 0, 0, 0]) and not np.signbit(dz).any()
        # u = z scale + shift = 6 exactly with a negative scale; dz carries the scale
        a, u = ref.bn_act([[-4.0], [-2.0]], [-1.0], [2.0], 'relu6', dt)
        assert np.array_equal(u[:, 0], [6, 4])
        assert np.array_equal(ref.bn_act_backward([[3.0], [3.0]], u, [-1.0], 'relu6', dt)[:, 0], [0, -3])


def test_swish_derivative():
    """Swish(u) = u sigma(u), Swish' = sigma (1 + u (1 - sigma)): 1 / 2 at 0, -> 1 far right, -> 0 far left; at u = 1:
    0.7310586 (1 + 0.2689414) = 0.9276706."""
    import torch
    u = torch.tensor([0.0, 1.0, 40.0, -40.0], dtype=torch.float64)
    d = ref.act_prime(u, 'swish').numpy()
    assert d[0] == 0.5 and abs(d[1] - 0.9276706) < 1e-7 and abs(d[2] - 1) < 1e-12 and abs(d[3]) < 1e-12
    ut = u.clone().requires_grad_(True)
    ref._act(ut, 'swish').sum().backward()
    assert np.allclose(ut.grad.numpy(), d, rtol=1e-13, atol=1e-16)
    assert np.array_equal(ref.bn_act_backward([[4.0]], [[0.0]], [-0.5], 'swish', np.float32), [[-1.0]])
    assert np.array_equal(ref.bn_act_backward([[4.0]], [[123.0]], [0.25], None), [[1.0]])


def test_written_out_derivatives_agree_with_autograd_away_from_the_kinks():
    import torch
    rng = np.random.default_rng(0)
    z = torch.tensor(3 * rng.standard_normal((50, 7)), requires_grad=True)
    scale, shift = torch.tensor(rng.uniform(-2, 2, 7)), torch.tensor(rng.standard_normal(7))
    da = rng.standard_normal((50, 7))
    for act in (None, 'relu6', 'swish'):
        (dz,) = torch.autograd.grad(ref._bn_act(z, scale, shift, act), z, torch.tensor(da))
        u = (z * scale + shift).detach().numpy()
        assert np.allclose(ref.bn_act_backward(da, u, scale.numpy(), act), dz.numpy(), rtol=1e-12, atol=1e-15)


# ----------------------------------------------------------------------------- the library
NEW_ENTRIES = ('yr_linear_dgrad', 'yr_depthwise_forward', 'yr_depthwise_dgrad', 'yr_depthwise_wgrad_chunk', 'yr_depthwise_wgrad_workspace_bytes',
               'yr_depthwise_wgrad', 'yr_bn_act_forward', 'yr_bn_act_backward')


def test_new_entries_are_exported_under_abi_9():
    from yoloret_amd import build, runtime
    L = ctypes.CDLL(build.LIB)
    L.yr_abi_version.restype = ctypes.c_int
    assert L.yr_abi_version() == 9 == runtime.ABI_VERSION
    for sym in NEW_ENTRIES:
        getattr(L, sym)
        assert sym in runtime.EXPORTS
    assert 'convgrad.hip' in build.SOURCES
    for name in ('linear_dgrad', 'depthwise_forward', 'depthwise_dgrad', 'depthwise_wgrad', 'depthwise_wgrad_workspace_bytes', 'bn_act_forward',
                 'bn_act_backward'):
        assert callable(getattr(runtime, name))
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'yoloret_hip.h')).read()
    assert all(sym + '(' in header for sym in NEW_ENTRIES)


def test_kernels_use_no_scratch():
    from yoloret_amd import build
    rows = build.kernel_resources()['convgrad.hip']
    assert len(rows) == 5 + 3 * 4 + 2          # cg_dgrad_kernel<1..5>, three depthwise kernels x (k, stride), two BatchNorm kernels
    assert all(scratch == 0 for _, _, scratch, _, _ in rows)
    # the slab sum is the library's one stage-2 kernel, in headtrain.hip (train_common.h): no copy of it here, and it does not spill either
    assert not any('sum_kernel' in name for name, _, _, _, _ in rows)
    shared = [r for r in build.kernel_resources()['headtrain.hip'] if 'tc_slab_sum_kernel' in r[0]]
    assert len(shared) == 1 and shared[0][2] == 0


def test_depthwise_chunk_is_a_function_of_the_sizes_only():
    from yoloret_amd import runtime as rt
    for b, oh, ow, c, k in ((1, 1, 1, 1, 3), (2, 13, 13, 512, 3), (64, 13, 13, 512, 3), (64, 26, 26, 256, 5), (64, 52, 52, 128, 3), (3, 8, 9, 67, 5), (64, 208, 208, 16, 3)):
        chunk = rt.depthwise_wgrad_chunk(b, oh, ow, c, k)
        assert chunk >= 1 and chunk * ow >= 128 and chunk == rt.depthwise_wgrad_chunk(b, oh, ow, c, k)
        slabs = -(-b * oh // chunk)
        assert slabs <= 1024
        assert rt.depthwise_wgrad_workspace_bytes(b, oh, ow, c, k) == slabs * k * k * c * 4
    assert rt.depthwise_wgrad_chunk(64, 208, 208, 16, 3) == 13          # 13312 rows: more than 1024 chunks of ceil(128 / 208) = 1
    for bad in ((0, 5, 7, 8, 3), (2, 5, 7, 8, 4), (2, 0, 7, 8, 3), (2, 5, 0, 8, 3), (2, 5, 7, 0, 5)):
        assert rt.depthwise_wgrad_chunk(*bad) == 0 and rt.depthwise_wgrad_workspace_bytes(*bad) == 0


# ----------------------------------------------------------------------------- what tests/test_gpu_convgrad.py reaches
def _blocking(n, most=5):
    t = (n + 15) // 16
    blocks = (t + most - 1) // most
    return blocks, (t + blocks - 1) // blocks


def _common_blocking_rule(src):
    """convgrad.hip takes its blocking from train_common.h, where the rule ``_blocking`` restates is written once -> TC_MAX_T."""
    import re
    from yoloret_amd import build
    common = open(os.path.join(os.path.dirname(build.__file__), 'csrc', 'train_common.h')).read()
    assert 'const int t = (n + 15) / 16;' in common and '*blocks = (t + TC_MAX_T - 1) / TC_MAX_T;' in common and '*per = (t + *blocks - 1) / *blocks;' in common
    assert '#include "train_common.h"' in src and 'tc_blocking(cin, &bi, &ti);' in src and '_MAX_T - 1)' not in src
    return int(re.search(r'#define TC_MAX_T (\d+)\s', common).group(1))


def test_gpu_cases_reach_what_they_claim():
    from tests import test_gpu_convgrad as g
    from yoloret_amd import build, runtime as rt
    src = open(os.path.join(os.path.dirname(build.__file__), 'csrc', 'convgrad.hip')).read()
    assert _common_blocking_rule(src) == 5 and '#define CG_KC 64 ' in src
    assert '#define CG_DW_MIN_PIXELS 128 ' in src and '#define CG_DW_WAVES 8' in src
    # the lists that row f-9 of DESIGN.md names
    assert g.DGRAD_PIXELS == [1, 3, 15, 16, 17, 69]
    assert set(g.DGRAD_SHAPES) >= {(1, 1), (16, 16), (17, 15), (75, 75), (80, 75), (3, 256), (256, 3), (255, 255)}
    assert set(g.DW_MAPS) >= {(1, 1), (2, 3), (5, 7), (13, 13), (16, 17)} and g.DW_CHANNELS == [1, 3, 4, 5, 64, 67] and g.DW_BATCHES == [1, 3]
    assert {(k, s) for k, s, _ in g.DW_FORMS} == {(3, 1), (3, 2), (5, 1), (5, 2)} and {p for _, s, p in g.DW_FORMS if s == 2} == {'same', 'mobilenet'}
    assert g.BN_PIXELS == [1, 63, 64, 65] and g.BN_CHANNELS == [1, 75, 256]
    # linear_dgrad: every cg_dgrad_kernel<NT>, a blocked grid, one / two / more passes of 64 output channels with a whole and a
    # partial last quartet, pixel counts below, at and above a wave's 16 and above a workgroup's 64
    forms = {_blocking(cin) for cin, _ in g.DGRAD_SHAPES}
    assert {per for _, per in forms} == {1, 2, 3, 4, 5} and any(blocks > 1 for blocks, _ in forms)
    couts = {cout for _, cout in g.DGRAD_SHAPES}
    assert any(c <= 64 for c in couts) and any(64 < c <= 128 for c in couts) and any(c > 128 for c in couts)
    assert any(c % 64 == 0 for c in couts) and any(c % 4 for c in couts) and any(c % 64 and c % 4 == 0 for c in couts)
    assert any(p < 16 for p in g.DGRAD_PIXELS) and 16 in g.DGRAD_PIXELS and 17 in g.DGRAD_PIXELS and any(p > 64 and p % 16 for p in g.DGRAD_PIXELS)
    # depthwise: odd and even sizes at stride 2 (the asymmetric pad on both sides), maps smaller than the kernel, one and two
    # channel blocks of 64, a partial block
    assert any(h % 2 == 0 and w % 2 for h, w in g.DW_MAPS) and any(h % 2 and w % 2 for h, w in g.DW_MAPS) and any(w % 2 == 0 for _, w in g.DW_MAPS)
    assert any(ref.geometry(h, w, 3, 2, 'same')[0][0] != ref.geometry(h, w, 3, 2, 'same')[0][2] for h, w in g.DW_MAPS)
    # the stride-1 kernels give a lane 4 consecutive columns: widths below 4 and every residue of 4, the last quartet whole and partial
    assert '#define CG_DW_NX 4 ' in src and {w % 4 for _, w in g.DW_MAPS} == {0, 1, 2, 3} and any(w < 4 for _, w in g.DW_MAPS) and any(w > 8 for _, w in g.DW_MAPS)
    assert (1, 1) in g.DW_MAPS and 64 in g.DW_CHANNELS and any(c > 64 and c % 64 for c in g.DW_CHANNELS)
    # the weight gradient's chunk cases ask the library: one slab, exactly one, two with one row, three with one row
    chunk, rows = g.dw_chunk_rows()
    assert chunk == -(-128 // g.DW_CHUNK_OW) and rows == [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    assert [-(-r // chunk) for r in rows] == [1, 1, 2, 3] and [-(-2 * r // chunk) for r in rows] == [2, 2, 3, 5]
    assert all((r * g.DW_CHUNK_OW) % 8 for r in rows[:3])          # the eight waves get unequal shares
    # BatchNorm: element counts below, at and above the 256 lanes of a workgroup, ties in every case that has room for two
    counts = sorted(p * c for p in g.BN_PIXELS for c in g.BN_CHANNELS)
    assert counts[0] == 1 and 256 in counts and any(n < 256 for n in counts) and any(n > 256 and n % 256 for n in counts)
    for p in g.BN_PIXELS:
        for c in g.BN_CHANNELS:
            z, scale, shift, _ = g.bn_exact_case(p, c)
            u = z.astype(np.float64) * scale + shift
            assert (u == 0).any() and ((u == 6).any() or p * c == 1)
            assert np.array_equal(u, (z * scale + shift).astype(np.float64)), 'u is exact in float32'


# ----------------------------------------------------------------------------- what tests/test_gpu_convgrad_forms.py reaches
def test_gpu_form_cases_reach_what_they_claim():
    import re
    from tests import test_gpu_convgrad_forms as f
    from yoloret_amd import build, runtime as rt
    src = open(os.path.join(os.path.dirname(build.__file__), 'csrc', 'convgrad.hip')).read()
    most, min_pixels = (int(re.search(r'#define %s (\d+)\s' % n, src).group(1)) for n in ('CG_DW_MAX_CHUNKS', 'CG_DW_MIN_PIXELS'))
    max_t = _common_blocking_rule(src)
    assert (most, min_pixels, max_t) == (1024, 128, 5)
    # the depthwise table, number for number
    assert f.DW_BIG == [((1, 1024, 128, 5, 3, 1, 'same'), 1, 1024), ((1, 1025, 128, 5, 3, 1, 'same'), 2, 513), ((5, 205, 128, 5, 5, 1, 'same'), 2, 513),
                        ((3, 1366, 128, 5, 5, 2, 'mobilenet'), 3, 683), ((3, 1366, 128, 5, 3, 2, 'same'), 3, 683),
                        ((1, 1025, 128, 67, 3, 1, 'same'), 2, 513)]
    out = {}
    for shape, chunk, chunks in f.DW_BIG:
        b, h, w, c, k, stride, padding = shape
        pads, (oh, ow) = ref.geometry(h, w, k, stride, padding)
        rows = b * oh
        minimum = -(-min_pixels // ow)
        assert rt.depthwise_wgrad_chunk(b, oh, ow, c, k) == chunk == max(minimum, -(-rows // most))
        assert -(-rows // chunk) == chunks <= most and rt.depthwise_wgrad_workspace_bytes(b, oh, ow, c, k) == chunks * k * k * c * 4
        assert 16 * b * oh * ow < 2 ** 24, 'integers in [-4, 4]: every partial sum is exact'
        assert b <= 65535 and h <= 65535 and oh <= 65535
        out[shape] = (oh, ow, rows, minimum)
    first, second, third, fourth, fifth, sixth = (s for s, _, _ in f.DW_BIG)
    assert out[first][2:] == (most, 1) and f.DW_BIG[0][2] == most                    # the most chunks the minimum allows: the last size of that branch
    assert out[second][2] == most + 1 and f.DW_BIG[1][1] > out[second][3]            # one row more: the `most` branch
    assert out[second][2] - (f.DW_BIG[1][2] - 1) * f.DW_BIG[1][1] == 1               # the last chunk one row
    assert all(chunk > out[s][3] for s, chunk, _ in f.DW_BIG[1:]), 'every shape but the first runs the `most` branch'
    oh, chunk = out[third][0], f.DW_BIG[2][1]                                        # 205 rows an image, chunk 2: chunk 102 = rows 204 (image 0), 205 (image 1)
    assert oh == 205 and 102 * chunk < oh < 103 * chunk
    for s in (fourth, fifth):
        oh, ow, rows, minimum = out[s]
        assert (oh, ow, rows, minimum) == (683, 64, 2049, 2) and oh % 3 and any(j * 3 < oh < (j + 1) * 3 for j in range(683))
    assert ref.geometry(1366, 128, 5, 2, 'mobilenet')[0] == ref.geometry(1366, 128, 5, 2, 'same')[0]          # even sizes: the same pads
    assert {(s[4], s[5]) for s in out} == {(3, 1), (5, 1), (5, 2), (3, 2)}           # all four instantiations of the partial kernel
    assert sixth[3] > 64 and sixth[3] % 64, 'two channel blocks, the second partial'
    assert f.DW_SAME_BYTES == f.DW_BIG[1]
    # the test's own tensors reach the largest |dw| the bound allows for: below 2^24
    x, taps, dy, y64, dx64, dw64 = f._big_case(second)
    assert np.abs(dw64).max() < 2 ** 24 and np.abs(y64).max() <= 16 * 9 and np.abs(dx64).max() <= 16 * 9
    # yr_linear_dgrad: the blockings and their wholly empty tiles
    assert f.DGRAD_CIN == [96, 97, 144, 161, 200] and f.DGRAD_COUT == [3, 75] and f.DGRAD_PIXELS == [69, 4161]
    for cin in f.DGRAD_CIN:
        blocks, per = _blocking(cin, max_t)
        assert (blocks, per) == f.DGRAD_BLOCKINGS[cin]
        assert blocks * per - (cin + 15) // 16 == f.DGRAD_EMPTY_TILES[cin]
    assert [f.DGRAD_BLOCKINGS[c] for c in f.DGRAD_CIN] == [(2, 3), (2, 4), (2, 5), (3, 4), (3, 5)]
    assert [f.DGRAD_EMPTY_TILES[c] for c in f.DGRAD_CIN] == [0, 1, 1, 1, 2]
    assert [(c + 15) // 16 for c in f.DGRAD_CIN] == [6, 7, 9, 11, 13]
    from tests import test_gpu_convgrad as g
    assert all(_blocking(cin, max_t)[0] * _blocking(cin, max_t)[1] == (cin + 15) // 16 for cin, _ in g.DGRAD_SHAPES), 'the older cases fill their blocks'
    assert any(c % 16 == 0 for c in f.DGRAD_CIN) and any(c % 16 == 1 for c in f.DGRAD_CIN) and any(c % 4 for c in f.DGRAD_CIN)
    assert any(c <= 64 and c % 4 for c in f.DGRAD_COUT) and any(c > 64 for c in f.DGRAD_COUT)
    assert any(p % 64 and p > 64 for p in f.DGRAD_PIXELS) and max(f.DGRAD_PIXELS) > 64 * 64
