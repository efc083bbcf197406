"""Host side of the 3 x 3 entry-convolution operators (no GPU): the restatement of tests/stemgrad_ref.py against the oracle and torch, the
new entries of the library, their refusals, and what the case lists of tests/test_gpu_stemgrad.py reach."""
import ctypes
import os
import re

import numpy as np

from tests import stemgrad_ref as ref

CASES = [(2, 7, 9, 3, 24, 2, 'same'), (1, 8, 8, 4, 5, 1, 'same'), (3, 9, 7, 1, 8, 2, (0, 0, 1, 1)), (2, 2, 3, 3, 64, 2, 'same'), (1, 1, 1, 3, 24, 1, 'same'),
         (2, 6, 5, 2, 27, 1, (0, 0, 1, 1)), (1, 20, 33, 3, 40, 2, 'same')]      # (b, h, w, cin, cout, stride, padding)


def _data(seed, b, h, w, cin, cout, stride, padding, ints=False):
    rng = np.random.default_rng(seed)
    _, (oh, ow) = ref.geometry(h, w, stride, padding)
    draw = (lambda s: rng.integers(-4, 5, s).astype(np.float32)) if ints else (lambda s: rng.standard_normal(s).astype(np.float32))
    return draw((b, h, w, cin)), draw((9 * cin, cout)), draw((b, oh, ow, cout))


# ----------------------------------------------------------------------------- the restatement
def test_float64_restatement_is_the_oracles_and_torchs_convolution():
    import torch
    import torch.nn.functional as F
    from oracle import nn
    for i, (b, h, w, cin, cout, stride, padding) in enumerate(CASES):
        x, wt, dy = _data(i, b, h, w, cin, cout, stride, padding)
        pads, _ = ref.geometry(h, w, stride, padding)
        y64 = ref.forward64(x, wt, stride, padding)
        dx64, dw64 = ref.grads64(x, wt, dy, stride, padding)
        if padding == 'same':
            assert np.allclose(nn.conv2d(x.astype(np.float64), wt.reshape(3, 3, cin, cout).astype(np.float64), stride, 'same'), y64, rtol=0, atol=1e-13)
        xt, wtt = torch.tensor(x, dtype=torch.float64, requires_grad=True), torch.tensor(wt, dtype=torch.float64, requires_grad=True)
        xp = F.pad(xt.permute(0, 3, 1, 2), (pads[1], pads[3], pads[0], pads[2]))
        yt = F.conv2d(xp, wtt.reshape(3, 3, cin, cout).permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)
        gx, gw = torch.autograd.grad(yt, (xt, wtt), torch.tensor(dy, dtype=torch.float64))
        for got, want in ((yt.detach().numpy(), y64), (gx.numpy(), dx64), (gw.numpy(), dw64)):
            assert got.shape == want.shape and np.allclose(got, want, rtol=0, atol=1e-12)


def test_float32_restatement_follows_the_float64_one():
    """standard-normal data: within a few float32 roundings of float64; integers in [-4, 4]: every partial sum is exact, so the
    ordered float32 chains must give the float64 result bit for bit - the order can change nothing, a wrong index would"""
    for i, (b, h, w, cin, cout, stride, padding) in enumerate(CASES):
        x, wt, dy = _data(i, b, h, w, cin, cout, stride, padding)
        y64 = ref.forward64(x, wt, stride, padding)
        dx64, dw64 = ref.grads64(x, wt, dy, stride, padding)
        for got, want in ((ref.forward32(x, wt, stride, padding), y64), (ref.dgrad32(dy, wt, (h, w), stride, padding), dx64), (ref.wgrad32(x, dy, stride, padding), dw64)):
            assert got.dtype == np.float32 and ref.rel_err(got, want) < 2e-6
        x, wt, dy = _data(i, b, h, w, cin, cout, stride, padding, ints=True)
        assert np.array_equal(ref.forward32(x, wt, stride, padding), ref.forward64(x, wt, stride, padding))
        dx64, dw64 = ref.grads64(x, wt, dy, stride, padding)
        assert np.array_equal(ref.dgrad32(dy, wt, (h, w), stride, padding), dx64) and np.array_equal(ref.wgrad32(x, dy, stride, padding), dw64)


def test_a_padded_tap_is_skipped():
    """1 x 1 map, stride 1, 'same': only the centre tap (t = 4) meets the map.  x = -1 / 4 and w[4] = 2^-149: the product, -2^-151, rounds to
    -0.  The taps 5..8 are padded: an fmaf with a padded zero would compute +0 * 1 + -0 = +0; skipped, the chain keeps its -0.
    And an input pixel no window reaches - row and column 5 of a 6 x 6 map at stride 2 without padding - gets +0."""
    x = np.full((1, 1, 1, 1), -0.25, np.float32)
    wt = np.ones((9, 1), np.float32)
    wt[4, 0] = np.float32(2.0 ** -149)
    y = ref.forward32(x, wt, 1, 'same')
    assert y.shape == (1, 1, 1, 1) and y[0, 0, 0, 0] == 0 and np.signbit(y[0, 0, 0, 0])
    dx = ref.dgrad32(np.ones((1, 2, 2, 1), np.float32), np.ones((9, 1), np.float32), (6, 6), 2, (0, 0, 0, 0))
    assert np.array_equal(dx[0, 5, :, 0], np.zeros(6)) and np.array_equal(dx[0, :, 5, 0], np.zeros(6)) and not np.signbit(dx).any()
    assert dx[0, 2, 2, 0] == 4 and dx[0, 0, 0, 0] == 1


# ----------------------------------------------------------------------------- the library
NEW_ENTRIES = ('yr_conv3x3_forward', 'yr_conv3x3_dgrad', 'yr_conv3x3_wgrad_chunk', 'yr_conv3x3_wgrad_workspace_bytes', 'yr_conv3x3_wgrad')


def test_new_entries_are_exported_under_abi_9():
    from yoloret_amd import autograd, build, runtime
    L = ctypes.CDLL(build.LIB)
    L.yr_abi_version.restype = ctypes.c_int
    assert L.yr_abi_version() == 9 == runtime.ABI_VERSION
    for sym in NEW_ENTRIES:
        getattr(L, sym)
        assert sym in runtime.EXPORTS
    assert 'stemgrad.hip' in build.SOURCES
    for name in ('conv3x3_forward', 'conv3x3_dgrad', 'conv3x3_wgrad', 'conv3x3_wgrad_chunk', 'conv3x3_wgrad_workspace_bytes'):
        assert callable(getattr(runtime, name))
    assert callable(autograd.conv3x3)
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'yoloret_hip.h')).read()
    assert all(sym + '(' in header for sym in NEW_ENTRIES)


def test_kernels_use_no_scratch():
    from yoloret_amd import build
    rows = build.kernel_resources()['stemgrad.hip']
    assert len(rows) == 9 + 2 * 9 + 1          # forward and dgrad (x 2 strides): cout 8, 16, .., 64 and the guarded form; one wgrad kernel
    assert all(scratch == 0 for _, _, scratch, _, _ in rows)


def test_chunk_is_a_function_of_the_sizes_only():
    from yoloret_amd import runtime as rt
    for b, oh, ow, cin, cout in ((1, 1, 1, 1, 1), (64, 208, 208, 3, 24), (64, 208, 208, 3, 48), (3, 8, 9, 4, 64), (1, 2049, 256, 1, 4), (2, 12, 16, 3, 24)):
        chunk = rt.conv3x3_wgrad_chunk(b, oh, ow, cin, cout)
        assert chunk == ref.wgrad_chunk(b, oh, ow) == rt.conv3x3_wgrad_chunk(b, oh, ow, cin, cout) and chunk * ow >= 256
        slabs = -(-b * oh // chunk)
        assert slabs <= 2048 and rt.conv3x3_wgrad_workspace_bytes(b, oh, ow, cin, cout) == slabs * 9 * cin * cout * 4
    assert rt.conv3x3_wgrad_chunk(64, 208, 208, 3, 24) == 7          # 13312 rows: more than 2048 chunks of ceil(256 / 208) = 2
    for bad in ((0, 5, 7, 3, 24), (2, 0, 7, 3, 24), (2, 5, 0, 3, 24), (2, 5, 7, 0, 24), (2, 5, 7, 5, 24), (2, 5, 7, 3, 0), (2, 5, 7, 3, 65)):
        assert rt.conv3x3_wgrad_chunk(*bad) == 0 and rt.conv3x3_wgrad_workspace_bytes(*bad) == 0
    assert [ref.wgrad_sets(c) for c in (1, 24, 28, 29, 40, 56, 57, 64)] == [4, 4, 4, 2, 2, 2, 1, 1]


def test_argument_errors_come_back_before_any_launch():
    """no device is needed: every refusal returns YR_ERR_ARG = -1 with a message before anything is launched"""
    from yoloret_amd import runtime as rt
    L = rt.lib()
    p = ctypes.c_void_p(0x1000)          # a fake, aligned pointer: a refused call touches nothing
    good = dict(B=2, H=8, W=8, cin=3, cout=24, stride=2, pt=0, pl=0, OH=4, OW=4)

    def calls(**kw):
        a = dict(good, **kw)
        geo = (a['B'], a['H'], a['W'], a['cin'], a['cout'], a['stride'], a['pt'], a['pl'], a['OH'], a['OW'])
        x_ld, y_ld, ptr = a.get('x_ld', a['cin']), a.get('y_ld', a['cout']), a.get('ptr', p)
        return [('forward', lambda: L.yr_conv3x3_forward(ptr, x_ld, p, *geo, p, y_ld, None)),
                ('dgrad', lambda: L.yr_conv3x3_dgrad(ptr, y_ld, p, *geo, p, x_ld, None)),
                ('wgrad', lambda: L.yr_conv3x3_wgrad(ptr, x_ld, p, y_ld, *geo, p, 1 << 20, p, None))]
    bad = [dict(cin=5), dict(cin=0), dict(cout=65), dict(cout=0), dict(stride=3), dict(stride=0), dict(pt=3), dict(pl=3), dict(pt=-1), dict(OH=5), dict(OW=2),
           dict(x_ld=2), dict(y_ld=23), dict(ptr=None), dict(ptr=ctypes.c_void_p(0x1002)), dict(B=0), dict(B=65536)]
    for kw in bad:
        for name, call in calls(**kw):
            assert call() == -1, (name, kw)
            msg = L.yr_last_error().decode()
            assert msg.startswith('conv3x3_' + name + ':'), (name, kw, msg)
    # the workspace: null, short, misaligned
    geo = tuple(good[k] for k in ('B', 'H', 'W', 'cin', 'cout', 'stride', 'pt', 'pl', 'OH', 'OW'))
    need = rt.conv3x3_wgrad_workspace_bytes(2, 4, 4, 3, 24)
    assert need == 1 * 27 * 24 * 4
    assert L.yr_conv3x3_wgrad(p, 3, p, 24, *geo, None, need, p, None) == -1 and 'null pointer' in L.yr_last_error().decode()
    for ws, size in ((p, need - 1), (ctypes.c_void_p(0x1008), need)):
        assert L.yr_conv3x3_wgrad(p, 3, p, 24, *geo, ws, size, p, None) == -1 and 'workspace' in L.yr_last_error().decode()


# ----------------------------------------------------------------------------- what tests/test_gpu_stemgrad.py reaches
def test_gpu_cases_reach_what_they_claim():
    from tests import test_gpu_stemgrad as g
    from yoloret_amd import build, runtime as rt
    src = open(os.path.join(os.path.dirname(build.__file__), 'csrc', 'stemgrad.hip')).read()
    assert '#define SG_MIN_PIXELS 256 ' in src and '#define SG_MAX_CHUNKS 2048\n' in src
    assert (ref.MIN_PIXELS, ref.MAX_CHUNKS) == (256, 2048)
    assert len(re.findall(r'blockIdx\.x \* 256 \+ threadIdx\.x', src)) == 2 and g.TILE == 256          # forward: output pixels; dgrad: cells
    # the channel cases the issue names, plus the guarded form (a cout that is no multiple of 8)
    assert set(g.CHANNELS) >= {(3, 8), (3, 24), (3, 40), (3, 64), (1, 24), (4, 24)} and any(cout % 8 for _, cout in g.CHANNELS)
    assert g.MAPS == [(1, 1), (2, 3), (8, 8), (7, 9), (9, 7)] and g.BATCHES == [1, 3] and g.ZERO_PAD == (0, 0, 1, 1)
    # every class of 'same' padding at stride 2: total pad 1 (even sizes: nothing in front) and 2 (odd: one in front), rows and columns
    fronts = {(ref.geometry(h, w, 2, 'same')[0][0], ref.geometry(h, w, 2, 'same')[0][1]) for h, w in g.MAPS}
    assert fronts >= {(0, 0), (1, 1), (0, 1)} and {(h % 2, w % 2) for h, w in g.MAPS} == {(0, 0), (1, 1), (0, 1)}
    # workgroup boundaries: T + 1 and 2 T - 1 outputs, as a row, a column and a block; the cells of the input gradient cross too
    for stride, maps in g.BOUNDARY_MAPS.items():
        outs, cells = [], []
        for h, w in maps:
            pads, (oh, ow) = ref.geometry(h, w, stride, 'same')
            outs.append(oh * ow)
            cells.append(((h - 1 + pads[0]) // stride + 1) * ((w - 1 + pads[1]) // stride + 1))
        assert outs == [g.TILE + 1, g.TILE + 1, 2 * g.TILE - 1]
        assert all(c > g.TILE and c % g.TILE for c in cells)
    # the weight gradient's chunk cases ask the library
    want = []
    for (b, h, w), what in g.CHUNK_CASES:
        chunk = rt.conv3x3_wgrad_chunk(b, h, w, 3, 24)
        rows = b * h
        want.append((chunk, -(-rows // chunk), rows % chunk, chunk > -(-256 // w), any(j * chunk < h < (j + 1) * chunk for j in range(rows)) and b > 1))
    assert want == [(16, 1, 0, False, False), (16, 2, 0, False, False), (16, 2, 8, False, True), (16, 2, 4, False, False), (2, 1025, 1, True, False)]
    assert {ref.wgrad_sets(cout) for _, cout in g.CHUNK_CHANNELS} == {4, 2, 1} and any(cout % 4 for _, cout in g.CHUNK_CHANNELS)
    assert all((16 * 16) % ref.wgrad_sets(cout) == 0 for _, cout in g.CHUNK_CHANNELS)
