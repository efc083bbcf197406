"""Tile index -> kernel of the pointwise family: for every value of op.k a POINTWISE op accepts, the kernel the launch reports
(yr_last_kernel) is the one this file's literal tables name, and the output equals the op.k = 0 run of the same op and form family bit
for bit - the tile-shape independence the tuner relies on.  The tables restate the library's (pointwise.hip, pointwise_lds.hip,
pointwise_split.hip, pointwise_h.hip, pointwise_hs.hip, pointwise_hq.hip) by hand; nothing here is derived from the library.

Every launch is tiny: two images of a 5 x 7 map (70 GEMM rows: one full 64-row tile and a ragged one; the up-sampled form needs an
even map and takes 6 x 6 - 72 rows, the same two tiles), 20 or 24 couts, through run_pointwise / run_pointwise16 (oracle parity and
red zones included) - the depthwise-folded source through the same calls spelled out here."""
import numpy as np
import pytest
import torch

from tests import fence
from tests.test_gpu_narrow import run_pointwise16
from tests.test_gpu_ops import _dev_vec, run_pointwise
from tests.util import PW_NUM_CFGS, to_dev

pytestmark = pytest.mark.gpu

B, H, W = 2, 5, 7


def _rt():
    from yoloret_amd import runtime as rt
    return rt


def _last():
    return _rt().lib().yr_last_kernel().decode()


# ---- float32.  (PT, CT, WM, WN) of the LDS-staged tile shapes 0 .. 13 (pw_kernel; pws_kernel in the split form, where the direct
# kernels' indices 14 .. 28 map onto them: index % 14), then (PT, CT) of the direct kernel's shapes 14 .. 28
LDS = [(4, 1, 4, 1), (2, 2, 4, 1), (2, 3, 4, 1), (4, 2, 2, 2), (2, 5, 4, 1), (4, 3, 2, 2), (4, 4, 2, 2),
       (1, 1, 4, 1), (1, 2, 4, 1), (1, 3, 4, 1), (1, 4, 4, 1), (1, 5, 4, 1), (1, 6, 4, 1), (1, 8, 4, 1)]
DIRECT = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 8), (2, 2), (2, 3), (2, 4), (2, 5), (2, 6), (4, 2), (4, 3), (4, 4)]
DIRECT_DEPTH = {1: 4, 2: 4, 3: 3, 4: 3, 5: 3, 6: 3, 8: 2, 10: 2, 12: 2, 16: 2}      # PT * CT -> chunks of loads in flight
F32_HEURISTIC = 7           # 70 rows x 20 couts: 64 x 16, the shape with the most workgroups

# the four source forms: name -> (segments at cin 24, segments at cin 40, gate, activation, map, source mode 0 | 1 | 2, pooled)
FORMS = {
    'identity': ([(24, 'identity')], [(40, 'identity')], False, 'relu6', (H, W), 1, False),
    'gated': ([(24, 'identity')], [(40, 'identity')], True, 'none', (H, W), 2, False),
    'up2': ([(16, 'identity'), (8, 'up2')], [(24, 'identity'), (16, 'up2')], False, 'swish', (6, 6), 0, False),
    'maxpool2': ([(24, 'maxpool2')], [(40, 'maxpool2')], False, 'relu6', (H, W), 0, True),
}


def _f32_name(k, mode, split):
    i = F32_HEURISTIC if k == 0 else k - 1
    if split:
        return 'pws_kernel<%d,%d,%d,%d,%d>' % (LDS[i % 14] + (int(mode != 0),))
    if i < 14:
        return 'pw_kernel<%d,%d,%d,%d,%d,0>' % (LDS[i] + (int(mode != 0),))
    pt, ct = DIRECT[i - 14]
    return 'pwd_kernel<%d,%d,%d,%d>' % (pt, ct, DIRECT_DEPTH[pt * ct], mode)


@pytest.mark.parametrize('f32_mfma', [False, True], ids=['split', 'f32_mfma'])
@pytest.mark.parametrize('form', list(FORMS))
def test_float32_index_to_kernel(dev, form, f32_mfma):
    segs, _, gate, act, (h, w), mode, _ = FORMS[form]
    assert len(LDS) + len(DIRECT) == PW_NUM_CFGS[0]
    first = None
    for k in range(PW_NUM_CFGS[0] + 1):
        got = run_pointwise(dev, np.random.default_rng(11), B, h, w, segs, 20, act, gate=gate, cfg=k, f32_mfma=f32_mfma)
        assert _last() == _f32_name(k, mode, not f32_mfma), 'op.k = %d' % k
        first = got if first is None else first
        assert np.array_equal(got, first), 'op.k = %d differs from op.k = 0' % k


@pytest.mark.parametrize('k,shape', [(0, 9), (1, 9), (10, 9), (14, 13)])
def test_float32_depthwise_folded_source(dev, k, shape):
    """A YR_X_DW3 source runs the LDS-staged float32-MFMA kernel in the 64-row shapes 9 .. 13 only; any other request takes the
    narrowest of them that covers the couts (20 couts: shape 9)."""
    rt = _rt()
    cin, cout = 24, 20
    outs = []
    for kk in (0, k):
        rng = np.random.default_rng(12)
        x = to_dev(rng.standard_normal((B, H, W, cin)).astype(np.float32), dev)
        keep = [_dev_vec(rng.standard_normal((cout, cin)) * np.sqrt(2.0 / cin), dev), _dev_vec(rng.uniform(0.5, 1.5, cout), dev),
                _dev_vec(rng.normal(0, 0.3, cout), dev), _dev_vec(rng.standard_normal((9, cin)) / 3.0, dev),
                _dev_vec(rng.uniform(0.5, 1.5, cin), dev), _dev_vec(rng.normal(0, 0.3, cin), dev)]
        out = torch.full((B, H, W, cout), float('nan'), dtype=torch.float32, device=dev)
        op = rt.new_op(rt.OP_POINTWISE, 'none')
        op.h, op.w, op.cin, op.cout, op.nsrc = H, W, cin, cout, 1
        op.src[0] = rt.make_src(x, c=cin, xform='dw3')
        op.se_reduced = 1 | (rt.ACT['relu6'] << rt.PWDW_ACT_SHIFT)        # stride 1, ReLU6 behind the depthwise stage
        op.wgt, op.scale, op.shift, op.wgt2, op.b1, op.b2 = [t.data_ptr() for t in keep]
        op.out, op.out_ld = out.data_ptr(), cout
        op.k = kk
        fence.run_op(op, B, writes=[out], reads=[x] + keep)
        name = _last()
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert name == 'pw_kernel<%d,%d,%d,%d,1,1>' % LDS[shape]
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


# ---- bf16 / f16.  Tile index -> launcher: ('h', PT, CP) the direct kernel, ('l', PT, CT) the LDS-tiled form, ('p', PT, CP) the
# walking small-K form, ('s', PT) the activation-stationary form, ('q', PT) the all-couts k-streaming form
H16 = [('h', 1, 1), ('h', 1, 2), ('h', 1, 3), ('h', 1, 4), ('h', 2, 1), ('h', 2, 2), ('h', 2, 3), ('l', 2, 4), ('h', 4, 1), ('h', 4, 2),
       ('p', 1, 1), ('p', 2, 1), ('p', 1, 2), ('p', 2, 2), ('l', 4, 4), ('l', 2, 4), ('l', 4, 2), ('l', 2, 2),
       ('s', 1), ('s', 2), ('s', 1), ('s', 2), ('q', 1), ('q', 2), ('q', 1), ('q', 2)]
H16_DEPTH = {(1, 1): 4, (1, 2): 3, (1, 3): 3, (1, 4): 2, (2, 1): 4, (2, 2): 3, (2, 3): 3, (4, 1): 2, (4, 2): 2}   # (PT, CP) -> chunks in flight
H16_HEURISTIC = 0           # 70 rows x 24 couts: 64 x 32


def _h16_name(dt, k, mode, pooled, act, kp):
    e = H16[H16_HEURISTIC if k == 0 else k - 1]
    nch = (kp + 31) // 32
    if e[0] == 'p' and (mode == 0 or nch > 4):          # the walking form takes one identity source of at most 128 channels
        e = ('h',) + e[1:]
    if e[0] == 's' and (kp > 256 or pooled):            # the stationary form: at most 256 channels, no pooled source
        e = ('l', 4, 2)
    if e[0] == 'q' and pooled:
        e = ('l', 4, 2)
    if e[0] == 'h':
        return 'pwh_kernel<%s,%d,%d,%d,%d>' % (dt, e[1], e[2], H16_DEPTH[e[1:]], mode)
    if e[0] == 'l':
        return 'pwhl_kernel<%s,%d,%d,%d,%d>' % (dt, e[1], e[2], mode, int(pooled))
    if e[0] == 'p':
        return 'pwhp_kernel<%s,%d,%d,%d,%d>' % (dt, e[1], e[2], {1: 1, 2: 2, 3: 4, 4: 4}[nch], mode)
    if e[0] == 's':      # (NCH 2 for up to 64 channels; the epilogue: generic | plain | plain with ReLU6)
        plain, clamp = {'swish': (0, 0), 'none': (1, 0), 'relu6': (1, 1)}[act]
        return 'pwhs_kernel<%s,%d,%d,%d,%d,%d>' % (dt, e[1], {2: 2}[nch], mode, plain, clamp)
    return 'pwhq_kernel<%s,%d,2,%d>' % (dt, e[1], mode)      # (24 couts: one pair, the narrowest instantiation holds two)


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('form', list(FORMS) + ['deep'])
def test_16bit_index_to_kernel(dev, dt, form):
    """'deep': 264 channels of one identity source - beyond the activation-stationary form's 256 and the walking form's 128."""
    _, segs, gate, act, (h, w), mode, pooled = FORMS[form] if form != 'deep' else (None, [(264, 'identity')], False, 'relu6', (H, W), 1, False)
    n = PW_NUM_CFGS[_rt().dtype_id(dt)]
    assert len(H16) == n
    kp = sum((c + 7) // 8 * 8 for c, _ in segs)
    first = None
    for k in range(n + 1):
        got = run_pointwise16(dev, dt, np.random.default_rng(13), B, h, w, segs, 24, act, gate=gate, cfg=k)
        assert _last() == _h16_name(dt, k, mode, pooled, act, kp), 'op.k = %d' % k
        first = got if first is None else first
        assert np.array_equal(got, first), 'op.k = %d differs from op.k = 0' % k
