"""tests/layers_ref.py on the CPU: what tests/test_gpu_layers_oracle.py relies on holds before any device is involved.

* the layout converters round-trip bit for bit and agree with what autograd.rfcr_parameters makes of a model's own weights;
* the NumPy oracle (oracle/model.py + oracle/nn.py) and the torch oracle (oracle/torch_ref.py) agree in float64 on every block of the
  table, so the device is compared with two implementations that share no arithmetic code;
* every committed seed keeps the float64 run's ReLU6 inputs away from 0 and 6 by more than 8 x the float32 run's deviation there;
* a float32 CPU composition of the same chain (layers_ref.host_block: the BatchNorms folded in float64 and rounded to float32, the
  operators' order) is inside the project's bar, max |got - ref64| / max |ref64| <= 4 E_ref + 2^-24, on every case: the bar asked of
  the device is one a correct float32 implementation meets.  Measured: the stand-in 0.6 to 1.4 x E_ref against bars of 7.1e-07 to 2.2e-06."""
import numpy as np
import pytest
import torch

from tests import layers_ref as lr
from tests.convgrad_ref import rel_err

EPS24 = 2.0 ** -24
BLOCK_IDS = [lr.block_id(c) for c in lr.BLOCKS]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- layouts
@pytest.mark.parametrize('cin,cout', [(16, 96), (3, 5), (17, 15), (120, 48)])
def test_pack_conv_round_trip(cin, cout):
    rng = np.random.default_rng(cin)
    kernel = rng.standard_normal((1, 1, cin, cout)).astype(np.float32)
    wt = lr.pack_conv(kernel)
    ld = (cin + 3) // 4 * 4
    assert wt.dtype == np.float32 and wt.shape == (cout, ld) and wt.flags.c_contiguous
    assert not _bits(wt[:, cin:]).any(), 'pad columns +0'
    for i, o in ((0, 0), (cin - 1, 0), (0, cout - 1), (cin // 2, cout // 3)):
        assert wt[o, i] == kernel[0, 0, i, o]
    back = lr.unpack_conv(wt, cin)
    assert back.shape == kernel.shape and np.array_equal(_bits(back), _bits(kernel))
    # a gradient: whatever stands in the pad columns is dropped, the rest comes back in the Keras layout
    g = rng.standard_normal((cout, ld)).astype(np.float32)
    assert np.array_equal(_bits(lr.pack_conv(lr.unpack_conv(g, cin))[:, :cin]), _bits(g[:, :cin]))


@pytest.mark.parametrize('k', [3, 5])
def test_pack_dw_round_trip(k):
    rng = np.random.default_rng(k)
    kernel = rng.standard_normal((k, k, 7)).astype(np.float32)
    w = lr.pack_dw(kernel)
    assert w.dtype == np.float32 and w.shape == (k * k, 7) and w.flags.c_contiguous
    for ky in range(k):
        for kx in range(k):
            assert np.array_equal(_bits(w[ky * k + kx]), _bits(kernel[ky, kx])), 'tap (ky, kx) is row ky * k + kx'
    assert np.array_equal(_bits(lr.pack_dw(kernel[..., None])), _bits(w)), 'the Keras kernel [k, k, C, 1] and the squeezed one'
    back = lr.unpack_dw(w)
    assert back.shape == kernel.shape and np.array_equal(_bits(back), _bits(kernel))


@pytest.mark.parametrize('model_name', lr.RFCR_MODELS)
def test_converters_are_rfcr_parameters_layouts(model_name):
    """autograd.rfcr_parameters on a model that was given the parameter store's values returns the converters' arrays"""
    from yoloret_amd import autograd
    case = lr.rfcr_case(model_name)
    values = case['P'].values
    par = autograd.rfcr_parameters(lr.product_net(model_name, values), 'cpu')
    for name in autograd.RFCR_CONVS + ('rfcr_sep_pw',):
        assert np.array_equal(_bits(par[name].detach().numpy()), _bits(lr.pack_conv(values[name + '/kernel']))), name
    assert np.array_equal(_bits(par['rfcr_sep_dw'].detach().numpy()), _bits(lr.pack_dw(values['rfcr_sep_dw/depthwise_kernel'])))
    assert np.array_equal(_bits(par['rfcr_wsum/alpha'].detach().numpy()), _bits(values['rfcr_wsum/alpha']))
    for bn in autograd.RFCR_BNS:
        for p in lr.BN_PARTS:
            assert np.array_equal(_bits(par['%s/%s' % (bn, p)].detach().numpy()), _bits(values['%s/%s' % (bn, p)]))
    assert len(par) == 5 + 1 + 1 + 8
    # the taps and outputs the device test is told to expect
    c1, c2, c3 = {'mobilenetv2x75': (120, 72, 24), 'efficientnetb0': (192, 112, 40)}[model_name]
    assert [t.shape for t in case['taps']] == [(2, 3, 3, c1), (2, 6, 6, c2), (2, 12, 12, c3), (2, 6, 6, 24)]
    assert [w.shape for w in case['want64']] == [(2, 3, 3, c1 + 96), (2, 6, 6, c2 + 96), (2, 12, 12, c3 + 96)]


# ----------------------------------------------------------------------------- the two oracles
@pytest.mark.parametrize('lite', [True, False], ids=['relu6', 'swish'])
@pytest.mark.parametrize('case', lr.BLOCKS, ids=BLOCK_IDS)
def test_the_two_oracles_agree_in_float64(case, lite):
    x, f = lr.block_inputs(case)
    y_np = lr.numpy_block(lr.fresh_store(), case, x, lite, np.float64)
    y_t = lr.torch_block(lr.fresh_store(), case, x, lite, torch.float64)['y']
    assert y_np.shape == f.shape == y_t.shape
    e = rel_err(y_t, y_np)
    print('%s: torch oracle against NumPy oracle %.3e (bar 1e-12)' % (lr.block_id(case), e))
    assert e <= 1e-12
    us, y = lr.preactivations(lr.fresh_store(), case, x, lite, np.float64)
    assert np.array_equal(y, y_np), 'preactivations is mbconv_block, operation for operation'
    assert len(us) == (1 if case[3] == 1 else 2)


@pytest.mark.parametrize('case', lr.BLOCKS, ids=BLOCK_IDS)
def test_seeds_keep_relu6_inputs_off_the_kinks(case):
    x, _ = lr.block_inputs(case)
    us64, _ = lr.preactivations(lr.fresh_store(), case, x, True, np.float64)
    us32, _ = lr.preactivations(lr.fresh_store(), case, x, True, np.float32)
    for what, distance, margin in lr.relu6_margins(us64, us32):
        print('%s %s: smallest distance %.3e, margin %.3e' % (lr.block_id(case), what, distance, margin))
        assert distance > margin, 'a kink lies too close - choose another seed'
    # and Swish's exponent stays inside expf's range
    us, _ = lr.preactivations(lr.fresh_store(), case, x, False, np.float64)
    assert max(float(np.abs(u).max()) for _, u in us) < 87.0


# ----------------------------------------------------------------------------- the bar is reachable
@pytest.mark.parametrize('lite', [True, False], ids=['relu6', 'swish'])
@pytest.mark.parametrize('case', lr.BLOCKS, ids=BLOCK_IDS)
def test_float32_chain_is_inside_the_bar(case, lite):
    x, _ = lr.block_inputs(case)
    P = lr.fresh_store()
    y64, y32 = lr.numpy_block(P, case, x, lite, np.float64), lr.numpy_block(P, case, x, lite, np.float32)
    got = lr.host_block(x, P.values, lr.effnet_names(case[0]), case[1], case[2], case[3], 'relu6' if lite else 'swish', lr.is_residual(case))
    e, e_ref = rel_err(got, y64), rel_err(y32, y64)
    print('%s: float32 chain %.3e, float32 oracle %.3e, bar %.3e' % (lr.block_id(case), e, e_ref, 4 * e_ref + EPS24))
    assert got.shape == y64.shape and e <= 4 * e_ref + EPS24


@pytest.mark.parametrize('hw', lr.MBV2_IMAGES, ids=['%dx%d' % hw for hw in lr.MBV2_IMAGES])
def test_float32_mobilenet_chain_is_inside_the_bar(hw):
    """block 0, 1, 2 of MobileNetV2 x0.75 chained from the float64 run's Conv1_relu rounded to float32, each output against the float64
    run with the full float32 run's deviation there as E_ref"""
    case = lr.mbv2_case(hw)
    a64, a32 = case['acts64'], case['acts32']
    h, w = -(-hw[0] // 2), -(-hw[1] // 2)
    h2, w2 = -(-h // 2), -(-w // 2)
    assert [a64[k].shape for k in ('Conv1_relu', 'block_0_out', 'block_1_out', 'block_2_out')] == [(2, h, w, 24), (2, h, w, 16), (2, h2, w2, 24), (2, h2, w2, 24)]
    assert a64['block_2_add'] is a64['block_2_out']
    t = a64['Conv1_relu'].astype(np.float32)
    for block, stride, expand, residual, out in lr.MBV2_CHAIN:
        t = lr.host_block(t, case['P'].values, lr.mbv2_names(block), 3, stride, expand, 'relu6', residual)
        e, e_ref = rel_err(t, a64[out]), rel_err(a32[out], a64[out])
        print('%d x %d %s: float32 chain %.3e, float32 oracle %.3e, bar %.3e' % (hw + (out, e, e_ref, 4 * e_ref + EPS24)))
        assert e <= 4 * e_ref + EPS24
