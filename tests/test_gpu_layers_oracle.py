"""The training operators of yoloret_amd/autograd.py on the model's own layers, with the model's own parameters, against the project's
two CPU oracles (oracle/model.py + oracle/nn.py in NumPy, oracle/torch_ref.py on torch): what is trained is what is shipped.

* the RFCR module of ``rfcr_parameters`` + ``rfcr_module(training=False)`` on the oracle's backbone taps against oracle.model.rfcr_module;
* EfficientNet's MBConv blocks of stages 1-3 (ReLU6, then Swish; no squeeze-excite) composed by tests/layers_ref.device_block from the
  Keras-layout kernels of a ParamStore: the forward against the NumPy oracle, the gradients of a fixed linear functional for the input
  and every kernel, mapped back to the Keras layouts, against torch.autograd over the torch oracle;
* MobileNetV2 x0.75's first three blocks by their Keras names, chained, against oracle.model.mobilenet_v2.

The bar is the project's own: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the float32 oracle's deviation from the
float64 oracle on the same inputs.  Every comparison prints its figures before it asserts (run with -s).  What the cases rest on (the
two oracles agree, the seeds keep ReLU6's inputs off its kinks, a float32 chain on the CPU meets the bar) is asserted without a device
in tests/test_layers_ref_host.py."""
import numpy as np
import pytest
import torch

from tests import layers_ref as lr
from tests.test_gpu_autograd import _bits, _dev, _within_bar

pytestmark = pytest.mark.gpu

BLOCK_IDS = [lr.block_id(c) for c in lr.BLOCKS]


def _ag():
    from yoloret_amd import autograd
    return autograd


# ----------------------------------------------------------------------------- a. the RFCR module
@pytest.mark.parametrize('model_name', lr.RFCR_MODELS)
def test_rfcr_module_is_the_oracles(dev, model_name):
    """``rfcr_parameters`` of a model that was given the ParamStore's values + ``rfcr_module(training=False)`` on the NumPy oracle's
    backbone taps (2 synthetic images, 96 x 96) against oracle.model.rfcr_module in float64; the taps pass through bit for bit, no
    parameter and no moving statistic changes.
    Measured on an MI355X (device, E_ref, bar), whole output / its 96 fused channels alone:
      mobilenetv2x75  1: 4.138e-07, 3.179e-07, 1.331e-06 / 6.860e-07, 5.270e-07, 2.168e-06;  2: 4.286e-07, 3.361e-07, 1.404e-06 / 6.860e-07, 5.380e-07, 2.212e-06;
                      3: 6.860e-07, 5.380e-07, 2.212e-06 / the same
      efficientnetb0  1, 2, 3: 3.244e-07, 4.250e-07, 1.760e-06 / the same (every output shows the same three figures)
    (the closest to its bar: mobilenetv2x75 output 1's fused channels, 6.9e-07 against 2.2e-06)."""
    ag = _ag()
    case = lr.rfcr_case(model_name)
    c1, c2, c3 = {'mobilenetv2x75': (120, 72, 24), 'efficientnetb0': (192, 112, 40)}[model_name]
    assert [t.shape for t in case['taps']] == [(2, 3, 3, c1), (2, 6, 6, c2), (2, 12, 12, c3), (2, 6, 6, 24)]
    par = ag.rfcr_parameters(lr.product_net(model_name, case['P'].values), dev)
    before = {k: v.detach().clone() for k, v in par.items()}
    taps = [_dev(t, dev) for t in case['taps']]
    outs = ag.rfcr_module(*taps, par, training=False)
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in outs] == [(2, 3, 3, c1 + 96), (2, 6, 6, c2 + 96), (2, 12, 12, c3 + 96)]
    ok = []
    for i, (o, tap) in enumerate(zip(outs, case['taps'])):
        ok.append(_within_bar('%s output %d' % (model_name, i + 1), o, case['want32'][i], case['want64'][i]))
        c = tap.shape[-1]      # the fused map's 96 channels on their own: the tap, which is exact, does not set the scale
        ok.append(_within_bar('%s output %d, fused channels' % (model_name, i + 1), o[..., c:], case['want32'][i][..., c:], case['want64'][i][..., c:]))
        assert np.array_equal(_bits(o[..., :tap.shape[-1]]), tap.view(np.uint32)), 'concat moves the tap'
    assert sorted(par) == sorted(before) and all(np.array_equal(_bits(par[k]), _bits(before[k])) for k in par), 'nothing is updated'
    assert all(ok)


# ----------------------------------------------------------------------------- b, c. EfficientNet's blocks
def _block_test(dev, case, lite):
    ag = _ag()
    name, k, stride, expand, cin, cout = case[:6]
    what = '%s %s' % (lr.block_id(case), 'relu6' if lite else 'swish')
    x, f = lr.block_inputs(case)
    P = lr.fresh_store()
    y64, y32 = lr.numpy_block(P, case, x, lite, np.float64), lr.numpy_block(P, case, x, lite, np.float32)
    us64, _ = lr.preactivations(P, case, x, lite, np.float64)
    if lite:
        us32, _ = lr.preactivations(P, case, x, lite, np.float32)
        for where, distance, margin in lr.relu6_margins(us64, us32):
            print('%s %s: smallest distance %.3e, margin %.3e' % (what, where, distance, margin))
            assert distance > margin, 'a kink lies too close - choose another seed'
    else:
        assert max(float(np.abs(u).max()) for _, u in us64) < 87.0, 'u beyond the clamp of expf'
    g64, g32 = lr.torch_block(P, case, x, lite, torch.float64, f), lr.torch_block(P, case, x, lite, torch.float32, f)

    tx = _dev(x, dev, True)
    y, leaves, frozen = lr.device_block(ag, tx, P.values, lr.effnet_names(name), k, stride, expand, 'relu6' if lite else 'swish',
                                        lr.is_residual(case))
    assert tuple(y.shape) == f.shape and sorted(leaves) == sorted(['dw', 'project'] + (['expand'] if expand != 1 else []))
    (y * _dev(f, dev)).sum().backward()
    torch.cuda.synchronize()
    ok = [_within_bar(what + ' y', y, y32, y64),
          _within_bar(what + ' d x', tx.grad, g32['x'], g64['x'])]
    for part, leaf in sorted(leaves.items()):
        g = leaf.grad
        assert g is not None and g.shape == leaf.shape, part
        if part == 'dw':
            got = lr.unpack_dw(g.cpu().numpy())
        else:
            c = g64[part].shape[2]
            assert not _bits(g[:, c:]).any(), 'pad columns of d %s are +0' % part
            got = lr.unpack_conv(g.cpu().numpy(), c)
        assert got.shape == g64[part].shape
        ok.append(_within_bar('%s d %s' % (what, part), torch.from_numpy(got), g32[part], g64[part]))
    assert len(frozen) == (6 if expand != 1 else 4) and all(t.grad is None and not t.requires_grad for t in frozen), 'scale and shift are frozen'
    assert all(ok)


@pytest.mark.parametrize('case', lr.BLOCKS, ids=BLOCK_IDS)
def test_lite_block_against_the_oracles(dev, case):
    """EfficientNet-lite's block (ReLU6): forward against the NumPy oracle, d / d x and d / d every kernel of (y * f).sum() against the
    torch oracle.
    Measured on an MI355X (device, E_ref, bar):
      stage1_block0 13x11:  y 1.672e-07, 1.672e-07, 7.283e-07;  d x 1.143e-07, 1.589e-07, 6.953e-07;  d dw 1.451e-07, 1.809e-07, 7.831e-07;  d project 1.557e-07, 1.557e-07, 6.824e-07
      stage2_block0 13x11:  y 2.495e-07, 1.899e-07, 8.191e-07;  d x 1.959e-07, 2.368e-07, 1.007e-06;  d dw 2.304e-07, 1.625e-07, 7.094e-07;  d expand 1.798e-07, 1.551e-07, 6.798e-07;  d project 1.990e-07, 1.557e-07, 6.824e-07
      stage2_block0 12x10:  y 2.635e-07, 2.330e-07, 9.914e-07;  d x 2.525e-07, 2.102e-07, 9.003e-07;  d dw 1.076e-07, 1.268e-07, 5.669e-07;  d expand 2.738e-07, 2.245e-07, 9.575e-07;  d project 2.282e-07, 1.862e-07, 8.042e-07
      stage2_block1 7x9:    y 1.808e-07, 1.922e-07, 8.285e-07;  d x 2.212e-07, 1.705e-07, 7.415e-07;  d dw 1.227e-07, 2.490e-07, 1.056e-06;  d expand 2.550e-07, 2.112e-07, 9.045e-07;  d project 3.356e-07, 2.004e-07, 8.613e-07
      stage3_block0 13x11:  y 2.676e-07, 2.221e-07, 9.480e-07;  d x 3.108e-07, 1.934e-07, 8.334e-07;  d dw 2.326e-07, 2.216e-07, 9.461e-07;  d expand 2.398e-07, 2.103e-07, 9.009e-07;  d project 1.957e-07, 1.611e-07, 7.038e-07
      stage3_block0 12x10:  y 2.785e-07, 2.129e-07, 9.113e-07;  d x 2.636e-07, 2.054e-07, 8.811e-07;  d dw 1.548e-07, 2.044e-07, 8.771e-07;  d expand 2.083e-07, 2.108e-07, 9.028e-07;  d project 2.146e-07, 1.936e-07, 8.338e-07
      stage3_block1 7x5:    y 2.160e-07, 2.392e-07, 1.016e-06;  d x 2.249e-07, 2.249e-07, 9.593e-07;  d dw 1.877e-07, 2.045e-07, 8.777e-07;  d expand 3.691e-07, 2.981e-07, 1.252e-06;  d project 4.098e-07, 3.889e-07, 1.615e-06
    (the closest to its bar: stage2_block1's d project, 3.4e-07 against 8.6e-07).  The ReLU6 inputs' smallest distance from a kink, against 8 x the
    float32 oracle's deviation there: between 3.0e-05 against 1.4e-05 (stage2_block1_dw_BN) and 2.4e-04 against 1.4e-05."""
    _block_test(dev, case, True)


@pytest.mark.parametrize('case', lr.BLOCKS, ids=BLOCK_IDS)
def test_swish_block_against_the_oracles(dev, case):
    """The same seven blocks with Swish (efficientnet.py's own activation; se_ratio None: no squeeze-excite).
    Measured on an MI355X (device, E_ref, bar):
      stage1_block0 13x11:  y 2.384e-07, 1.628e-07, 7.109e-07;  d x 2.000e-07, 1.702e-07, 7.405e-07;  d dw 9.856e-08, 1.897e-07, 8.185e-07;  d project 1.845e-07, 1.753e-07, 7.609e-07
      stage2_block0 13x11:  y 3.733e-07, 4.936e-07, 2.034e-06;  d x 3.611e-07, 3.149e-07, 1.319e-06;  d dw 2.230e-07, 4.291e-07, 1.776e-06;  d expand 2.338e-07, 3.306e-07, 1.382e-06;  d project 3.129e-07, 1.661e-07, 7.240e-07
      stage2_block0 12x10:  y 3.658e-07, 3.861e-07, 1.604e-06;  d x 2.667e-07, 2.152e-07, 9.204e-07;  d dw 1.981e-07, 2.554e-07, 1.081e-06;  d expand 6.271e-07, 3.619e-07, 1.507e-06;  d project 3.379e-07, 2.646e-07, 1.118e-06
      stage2_block1 7x9:    y 3.063e-07, 2.171e-07, 9.278e-07;  d x 3.415e-07, 3.789e-07, 1.575e-06;  d dw 1.682e-07, 2.170e-07, 9.275e-07;  d expand 3.940e-07, 3.209e-07, 1.343e-06;  d project 2.916e-07, 1.544e-07, 6.773e-07
      stage3_block0 13x11:  y 3.375e-07, 2.810e-07, 1.184e-06;  d x 3.588e-07, 2.385e-07, 1.014e-06;  d dw 2.435e-07, 2.680e-07, 1.132e-06;  d expand 3.155e-07, 5.343e-07, 2.197e-06;  d project 2.539e-07, 1.886e-07, 8.142e-07
      stage3_block0 12x10:  y 2.233e-07, 3.660e-07, 1.524e-06;  d x 3.574e-07, 3.728e-07, 1.551e-06;  d dw 3.348e-07, 2.476e-07, 1.050e-06;  d expand 4.506e-07, 4.369e-07, 1.807e-06;  d project 1.783e-07, 1.656e-07, 7.220e-07
      stage3_block1 7x5:    y 2.352e-07, 2.484e-07, 1.053e-06;  d x 4.120e-07, 4.598e-07, 1.899e-06;  d dw 2.528e-07, 2.371e-07, 1.008e-06;  d expand 3.543e-07, 3.303e-07, 1.381e-06;  d project 3.696e-07, 3.271e-07, 1.368e-06
    (the closest to its bar, here and in the whole file: stage2_block0 13x11's d project, 3.1e-07 against 7.2e-07)."""
    _block_test(dev, case, False)


# ----------------------------------------------------------------------------- d. MobileNetV2 x0.75's first blocks
@pytest.mark.parametrize('hw', lr.MBV2_IMAGES, ids=['%dx%d' % hw for hw in lr.MBV2_IMAGES])
def test_mobilenet_first_blocks_against_the_oracle(dev, hw):
    """expanded_conv_ (no expand convolution), block_1_ (stride 2) and block_2_ (residual) chained on the device from the float64 run's
    Conv1_relu rounded to float32; block_0_out, block_1_out and block_2_add against oracle.model.mobilenet_v2 in float64.  E_ref at each
    output is the full float32 run's deviation there, the stem's rounding included.  50 x 38: block 0 runs on an odd 25 x 19 map and
    block 1 applies its stride 2 to it.
    Measured on an MI355X (device, E_ref, bar), block_0_out;  block_1_out;  block_2_add:
      64 x 64  1.992e-07, 3.013e-07, 1.265e-06;  3.525e-07, 3.378e-07, 1.411e-06;  4.574e-07, 5.398e-07, 2.219e-06
      50 x 38  1.695e-07, 2.274e-07, 9.693e-07;  3.471e-07, 2.995e-07, 1.258e-06;  4.375e-07, 4.386e-07, 1.814e-06
    (the closest to its bar: 50 x 38 block_1_out, 3.5e-07 against 1.3e-06).  The float32 chain on the CPU meets the same bars
    (tests/test_layers_ref_host.py), so no per-block reference was needed."""
    ag = _ag()
    case = lr.mbv2_case(hw)
    a64, a32 = case['acts64'], case['acts32']
    h, w = -(-hw[0] // 2), -(-hw[1] // 2)
    assert a64['Conv1_relu'].shape == (2, h, w, 24) and a64['block_2_add'].shape == (2, -(-h // 2), -(-w // 2), 24)
    t = _dev(a64['Conv1_relu'], dev)
    ok = []
    for block, stride, expand, residual, out in lr.MBV2_CHAIN:
        t, _, _ = lr.device_block(ag, t, case['P'].values, lr.mbv2_names(block), 3, stride, expand, 'relu6', residual)
        t = t.detach()
        ok.append(_within_bar('%d x %d %s' % (hw + (out,)), t, a32[out], a64[out]))
    assert all(ok)
