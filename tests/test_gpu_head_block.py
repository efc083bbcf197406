"""The reference's head block (model.py:91-115, make_last_layers_efficientnet_lite) as ``autograd.head_block_parameters`` +
``autograd.head_block`` build it, with the model's own parameters, against the project's CPU oracles: 'bu3' of MobileNetV2 x0.75 and of
EfficientNet-B0 and 'td3' of MobileNetV2 x0.75 (248 input channels), on 2 images at 12 x 12.  The parameters are the values of a
``layers_ref.fresh_store()`` (the one ``layers_ref.rfcr_case`` completed for the whole ``yolov3_body``), taken through
``layers_ref.product_net``: what is trained is what is shipped.

The bar is the project's own: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the float32 torch oracle's deviation from
the float64 one on the same inputs.  Every comparison prints its figures before it asserts (run with -s).  What the cases rest on (the
two oracles agree, the seeds keep ReLU6's inputs off its kinks, |u| < 87 before every Swish and sigmoid, a float32 chain on the CPU
meets the bar) is asserted without a device in tests/test_segrad_host.py.

The figures measured on an MI355X are in the docstrings of the tests."""
import numpy as np
import pytest
import torch

from tests import bntrain_ref, layers_ref as lr, selayers_ref as sl
from tests.test_gpu_autograd import _bits, _dev, _within_bar

pytestmark = pytest.mark.gpu


def _ag():
    from yoloret_amd import autograd
    return autograd


def _params(dev, case):
    return _ag().head_block_parameters(lr.product_net(case[0], sl.head_store(case).values), case[1], dev)


def _tensors(par):
    return {k: v for k, v in par.items() if k != 'name'}


@pytest.mark.parametrize('case', sl.HEAD_CASES, ids=sl.HEAD_IDS)
def test_head_block_is_the_oracles(dev, case):
    """``head_block(training=False)``: x_out and y against oracle.torch_ref._Net.head_block in float64 (E_ref: the same in float32), the
    gradients of (x_out * f1).sum() + (y * f2).sum() for the input and every kernel and bias against torch.autograd over it, mapped back to
    the Keras layouts; gamma and beta are folded and get no gradient; no parameter and no moving statistic changes.  td3 has no y: the
    product's model, like the reference's, discards the top-down blocks' y convolutions, so its functional is (x_out * f1).sum().
    Measured on an MI355X (device, E_ref, bar); bu3's figures are the same for both models (the block's parameters depend on its name):
      bu3  x_out 4.830e-07, 3.193e-07, 1.337e-06;  y 4.536e-07, 3.869e-07, 1.607e-06;  d x 2.966e-07, 2.638e-07, 1.115e-06;
           d _conv 3.573e-07, 3.383e-07, 1.413e-06;  d _mb_dw 2.870e-07, 2.750e-07, 1.160e-06;  d _mb_se_reduce 4.628e-07, 1.132e-06, 4.588e-06;
           d _mb_se_reduce/bias 4.380e-07, 9.861e-07, 4.004e-06;  d _mb_se_expand 3.331e-07, 4.457e-07, 1.842e-06;
           d _mb_se_expand/bias 2.373e-07, 2.379e-07, 1.011e-06;  d _mb_project 2.769e-07, 3.058e-07, 1.283e-06;  d _y 3.112e-07, 6.097e-07, 2.498e-06
      td3  d x 3.939e-07, 3.181e-07, 1.332e-06;  d _conv 3.230e-07, 5.477e-07, 2.250e-06;  d _mb_dw 3.098e-07, 2.860e-07, 1.203e-06;
           d _mb_se_reduce 4.969e-07, 4.320e-07, 1.788e-06;  d _mb_se_reduce/bias 5.537e-07, 4.741e-07, 1.956e-06;  d _mb_se_expand 4.545e-07, 8.432e-07, 3.433e-06;
           d _mb_se_expand/bias 3.115e-07, 2.280e-07, 9.715e-07;  d _mb_project 3.817e-07, 3.361e-07, 1.404e-06
    (the closest to its bar in the file: bu3's x_out, 0.36 of it)."""
    ag = _ag()
    model_name, name, cin, _ = case
    x, f1, f2 = sl.head_inputs(case)
    P = sl.head_store(case)
    t64, t32 = sl.torch_head(P, name, x, torch.float64, f1, f2), sl.torch_head(P, name, x, torch.float32, f1, f2)
    par = _params(dev, case)
    assert par['name'] == name and par['_conv'].shape == (sl.HEAD_F, (cin + 3) // 4 * 4) and par['_mb_se_reduce'].shape == (sl.HEAD_F, 32)
    kernels = sl.head_kernels(name)
    trained = [k for k, v in _tensors(par).items() if v.requires_grad]
    assert sorted(trained) == sorted(k for k in sl.HEAD_TRAINED if k != '_y' or '_y' in kernels) and len(_tensors(par)) == len(trained) + 6
    before = {k: v.detach().clone() for k, v in _tensors(par).items()}
    tx = _dev(x, dev, True)
    xo, y = ag.head_block(tx, par, training=False)
    assert tuple(xo.shape) == (2, 12, 12, sl.HEAD_O)
    loss = (xo * _dev(f1, dev)).sum()
    if '_y' in kernels:
        assert tuple(y.shape) == (2, 12, 12, sl.HEAD_O)
        loss = loss + (y * _dev(f2, dev)).sum()
    else:
        assert y is None and name == 'td3', 'the model holds no y convolution for a top-down block'
    loss.backward()
    torch.cuda.synchronize()
    what = '%s %s' % (model_name, name)
    ok = [_within_bar(what + ' x_out', xo, t32['x_out'], t64['x_out']), _within_bar(what + ' d x', tx.grad, t32['x'], t64['x'])]
    if '_y' in kernels:
        ok.append(_within_bar(what + ' y', y, t32['y'], t64['y']))
    for key in kernels:
        g = par[key].grad
        assert g is not None and g.shape == par[key].shape, key
        if key in ('_conv', '_mb_project', '_y'):
            assert not _bits(g[:, t64[key].shape[2]:]).any(), 'pad columns of d %s are +0' % key
        got = sl.unpack_head_grad(key, g.cpu().numpy(), t64[key].shape)
        assert got.shape == t64[key].shape, key
        ok.append(_within_bar('%s d %s' % (what, key), torch.from_numpy(np.ascontiguousarray(got)), t32[key], t64[key]))
    for key, v in _tensors(par).items():
        assert key in kernels or v.grad is None, 'the folded BatchNorms take no gradient: ' + key
        assert np.array_equal(_bits(v), _bits(before[key])), 'nothing is updated: ' + key
    assert all(ok)


def test_head_block_in_training_mode(dev):
    """``head_block(training=True)`` on bu3 of MobileNetV2 x0.75: BatchNorm on the statistics of the batch; x_out, y and the gradients for
    the input and all fourteen trained tensors (gamma and beta included) against float64 torch autograd over
    tests/selayers_ref.train_head (E_ref: the same in float32); the six moving statistics move, by the rule of bntrain_ref.moving64 with
    momentum 0.99.
    Measured on an MI355X (device, E_ref, bar):  y 3.963e-07, 4.320e-07, 1.788e-06;  d x 4.069e-07, 4.164e-07, 1.725e-06;  the fourteen
    parameter gradients between d _mb_project_BN/beta 1.828e-07, 2.077e-07, 8.905e-07 and d _conv_BN/gamma 2.240e-06, 2.596e-06, 1.045e-05
    (the sum behind gamma of the first BatchNorm cancels: float32 torch deviates as much), none above 0.25 of its bar."""
    ag = _ag()
    case = sl.HEAD_TRAIN_CASE
    x, f1, f2 = sl.head_inputs(case)
    par = _params(dev, case)
    host = {k: v.detach().cpu().numpy() for k, v in _tensors(par).items()}
    t64, t32 = sl.train_head(host, x, f1, f2, 'float64'), sl.train_head(host, x, f1, f2, 'float32')
    u = t64['stats']['_conv_BN']
    tx = _dev(x, dev, True)
    xo, y = ag.head_block(tx, par, training=True)
    ((xo * _dev(f1, dev)).sum() + (y * _dev(f2, dev)).sum()).backward()
    torch.cuda.synchronize()
    ok = [_within_bar('training x_out', xo, t32['x_out'], t64['x_out']), _within_bar('training y', y, t32['y'], t64['y']),
          _within_bar('training d x', tx.grad, t32['x'], t64['x'])]
    for key in sl.HEAD_TRAINED:
        g = par[key].grad
        assert g is not None and g.shape == par[key].shape, key
        ok.append(_within_bar('training d ' + key, g, t32[key], t64[key]))
    for bn, (mean, var, n) in t64['stats'].items():
        assert n == 2 * 12 * 12 and u[2] == n
        mm, mv = bntrain_ref.moving64(host[bn + '/moving_mean'], host[bn + '/moving_variance'], mean, var, n, ag.HEAD_BN_MOMENTUM)
        for part, want in (('moving_mean', mm), ('moving_variance', mv)):
            got = par['%s/%s' % (bn, part)]
            assert not got.requires_grad and got.grad is None
            assert not np.array_equal(_bits(got), host['%s/%s' % (bn, part)].view(np.uint32)), 'the moving statistics move: %s/%s' % (bn, part)
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-6)
    for key in sl.HEAD_TRAINED:
        assert np.array_equal(_bits(par[key]), host[key].view(np.uint32)), 'no trained parameter changes: ' + key
    assert all(ok)


def test_wider_blocks_raise_the_linear_entries_error(dev):
    """td1's first convolution is 216 -> 512: the 1x1 operators take cout <= 256 today, and say so"""
    ag = _ag()
    case = sl.HEAD_CASES[0]
    par = ag.head_block_parameters(lr.product_net(case[0], sl.head_store(case).values), 'td1', dev)
    cin = 120 + 96
    assert par['_conv'].shape == (512, cin) and '_y' not in par
    with pytest.raises(ValueError, match='cout <= 256'):
        ag.head_block(torch.zeros((1, 3, 3, cin), dtype=torch.float32, device=dev), par, training=False)
    with pytest.raises(ValueError):
        ag.head_block_parameters(lr.product_net(case[0], sl.head_store(case).values), 'td4', dev)
