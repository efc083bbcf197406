"""``autograd.conv1x1`` (the 1x1 convolution of any width up to 1024, csrc/linearwide.hip) and ``autograd.head_block(wide=True)`` on the
device.

* at widths both accept, ``conv1x1`` IS ``linear1x1``: the same entries and the same bytes, forward and both gradients;
* at the widths of td1 of MobileNetV2 x0.75 (216 -> 512 and 512 -> 75) both gradients against float64 torch autograd within the
  project's bar, max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the float32 torch run's deviation on the same data;
* a gradient that is not required is None and its entry is not called;
* ``head_block(wide=True)`` on td1 of MobileNetV2 x0.75 (216 -> 512 -> 75 on 2 images at 3 x 3, the map td1 has at 96 x 96) against
  oracle.torch_ref._Net.head_block in float64 with tests/selayers_ref.py's machinery, forward and every gradient.  The seed of the case
  keeps ReLU6's inputs off its kinks (tests/test_neck_host.py asserts it).

Every comparison prints its figures before it asserts (run with -s); the measured ones are in the docstrings."""
import numpy as np
import pytest
import torch

from oracle import torch_ref
from tests import convgrad_ref as cref, layers_ref as lr, neck_ref as nr, selayers_ref as sl
from tests.test_gpu_autograd import Calls, _bits, _dev, _within_bar

pytestmark = pytest.mark.gpu

WIDE_ENTRIES = ('linear_wide_forward', 'linear_wide_dgrad', 'linear_wide_wgrad')
NARROW_ENTRIES = ('linear_forward', 'linear_dgrad', 'linear_wgrad')


def _ag():
    from yoloret_amd import autograd
    return autograd


def _rt():
    from yoloret_amd import runtime
    return runtime


def _case(seed, pixels_shape, cin, cout):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(pixels_shape + (cin,)).astype(np.float32)
    w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    dy = rng.standard_normal(pixels_shape + (cout,)).astype(np.float32)
    return x, w, dy


def test_narrow_widths_are_linear1x1(dev, monkeypatch):
    ag = _ag()
    x, w, dy = _case(75, (2, 5, 7), 75, 75)
    calls = Calls(monkeypatch, WIDE_ENTRIES + NARROW_ENTRIES)
    res = []
    for f in (ag.conv1x1, ag.linear1x1):
        tx, tw = _dev(x, dev, True), _dev(cref.pack_wt(w), dev, True)
        y = f(tx, tw)
        y.backward(_dev(dy, dev))
        res.append((y, tx.grad, tw.grad))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert np.array_equal(_bits(a), _bits(b))
    assert all(calls.n[k] == 0 for k in WIDE_ENTRIES) and all(calls.n[k] == 2 for k in NARROW_ENTRIES)


@pytest.mark.parametrize('cin,cout', [(216, 512), (512, 75)])
def test_wide_gradients_against_float64(dev, monkeypatch, cin, cout):
    """Measured on an MI355X (device, E_ref, bar), 2 x 9 x 9 pixels:
    216 -> 512  y 5.251e-07, 5.251e-07, 2.160e-06;  d x 1.119e-06, 1.119e-06, 4.536e-06;  d wt 4.666e-07, 4.666e-07, 1.926e-06
    512 -> 75   y 7.445e-07, 7.445e-07, 3.038e-06;  d x 3.262e-07, 3.262e-07, 1.365e-06;  d wt 2.967e-07, 4.608e-07, 1.903e-06"""
    ag = _ag()
    x, w, dy = _case(cin, (2, 9, 9), cin, cout)
    x2, dy2 = x.reshape(-1, cin), dy.reshape(-1, cout)
    y64 = cref.linear(x2, w)
    dx64, dw64 = cref.linear_grads(x2, w, dy2)
    dx32, dw32 = cref.linear_grads(x2, w, dy2, np.float32)
    calls = Calls(monkeypatch, WIDE_ENTRIES + NARROW_ENTRIES)
    tx, tw = _dev(x, dev, True), _dev(cref.pack_wt(w), dev, True)
    y = ag.conv1x1(tx, tw)
    y.backward(_dev(dy, dev))
    torch.cuda.synchronize()
    assert all(calls.n[k] == 1 for k in WIDE_ENTRIES) and all(calls.n[k] == 0 for k in NARROW_ENTRIES)
    kp = (cin + 3) // 4 * 4
    assert tw.grad.shape == (cout, kp) and not _bits(tw.grad[:, cin:]).any(), 'pad columns of d wt are +0'
    what = 'conv1x1 %d->%d ' % (cin, cout)
    ok = [_within_bar(what + 'y', y.reshape(-1, cout), cref.linear(x2, w, np.float32), y64),
          _within_bar(what + 'd x', tx.grad.reshape(-1, cin), dx32, dx64),
          _within_bar(what + 'd wt', tw.grad[:, :cin], dw32, dw64)]
    assert all(ok)


def test_gradients_that_are_not_required_are_not_computed(dev, monkeypatch):
    ag, rt = _ag(), _rt()
    x, w, dy = _case(3, (40,), 300, 260)
    calls = Calls(monkeypatch, WIDE_ENTRIES)
    for need_x, need_w in ((True, False), (False, True)):
        before = dict(calls.n)
        tx, tw = _dev(x, dev, need_x), _dev(cref.pack_wt(w), dev, need_w)
        y = ag.conv1x1(tx, tw)
        torch.cuda.synchronize()
        assert rt.lib().yr_last_kernel().decode().startswith('lw_product_kernel<') and rt.lib().yr_last_kernel().decode().endswith(',0>')
        # yr_last_kernel is per thread and torch runs backward on a thread of its own: a hook on the one gradient that is computed reads
        # it there, right after _LinearWide.backward returned.  The weight gradient is launched after the input gradient, so the input
        # gradient's kernel as the LAST one shows that no stage 1 followed it; the other way round the name cannot tell (the weight
        # gradient is last in any case), and the entries' calls are counted - which sees no launch made beneath a wrapper
        seen = []
        (tx if need_x else tw).register_hook(lambda g: seen.append(rt.lib().yr_last_kernel().decode()))
        y.backward(_dev(dy, dev))
        torch.cuda.synchronize()
        assert (tx.grad is not None) == need_x and (tw.grad is not None) == need_w
        assert len(seen) == 1 and (seen[0].startswith('lw_product_kernel<') and seen[0].endswith(',1>') if need_x
                                   else seen[0].startswith('lw_wgrad_partial_kernel<'))
        assert calls.n['linear_wide_dgrad'] - before['linear_wide_dgrad'] == int(need_x)
        assert calls.n['linear_wide_wgrad'] - before['linear_wide_wgrad'] == int(need_w)
        assert rt.lib().yr_last_kernel().decode().endswith(',0>'), 'this thread launched nothing after the forward'
    with pytest.raises(ValueError):
        ag.conv1x1(_dev(np.zeros((4, 1025), np.float32), dev), _dev(np.zeros((8, 1028), np.float32), dev))


def test_wide_head_block_is_the_oracles(dev):
    """``head_block(wide=True, training=False)`` on td1 of MobileNetV2 x0.75 (the block ``head_block`` refuses by default): x_out
    against oracle.torch_ref._Net.head_block in float64 (E_ref: the same in float32), the gradients of (x_out * f1).sum() for the input
    and every kernel and bias against torch.autograd over it, mapped back to the Keras layouts; y is None (a top-down block); gamma
    and beta are folded and get no gradient; no parameter changes.
    Measured on an MI355X (device, E_ref, bar): x_out 1.113e-06, 6.536e-07, 2.674e-06 (the closest to its bar, 0.42 of it);
    d x 4.306e-07, 4.055e-07, 1.682e-06;  d _conv 1.978e-07, 2.037e-07, 8.744e-07;  d _mb_dw 3.270e-07, 2.646e-07, 1.118e-06;
    d _mb_se_reduce 5.922e-07, 5.510e-07, 2.264e-06;  d _mb_se_reduce/bias 5.580e-07, 4.992e-07, 2.056e-06;  d _mb_se_expand 4.164e-07, 3.803e-07,
    1.581e-06;  d _mb_se_expand/bias 3.230e-07, 2.595e-07, 1.098e-06;  d _mb_project 3.844e-07, 3.033e-07, 1.273e-06"""
    ag = _ag()
    model_name, name, cin, f = nr.TD1_CASE[:4]
    x, f1 = nr.td1_inputs()
    P = lr.rfcr_case(model_name)['P']

    def oracle(dtype):
        net = torch_ref._Net(P, dtype)
        xt = sl._nchw(x, dtype)
        with torch.no_grad():
            net.head_block(name, xt, f, sl.HEAD_O)      # (fills the cache; the oracle's own y convolution is not the model's)
        sl._leaves_of(net)
        xt.requires_grad_()
        xo, _ = net.head_block(name, xt, f, sl.HEAD_O)
        (xo * sl._nchw(f1, dtype)).sum().backward()
        out = {'x_out': sl._nhwc(xo), 'x': sl._nhwc(xt.grad)}
        out.update({k: v for k, v in sl._keras_grads(net, name).items() if k != '_y'})
        return out
    t64, t32 = oracle(torch.float64), oracle(torch.float32)
    kernels = sl.head_kernels(name)
    assert sorted(k for k in t64 if k.startswith('_')) == sorted(kernels)
    par = ag.head_block_parameters(lr.product_net(model_name, P.values), name, dev)
    assert par['_conv'].shape == (f, cin) and par['_mb_project'].shape == (sl.HEAD_O, f) and '_y' not in par
    tensors = {k: v for k, v in par.items() if k != 'name'}
    before = {k: v.detach().clone() for k, v in tensors.items()}
    tx = _dev(x, dev, True)
    with pytest.raises(ValueError, match='cout <= 256'):
        ag.head_block(tx, par, training=False)      # the default is today's function
    xo, y = ag.head_block(tx, par, training=False, wide=True)
    assert y is None and tuple(xo.shape) == (2, 3, 3, sl.HEAD_O)
    (xo * _dev(f1, dev)).sum().backward()
    torch.cuda.synchronize()
    ok = [_within_bar('td1 x_out', xo, t32['x_out'], t64['x_out']), _within_bar('td1 d x', tx.grad, t32['x'], t64['x'])]
    for key in kernels:
        g = par[key].grad
        assert g is not None and g.shape == par[key].shape, key
        if key in ('_conv', '_mb_project'):
            assert not _bits(g[:, t64[key].shape[2]:]).any(), 'pad columns of d %s are +0' % key
        got = sl.unpack_head_grad(key, g.cpu().numpy(), t64[key].shape)
        assert got.shape == t64[key].shape, key
        ok.append(_within_bar('td1 d %s' % key, torch.from_numpy(np.ascontiguousarray(got)), t32[key], t64[key]))
    for key, v in tensors.items():
        assert key in kernels or v.grad is None, 'the folded BatchNorms take no gradient: ' + key
        assert np.array_equal(_bits(v), _bits(before[key])), 'nothing is updated: ' + key
    assert all(ok)
