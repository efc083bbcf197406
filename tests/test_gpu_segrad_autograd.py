"""``autograd.squeeze_excite`` under ``loss.backward()``: against float64 autograd for every subset of {x} and {parameters} that requires
a gradient (the kernels of a gradient nobody asked for are not launched), inside EfficientNet's blocks of stages 1, 2 and 3 against the
project's two CPU oracles, and under a few ``adam_step``s.

The bar is the project's own: max |device - ref64| / max |ref64| <= 4 * E_ref + 2^-24, E_ref the float32 reference's deviation from
float64 on the same inputs (tests/segrad_ref.py's restatement for the operator alone, the float32 torch oracle for the blocks).  Every
comparison prints its figures before it asserts (run with -s).  What the block cases rest on is asserted without a device in
tests/test_segrad_host.py."""
import numpy as np
import pytest
import torch

from tests import layers_ref as lr, segrad_ref as ref, selayers_ref as sl
from tests.test_gpu_autograd import CLASSES, Calls, _ag, _bits, _case, _dev, _rt, _within_bar
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

PARAMS = ('w1', 'b1', 'w2', 'b2')
# which inputs require a gradient: x and all parameters, each alone, neither, and one parameter alone (the batch sums run, three of
# their four results are dropped)
SUBSETS = [(True, PARAMS), (True, ()), (False, PARAMS), (False, ()), (False, ('b1',)), (True, ('w2',))]


@pytest.mark.parametrize('gx,gp', SUBSETS, ids=['x+params', 'x', 'params', 'none', 'b1', 'x+w2'])
def test_squeeze_excite(dev, monkeypatch, gx, gp):
    """Measured on an MI355X (device = E_ref in every figure: the operator returns the restatement's bits), device then bar, x+params:
    y 1.412e-07, 6.243e-07;  dx 1.493e-07, 6.569e-07;  dw1 1.896e-07, 8.181e-07;  db1 1.693e-07, 7.367e-07;  dw2 2.392e-07, 1.017e-06;
    db2 1.753e-07, 7.609e-07."""
    rt = _rt()
    calls = Calls(monkeypatch, ['se_forward', 'se_backward'])
    asked = []
    counted = rt.se_backward
    monkeypatch.setattr(rt, 'se_backward', lambda *a, **kw: asked.append((kw['need_dx'], kw['need_params'])) or counted(*a, **kw))
    b, h, w, c, r = 3, 7, 5, 75, 33
    x, dy, w1, b1, w2, b2 = ref.se_case(b, h, w, c, r, seed=3)
    tx = _dev(x, dev, gx)
    tp = {k: _dev(v, dev, k in gp) for k, v in zip(PARAMS, (w1, b1, w2, b2))}
    y = _ag().squeeze_excite(tx, *(tp[k] for k in PARAMS))
    assert tuple(y.shape) == x.shape and y.requires_grad == (gx or bool(gp))
    if y.requires_grad:
        y.backward(_dev(dy, dev))
    torch.cuda.synchronize()
    assert calls.n == {'se_forward': 1, 'se_backward': int(gx or bool(gp))}
    assert asked == ([(gx, bool(gp))] if (gx or gp) else []), 'the pass over the map and the batch sums run only where a gradient is asked for'
    chunk = rt.se_chunk(b, h * w, c)
    f32 = ref.forward32(x, w1, b1, w2, b2, chunk)
    g32 = ref.backward32(dy, x, w1, w2, f32['m'], f32['z1'], f32['g'], chunk)
    t64 = ref.grads_torch(x, w1, b1, w2, b2, dy)
    ok = [_within_bar('squeeze_excite y', y, f32['y'], t64['y'])]
    if gx:
        ok.append(_within_bar('squeeze_excite dx', tx.grad, g32['dx'], t64['dx']))
    else:
        assert tx.grad is None
    for k in PARAMS:
        if k in gp:
            assert tp[k].grad.shape == tp[k].shape
            ok.append(_within_bar('squeeze_excite d' + k, tp[k].grad, g32['d' + k], t64['d' + k]))
        else:
            assert tp[k].grad is None
    assert all(ok)


def test_saves_only_what_backward_reads(dev):
    """x, w1, w2 and the three small tensors of the forward; the workspace comes from the module's cache"""
    ag = _ag()
    b, h, w, c, r = 2, 5, 4, 32, 8
    x, dy, w1, b1, w2, b2 = ref.se_case(b, h, w, c, r, seed=4)
    before = len(ag._workspaces)
    y = ag.squeeze_excite(_dev(x, dev, True), _dev(w1, dev, True), _dev(b1, dev, True), _dev(w2, dev, True), _dev(b2, dev, True))
    saved = y.grad_fn.saved_tensors
    assert [tuple(t.shape) for t in saved] == [(b, h, w, c), (c, r), (r, c), (b, c), (b, r), (b, c)]
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), _rt().se_workspace_bytes(b, h * w, c, r))
    assert key in ag._workspaces and len(ag._workspaces) <= before + 1


def _se_block_test(dev, case):
    ag = _ag()
    name, k, stride, expand, cin, cout = case[:6]
    what = '%s se 0.25 swish' % lr.block_id(case)
    x, f = lr.block_inputs(case)
    P = lr.fresh_store()
    y64, y32 = sl.numpy_se_block(P, case, x, np.float64), sl.numpy_se_block(P, case, x, np.float32)
    assert max(float(np.abs(u).max()) for _, u in sl.preacts(P, name, x, k, stride, expand, cin, np.float64)) < 87.0, 'u beyond the clamp of expf'
    g64, g32 = sl.torch_se_block(P, case, x, torch.float64, f), sl.torch_se_block(P, case, x, torch.float32, f)
    tx = _dev(x, dev, True)
    y, leaves, frozen = sl.device_se_block(ag, tx, P.values, name, k, stride, expand, cin, lr.is_residual(case))
    assert tuple(y.shape) == f.shape and sorted(leaves) == sorted(['dw', 'project'] + list(sl.SE_LEAVES) + (['expand'] if expand != 1 else []))
    (y * _dev(f, dev)).sum().backward()
    torch.cuda.synchronize()
    ok = [_within_bar(what + ' y', y, y32, y64), _within_bar(what + ' y against the torch oracle', y, g32['y'], g64['y']),
          _within_bar(what + ' d x', tx.grad, g32['x'], g64['x'])]
    for part, leaf in sorted(leaves.items()):
        g = leaf.grad
        assert g is not None and g.shape == leaf.shape, part
        key = '_' + part.replace('_bias', '/bias')
        if part == 'dw':
            got = lr.unpack_dw(g.cpu().numpy())
        elif part in ('expand', 'project'):
            ci = g64[key].shape[2]
            assert not _bits(g[:, ci:]).any(), 'pad columns of d %s are +0' % part
            got = lr.unpack_conv(g.cpu().numpy(), ci)
        elif part in ('se_reduce', 'se_expand'):
            got = g.cpu().numpy()[None, None]
        else:
            got = g.cpu().numpy()
        assert got.shape == g64[key].shape, part
        ok.append(_within_bar('%s d %s' % (what, part), torch.from_numpy(got), g32[key], g64[key]))
    assert all(t.grad is None and not t.requires_grad for t in frozen), 'scale and shift are frozen'
    assert all(ok)


@pytest.mark.parametrize('case', sl.SE_BLOCKS, ids=sl.SE_BLOCK_IDS)
def test_efficientnet_block_with_squeeze_excite(dev, case):
    """EfficientNet's own block (Swish, se_ratio 0.25; squeeze-excite widths C / R = 32 / 8, 96 / 4, 144 / 6) composed from the
    operators: the forward against oracle.model.mbconv_block, d / d x and d / d every kernel and bias of (y * f).sum() against
    torch.autograd over oracle.torch_ref._Net.mbconv, mapped back to the Keras layouts.
    Measured on an MI355X (device, E_ref, bar), the forward and the extremes of the ten or eleven gradients of a block:
      stage1_block0  y 2.200e-07, 2.609e-07, 1.103e-06;  d se_reduce_bias 7.682e-08, 1.212e-07, 5.445e-07;  d se_expand 2.937e-07, 5.787e-07, 2.374e-06
      stage2_block0  y 3.309e-07, 3.666e-07, 1.526e-06;  d expand 2.015e-07, 2.356e-07, 1.002e-06;  d se_expand 4.621e-07, 2.663e-07, 1.125e-06
      stage3_block0  y 3.824e-07, 4.444e-07, 1.837e-06;  d project 2.011e-07, 2.490e-07, 1.056e-06;  d x 7.427e-07, 3.250e-07, 1.360e-06
    (34 comparisons, device 7.7e-08 to 7.4e-07; the closest to its bar: stage3_block0's d x, 0.55 of it)."""
    _se_block_test(dev, case)


def test_adam_steps_lower_the_loss(dev):
    """depthwise 3 x 3 -> BN + Swish -> squeeze_excite (C 75, R 18) -> 1x1 -> YoloLoss on the finest scale's device features of
    tests/test_gpu_autograd._case; six Adam steps at 1e-3 on the depthwise taps, the four squeeze-excite parameters and the 1x1 kernel.
    Measured on an MI355X, the loss before each step: 289.3290 276.6485 264.4133 251.7980 239.8774 228.8940."""
    from yoloret_amd.yolo3.model import YoloLoss
    ag, rt = _ag(), _rt()
    f, y_np, init = _case(dev)
    s, c, r = 2, 75, 18
    rng = np.random.default_rng(9)
    par = {'dw': init[s]['dw'], 'wt': init[s]['wt1'], 'w1': (rng.standard_normal((c, r)) / np.sqrt(c)).astype(np.float32), 'b1': np.zeros(r, np.float32),
           'w2': (rng.standard_normal((r, c)) / np.sqrt(r)).astype(np.float32), 'b2': np.zeros(c, np.float32)}
    leaves = {k: _dev(v, dev, True) for k, v in par.items()}
    scale, shift = _dev(init[s]['scale1'], dev), _dev(init[s]['shift1'], dev)
    feats = _dev(f[s], dev)
    moments = {k: (torch.zeros_like(w), torch.zeros_like(w)) for k, w in leaves.items()}
    losses = []
    for t in range(1, 7):
        a = ag.frozen_bn_act(ag.depthwise(feats, leaves['dw'], 1, 'same'), scale, shift, 'swish')
        a = ag.squeeze_excite(a, leaves['w1'], leaves['b1'], leaves['w2'], leaves['b2'])
        out = ag.linear1x1(a, leaves['wt'])
        loss = YoloLoss(s, ANCHORS, 3, print_loss=False).call(y_np[s], out.reshape(out.shape[:3] + (3, 5 + CLASSES)))
        grads = torch.autograd.grad(loss, list(leaves.values()))
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
        if t == 1:
            assert all(float(g.abs().max()) > 0 for g in grads), 'every parameter, the squeeze-excite ones included, is reached by the loss'
        with torch.no_grad():
            for (k, w), g in zip(leaves.items(), grads):
                rt.adam_step(w, moments[k][0], moments[k][1], g.contiguous(), rt.adam_alpha(1e-3, t))
        losses.append(float(loss.detach()))
    print('losses before each step: ' + ' '.join('%.4f' % v for v in losses))
    assert losses[-1] < losses[0], losses
