"""The model's layers that hold a squeeze-excite block, rebuilt from the operators of yoloret_amd/autograd.py, and the two CPU oracles
driven on the same layers: what tests/test_gpu_segrad_autograd.py, tests/test_gpu_head_block.py (device) and tests/test_segrad_host.py
(CPU) share.  It continues tests/layers_ref.py, whose converters, stores and margins it uses:

* ``device_se_block``: EfficientNet's MBConv with se_ratio 0.25 and Swish (efficientnet.py:467-536) composed of autograd.linear1x1,
  autograd.depthwise, autograd.fold_batchnorm + autograd.frozen_bn_act and autograd.squeeze_excite on a ``ParamStore.values`` dictionary;
* drivers of the NumPy oracle (oracle.model.mbconv_block / make_last_layers_efficientnet_lite) and of the torch oracle
  (oracle.torch_ref._Net.mbconv / head_block: output and torch.autograd gradients), gradients in the Keras layouts;
* ``preacts``: the inputs of every ReLU6, Swish and sigmoid of a block, from the NumPy oracle's own primitives;
* ``host_head``: the head block as a float32 chain on the CPU, the stand-in that shows the rounding bar is reachable;
* ``train_head``: the head block with BatchNorm on the statistics of the batch, on torch (float64 or float32), for the training case;
* the case tables with their committed seeds.

Nothing here imports the device runtime at module level; ``device_se_block`` is handed the autograd module."""
import numpy as np
import torch

from oracle import model as om, nn, torch_ref
from tests import bntrain_ref, convgrad_ref as cref, layers_ref as lr, segrad_ref as sref

SE_RATIO = 0.25
# stages 1, 2 and 3 of efficientnet.py on the odd 13 x 11 map: squeeze-excite widths C / R = 32 / 8, 96 / 4, 144 / 6
SE_BLOCKS = [lr.BLOCKS[0], lr.BLOCKS[1], lr.BLOCKS[4]]
SE_BLOCK_IDS = [lr.block_id(c) for c in SE_BLOCKS]
SE_LEAVES = ('se_reduce', 'se_reduce_bias', 'se_expand', 'se_expand_bias')


def reduced(cin):
    return max(1, int(cin * SE_RATIO))


def _se_args(case):
    name, k, s, e, cin, cout = case[:6]
    return om.BlockArgs(kernel_size=k, num_repeat=1, input_filters=cin, output_filters=cout, expand_ratio=e, id_skip=True, strides=[s, s],
                        se_ratio=SE_RATIO)


def numpy_se_block(P, case, x, dtype):
    y = om.mbconv_block(P, case[0], np.asarray(x).astype(dtype), _se_args(case), lite=False)
    assert y.dtype == dtype
    return y


def device_se_block(ag, x, values, name, k, stride, expand, cin, residual):
    """``layers_ref.device_block`` with Swish and the squeeze-excite block behind the depthwise stage -> (y, leaves, frozen); leaves:
    'expand' (when expand != 1), 'dw', 'se_reduce' [C, R], 'se_reduce_bias' [R], 'se_expand' [R, C], 'se_expand_bias' [C], 'project'"""
    dev = x.device

    def leaf(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
    leaves, frozen = {}, []

    def bn_act(z, bn, a):
        stats = [torch.from_numpy(np.ascontiguousarray(values['%s/%s' % (bn, p)], np.float32)).to(dev) for p in lr.BN_PARTS]
        scale, shift = ag.fold_batchnorm(*stats, eps=om.BN_EPS)
        frozen.extend((scale, shift))
        return ag.frozen_bn_act(z, scale, shift, a)
    t = x
    if expand != 1:
        leaves['expand'] = leaf(lr.pack_conv(values[name + '_expand/kernel']))
        t = bn_act(ag.linear1x1(t, leaves['expand']), name + '_expand_BN', 'swish')
    leaves['dw'] = leaf(lr.pack_dw(values[name + '_dw/depthwise_kernel']))
    t = bn_act(ag.depthwise(t, leaves['dw'], stride, 'same'), name + '_dw_BN', 'swish')
    c, r = t.shape[-1], reduced(cin)
    assert values[name + '_se_reduce/kernel'].shape == (1, 1, c, r) and values[name + '_se_expand/kernel'].shape == (1, 1, r, c)
    leaves['se_reduce'], leaves['se_reduce_bias'] = leaf(values[name + '_se_reduce/kernel'][0, 0]), leaf(values[name + '_se_reduce/bias'])
    leaves['se_expand'], leaves['se_expand_bias'] = leaf(values[name + '_se_expand/kernel'][0, 0]), leaf(values[name + '_se_expand/bias'])
    t = ag.squeeze_excite(t, *(leaves[k] for k in SE_LEAVES))
    leaves['project'] = leaf(lr.pack_conv(values[name + '_project/kernel']))
    t = bn_act(ag.linear1x1(t, leaves['project']), name + '_project_BN', None)
    if residual:
        t = t + x
    return t, leaves, frozen


def _keras_grads(net, prefix):
    """the gradients of the torch oracle's cached parameters whose names start with ``prefix`` -> {name without the prefix: array in
    the Keras layout}: '<layer>' [1, 1, cin, cout] or, for a depthwise layer, [k, k, C]; '<layer>/bias' [c]"""
    out = {}
    for key, t in net.cache.items():
        if not key.startswith(prefix) or not isinstance(t, torch.Tensor) or t.grad is None:
            continue
        layer, kind = key[len(prefix):].rsplit('/', 1)
        if kind == 'k':
            out[layer] = t.grad.permute(2, 3, 1, 0).contiguous().numpy()          # [cout, cin, 1, 1] -> [1, 1, cin, cout]
        elif kind == 'dk':
            out[layer] = t.grad.squeeze(1).permute(1, 2, 0).contiguous().numpy()          # [C, 1, k, k] -> [k, k, C]
        else:
            assert kind == 'b'
            out[layer + '/bias'] = t.grad.numpy()
    return out


def _leaves_of(net):
    for key, t in net.cache.items():
        if key.endswith(('/k', '/dk', '/b')):
            t.requires_grad_()


def _nchw(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def torch_se_block(P, case, x, dtype, f):
    """the torch oracle's block (oracle.torch_ref._Net.mbconv, se = 0.25, Swish) in ``dtype`` -> {'y', 'x' (d / d x of (y * f).sum()),
    and per layer of the block ('_expand', '_dw', '_se_reduce', '_se_reduce/bias', ..., '_project') its gradient in the Keras layout}"""
    name, k, s, e, cin, cout = case[:6]
    net = torch_ref._Net(P, dtype)
    xt = _nchw(x, dtype)
    with torch.no_grad():
        net.mbconv(name, xt, k, s, e, cin, cout, SE_RATIO, False)          # (fills the cache)
    _leaves_of(net)
    xt.requires_grad_()
    y = net.mbconv(name, xt, k, s, e, cin, cout, SE_RATIO, False)
    (y * _nchw(f, dtype)).sum().backward()
    out = {'y': _nhwc(y), 'x': _nhwc(xt.grad)}
    out.update(_keras_grads(net, name))
    return out


def preacts(P, name, x, k, s, e, cin, dtype, conv=None):
    """the inputs of a block's activations from the NumPy oracle's primitives, in mbconv_block's order -> [(what, u)]: 'ReLU6 of ..'
    (conv = (layer, filters): the head block's first convolution in front of the MBConv ``name``), 'Swish of ..', 'sigmoid of ..'"""
    t, us = np.asarray(x).astype(dtype), []
    if conv is not None:
        u = om._bn(P, conv[0] + '_BN', om._conv1x1(P, conv[0], t, conv[1]))
        us.append(('ReLU6 of ' + conv[0] + '_BN', u))
        t = nn.relu6(u)
    if e != 1:
        u = om._bn(P, name + '_expand_BN', om._conv1x1(P, name + '_expand', t, cin * e))
        us.append(('Swish of ' + name + '_expand_BN', u))
        t = nn.swish(u)
    u = om._bn(P, name + '_dw_BN', nn.depthwise(t, P.dw(name + '_dw', k, t.shape[-1]), stride=s, padding='same'))
    us.append(('Swish of ' + name + '_dw_BN', u))
    t = nn.swish(u)
    z1 = om._conv1x1(P, name + '_se_reduce', nn.mean_hw(t), reduced(cin), bias=True)
    us.append(('Swish of ' + name + '_se_reduce', z1))
    z2 = om._conv1x1(P, name + '_se_expand', nn.swish(z1), t.shape[-1], bias=True)
    us.append(('sigmoid of ' + name + '_se_expand', z2))
    return us


# ----------------------------------------------------------------------------- the head block (model.py:91-115)
HEAD_F, HEAD_O, HEAD_HW = 128, 3 * (lr.CLASSES + 5), (12, 12)
# (model, block, input channels, seed): the seed draws the input and the two functionals; chosen so that the float64 run's ReLU6 inputs
# stay off the kinks by ``layers_ref.relu6_margins`` (tests/test_segrad_host.py asserts it), never by what the device computes
HEAD_CASES = [('mobilenetv2x75', 'bu3', 75, 0), ('efficientnetb0', 'bu3', 75, 0), ('mobilenetv2x75', 'td3', 248, 1)]      # (td3: seed 0 puts a ReLU6 input 1.0e-05 from a kink, margin 2.7e-05)
HEAD_IDS = ['%s-%s' % c[:2] for c in HEAD_CASES]
# the training-mode case: with BatchNorm on the batch's statistics seed 0 puts a ReLU6 input 4.6e-06 from a kink (margin 1.1e-05); seed 1 is the first that holds
HEAD_TRAIN_CASE = ('mobilenetv2x75', 'bu3', 75, 1)
HEAD_KERNELS = ('_conv', '_mb_dw', '_mb_se_reduce', '_mb_se_reduce/bias', '_mb_se_expand', '_mb_se_expand/bias', '_mb_project', '_y')


def head_kernels(name):
    """the kernels and biases of the block ``name`` in the product's model: the top-down blocks' y convolutions are discarded by
    ``yolov3_body`` (model.py:240-241), so 'td3' has no '_y'"""
    return HEAD_KERNELS if name.startswith('bu') else HEAD_KERNELS[:-1]


def head_inputs(case):
    """-> (x [2, 12, 12, cin], f1, f2 [2, 12, 12, 75]) float32: the input and the functionals of x_out and of y"""
    rng = np.random.default_rng([case[3], case[2]])
    shape = (lr.BATCH,) + HEAD_HW
    return (rng.standard_normal(shape + (case[2],)).astype(np.float32), rng.standard_normal(shape + (HEAD_O,)).astype(np.float32),
            rng.standard_normal(shape + (HEAD_O,)).astype(np.float32))


def head_store(case):
    """the ParamStore of ``layers_ref.rfcr_case``: a ``fresh_store`` whose values are complete for the model's ``yolov3_body``"""
    return lr.rfcr_case(case[0])['P']


def numpy_head(P, name, x, dtype):
    xo, y = om.make_last_layers_efficientnet_lite(P, name, np.asarray(x).astype(dtype), HEAD_F, HEAD_O)
    assert xo.dtype == dtype and y.dtype == dtype
    return xo, y


def head_preacts(P, name, x, dtype):
    return preacts(P, name + '_mb', x, 3, 1, 1, HEAD_F, dtype, conv=(name + '_conv', HEAD_F))


def torch_head(P, name, x, dtype, f1=None, f2=None):
    """oracle.torch_ref._Net.head_block in ``dtype`` -> {'x_out', 'y'}; with the functionals also 'x' (d / d x of
    (x_out * f1).sum() + (y * f2).sum(); a top-down block, whose y the model discards: of (x_out * f1).sum() alone) and the gradients
    of ``head_kernels(name)`` in the Keras layouts"""
    net = torch_ref._Net(P, dtype)
    xt = _nchw(x, dtype)
    with torch.no_grad():
        xo, y = net.head_block(name, xt, HEAD_F, HEAD_O)
    out = {'x_out': _nhwc(xo), 'y': _nhwc(y)}
    if f1 is None:
        return out
    _leaves_of(net)
    xt.requires_grad_()
    xo, y = net.head_block(name, xt, HEAD_F, HEAD_O)
    loss = (xo * _nchw(f1, dtype)).sum()
    if '_y' in head_kernels(name):
        loss = loss + (y * _nchw(f2, dtype)).sum()
    loss.backward()
    out['x'] = _nhwc(xt.grad)
    grads = _keras_grads(net, name)
    assert sorted(grads) == sorted(head_kernels(name)), sorted(grads)
    out.update(grads)
    return out


def host_head(values, name, x):
    """the head block as a float32 chain on the CPU from oracle/nn.py's primitives, the BatchNorms folded in float64 and rounded to
    float32 (``layers_ref.fold32``), the squeeze-excite block by tests/segrad_ref.forward32 in sequential order -> (x_out, y)"""
    def bn(z, b):
        scale, shift = lr.fold32(values, name + b)
        return z * scale + shift
    x = np.ascontiguousarray(x, np.float32)
    t = nn.relu6(bn(nn.pointwise(x, values[name + '_conv/kernel'][0, 0]), '_conv_BN'))
    t = nn.swish(bn(nn.depthwise(t, values[name + '_mb_dw/depthwise_kernel'], 1, 'same'), '_mb_dw_BN'))
    t = sref.forward32(t, values[name + '_mb_se_reduce/kernel'][0, 0], values[name + '_mb_se_reduce/bias'], values[name + '_mb_se_expand/kernel'][0, 0],
                       values[name + '_mb_se_expand/bias'])['y']
    xo = bn(nn.pointwise(t, values[name + '_mb_project/kernel'][0, 0]), '_mb_project_BN')
    y = nn.pointwise(xo, values[name + '_y/kernel'][0, 0])
    assert xo.dtype == np.float32 and y.dtype == np.float32
    return xo, y


def unpack_head_grad(key, g, want_shape):
    """a gradient in the layout of ``autograd.head_block_parameters`` -> the Keras layout of ``torch_head``"""
    g = np.asarray(g)
    if key in ('_conv', '_mb_project', '_y'):
        return lr.unpack_conv(g, want_shape[2])
    if key == '_mb_dw':
        return lr.unpack_dw(g)
    if key in ('_mb_se_reduce', '_mb_se_expand'):
        return g[None, None]
    return g


HEAD_TRAINED = ('_conv', '_conv_BN/gamma', '_conv_BN/beta', '_mb_dw', '_mb_dw_BN/gamma', '_mb_dw_BN/beta', '_mb_se_reduce', '_mb_se_reduce/bias',
                '_mb_se_expand', '_mb_se_expand/bias', '_mb_project', '_mb_project_BN/gamma', '_mb_project_BN/beta', '_y')


def train_head(host, x, f1, f2, dtype):
    """the head block with BatchNorm on the statistics of the batch (training=True) on torch in ``dtype`` ('float64' / 'float32').
    host: {key: array} in the layouts of ``autograd.head_block_parameters`` -> {'x_out', 'y', 'x', the gradients of ``HEAD_TRAINED`` in
    those layouts (pad columns of the 1x1 kernels 0), 'stats': {bn: (mean, biased variance, N)}, 'u': {bn: the BatchNorm's output}}"""
    dt = cref.DT[dtype]
    p = {k: torch.tensor(np.asarray(v, np.float64), dtype=dt, requires_grad=k in HEAD_TRAINED) for k, v in host.items() if k != 'name'}
    xt = torch.tensor(np.asarray(x, np.float64), dtype=dt, requires_grad=True)
    stats, us = {}, {}

    def lin(t, w):
        cin = t.shape[-1]
        return cref._linear(t.reshape(-1, cin), w[:, :cin]).reshape(tuple(t.shape[:-1]) + (w.shape[0],))

    def bn(z, b, act):
        u, _, mean, var, _ = bntrain_ref._forward64(z.reshape(-1, z.shape[-1]), p[b + '/gamma'], p[b + '/beta'], 1e-3)
        stats[b] = (mean.detach().numpy(), var.detach().numpy(), u.shape[0])
        us[b] = u.detach().numpy()
        return cref._act(u, act).reshape(z.shape)
    t = bn(lin(xt, p['_conv']), '_conv_BN', 'relu6')
    t = bn(cref._depthwise(t, p['_mb_dw'], 3, 1, (1, 1, 1, 1)), '_mb_dw_BN', 'swish')
    t = sref.se_torch(t, p['_mb_se_reduce'], p['_mb_se_reduce/bias'], p['_mb_se_expand'], p['_mb_se_expand/bias'])
    xo = bn(lin(t, p['_mb_project']), '_mb_project_BN', None)
    y = lin(xo, p['_y'])
    ((xo * torch.tensor(np.asarray(f1, np.float64), dtype=dt)).sum() + (y * torch.tensor(np.asarray(f2, np.float64), dtype=dt)).sum()).backward()
    out = {'x_out': xo.detach().numpy(), 'y': y.detach().numpy(), 'x': xt.grad.numpy(), 'stats': stats, 'u': us}
    out.update({k: p[k].grad.numpy() for k in HEAD_TRAINED})
    return out
