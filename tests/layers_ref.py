"""The layers of the shipped network rebuilt from the operators of yoloret_amd/autograd.py, and the two CPU oracles driven on the same
layers: what tests/test_gpu_layers_oracle.py (device) and tests/test_layers_ref_host.py (CPU) share.

* the layout converters, written from the layouts autograd.py's module text documents: a Keras Conv2D kernel [1, 1, cin, cout] is the
  operators' wt [cout, round_up(cin, 4)] with pad columns +0, a DepthwiseConv2D kernel [k, k, C, 1] (the parameter store keeps it
  squeezed, [k, k, C]) is w [k * k, C]; the inverses map a gradient back to the Keras layout;
* ``device_block``: one inverted-residual / MBConv block (no squeeze-excite) composed of autograd.linear1x1, autograd.depthwise(...,
  'same'), autograd.fold_batchnorm + autograd.frozen_bn_act and a torch add, on a ``ParamStore.values`` dictionary;
* ``host_block``: the same chain in float32 on the CPU from oracle/nn.py's primitives, the BatchNorms folded in float64 and rounded to
  float32, in the operators' documented order: the stand-in that shows the rounding bar is reachable by a correct float32 chain;
* drivers of the NumPy oracle (oracle/model.py) and of the torch oracle (oracle/torch_ref.py: output and torch.autograd gradients),
  both returning plain NHWC arrays and gradients in the Keras layouts;
* ``relu6_margins`` / ``preactivations``: how far the float64 run's ReLU6 inputs stay from 0 and 6, the convention of
  tests/test_gpu_fusegrad_autograd.margins;
* the case tables with their committed seeds.

Nothing here imports the device runtime at module level; ``device_block`` is handed the autograd module."""
import numpy as np
import torch

from oracle import model as om, nn, params, torch_ref

BN_PARTS = ('gamma', 'beta', 'moving_mean', 'moving_variance')
WEIGHT_SEED, RECIPE = 1234, 'conditioned'
_shared = {}


# ----------------------------------------------------------------------------- layouts
def pack_conv(kernel):
    """Keras [1, 1, cin, cout] -> wt [cout, round_up(cin, 4)] float32, pad columns +0"""
    kernel = np.asarray(kernel, np.float32)
    assert kernel.ndim == 4 and kernel.shape[:2] == (1, 1), kernel.shape
    cin, cout = kernel.shape[2:]
    wt = np.zeros((cout, (cin + 3) // 4 * 4), np.float32)
    wt[:, :cin] = kernel[0, 0].T
    return wt


def unpack_conv(wt, cin):
    """wt [cout, round_up(cin, 4)] -> Keras [1, 1, cin, cout] (the pad columns are dropped)"""
    wt = np.asarray(wt)
    assert wt.ndim == 2 and wt.shape[1] == (cin + 3) // 4 * 4, (wt.shape, cin)
    return np.ascontiguousarray(wt[:, :cin].T)[None, None]


def pack_dw(kernel):
    """Keras [k, k, C, 1], or squeezed [k, k, C] -> w [k * k, C]: tap (ky, kx) is row ky * k + kx"""
    kernel = np.asarray(kernel, np.float32)
    if kernel.ndim == 4:
        assert kernel.shape[3] == 1, kernel.shape
        kernel = kernel[..., 0]
    k, k2, c = kernel.shape
    assert k == k2 and k in (3, 5), kernel.shape
    return np.ascontiguousarray(kernel.reshape(k * k, c))


def unpack_dw(w):
    """w [k * k, C] -> [k, k, C]"""
    w = np.asarray(w)
    k = {9: 3, 25: 5}[w.shape[0]]
    return np.ascontiguousarray(w.reshape(k, k, w.shape[1]))


# ----------------------------------------------------------------------------- names
def effnet_names(name):
    """the layer names of efficientnet.py's block ``name`` ('stage2_block0')"""
    return dict(expand=name + '_expand', expand_bn=name + '_expand_BN', dw=name + '_dw', dw_bn=name + '_dw_BN',
                project=name + '_project', project_bn=name + '_project_BN')


def mbv2_names(block):
    """the Keras names of MobileNetV2's block ``block`` (0: 'expanded_conv_', which has no expand convolution)"""
    p = 'expanded_conv_' if block == 0 else 'block_%d_' % block
    return dict(expand=p + 'expand', expand_bn=p + 'expand_BN', dw=p + 'depthwise', dw_bn=p + 'depthwise_BN',
                project=p + 'project', project_bn=p + 'project_BN')


# ----------------------------------------------------------------------------- the block on the device
def device_block(ag, x, values, names, k, stride, expand, act, residual):
    """One block from the operators of ``ag`` (yoloret_amd.autograd): [1x1 expand -> BN -> act] -> k x k depthwise, 'same' -> BN -> act
    -> 1x1 project -> BN [-> + x].  x: a float32 device tensor [B, H, W, cin]; values: ``ParamStore.values``; names: ``effnet_names`` /
    ``mbv2_names``; the expand convolution is absent when expand == 1; act 'relu6' | 'swish'.
    -> (y, leaves, frozen): leaves {'expand', 'dw', 'project'} are the kernels in the operators' layouts, requiring a gradient;
    frozen are the folded scale / shift tensors, which must never get one."""
    dev = x.device

    def leaf(a):
        return torch.from_numpy(a).to(dev).requires_grad_(True)
    leaves, frozen = {}, []

    def bn_act(z, bn, a):
        stats = [torch.from_numpy(np.ascontiguousarray(values['%s/%s' % (bn, p)], np.float32)).to(dev) for p in BN_PARTS]
        scale, shift = ag.fold_batchnorm(*stats, eps=om.BN_EPS)
        frozen.extend((scale, shift))
        return ag.frozen_bn_act(z, scale, shift, a)
    t = x
    if expand != 1:
        kernel = values[names['expand'] + '/kernel']
        assert kernel.shape == (1, 1, x.shape[-1], expand * x.shape[-1]), kernel.shape
        leaves['expand'] = leaf(pack_conv(kernel))
        t = bn_act(ag.linear1x1(t, leaves['expand']), names['expand_bn'], act)
    taps = values[names['dw'] + '/depthwise_kernel']
    assert taps.shape[:2] == (k, k), taps.shape
    leaves['dw'] = leaf(pack_dw(taps))
    t = bn_act(ag.depthwise(t, leaves['dw'], stride, 'same'), names['dw_bn'], act)
    leaves['project'] = leaf(pack_conv(values[names['project'] + '/kernel']))
    t = bn_act(ag.linear1x1(t, leaves['project']), names['project_bn'], None)
    if residual:
        assert stride == 1 and t.shape == x.shape
        t = t + x
    return t, leaves, frozen


# ----------------------------------------------------------------------------- the same chain in float32 on the CPU
def fold32(values, bn):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale in float64, rounded to float32 (autograd.fold_batchnorm)"""
    g, b, m, v = (np.asarray(values['%s/%s' % (bn, p)], np.float64) for p in BN_PARTS)
    scale = g / np.sqrt(v + om.BN_EPS)
    return scale.astype(np.float32), (b - m * scale).astype(np.float32)


def host_block(x, values, names, k, stride, expand, act, residual):
    """``device_block``'s chain on oracle/nn.py's primitives in float32: x [B, H, W, cin] float32 -> y float32"""
    f = {'relu6': nn.relu6, 'swish': nn.swish, None: lambda u: u}

    def bn_act(z, bn, a):
        scale, shift = fold32(values, bn)
        out = f[a](z * scale + shift)
        assert out.dtype == np.float32
        return out
    x = np.ascontiguousarray(x, np.float32)
    t = x
    if expand != 1:
        t = bn_act(nn.pointwise(t, values[names['expand'] + '/kernel'][0, 0]), names['expand_bn'], act)
    t = bn_act(nn.depthwise(t, values[names['dw'] + '/depthwise_kernel'], stride, 'same'), names['dw_bn'], act)
    t = bn_act(nn.pointwise(t, values[names['project'] + '/kernel'][0, 0]), names['project_bn'], None)
    return t + x if residual else t


# ----------------------------------------------------------------------------- the EfficientNet block table
# (name, k, stride, expand, cin, cout, H, W, seed): efficientnet.py's stages 1-3 on the smallest maps that carry every class of 'same'
# padding.  The seed draws the input and the functional of the gradient test; it is chosen so that ``relu6_margins`` holds
# (tests/test_layers_ref_host.py asserts it), never by what the device computes.
BLOCKS = [
    ('stage1_block0', 3, 1, 1, 32, 16, 13, 11, 0),      # no expand convolution
    ('stage2_block0', 3, 2, 6, 16, 24, 13, 11, 0),      # odd map: pads 1 / 1
    ('stage2_block0', 3, 2, 6, 16, 24, 12, 10, 0),      # even map: pads 0 / 1
    ('stage2_block1', 3, 1, 6, 24, 24, 7, 9, 2),        # residual: the input fans out
    ('stage3_block0', 5, 2, 6, 24, 40, 13, 11, 0),      # odd map: pads 2 / 2
    ('stage3_block0', 5, 2, 6, 24, 40, 12, 10, 0),      # even map: pads 1 / 2
    ('stage3_block1', 5, 1, 6, 40, 40, 7, 5, 1),        # residual, 240 expanded channels
]
BATCH = 2


def block_id(case):
    return '%s-k%ds%de%d-%dx%d' % (case[0], case[1], case[2], case[3], case[6], case[7])


def is_residual(case):
    return case[2] == 1 and case[4] == case[5]


def out_hw(case):
    s = case[2]
    return -(-case[6] // s), -(-case[7] // s)


def block_inputs(case):
    """-> (x [2, H, W, cin], f [2, OH, OW, cout]) float32 standard normals of the case's seed"""
    rng = np.random.default_rng(case[8])
    x = rng.standard_normal((BATCH, case[6], case[7], case[4])).astype(np.float32)
    f = rng.standard_normal((BATCH,) + out_hw(case) + (case[5],)).astype(np.float32)
    return x, f


def fresh_store():
    return params.ParamStore(WEIGHT_SEED, RECIPE)


def _args(case):
    name, k, s, e, cin, cout = case[:6]
    return om.BlockArgs(kernel_size=k, num_repeat=1, input_filters=cin, output_filters=cout, expand_ratio=e, id_skip=True,
                        strides=[s, s], se_ratio=None)


def numpy_block(P, case, x, lite, dtype):
    """the NumPy oracle's block output (oracle.model.mbconv_block, no squeeze-excite; lite: ReLU6, else Swish) in ``dtype``"""
    y = om.mbconv_block(P, case[0], np.asarray(x).astype(dtype), _args(case), lite=lite)
    assert y.dtype == dtype
    return y


def preactivations(P, case, x, lite, dtype):
    """the inputs of the block's activations, from the NumPy oracle's own primitives in mbconv_block's order
    -> ([(BatchNorm name, u)], y); y is bit for bit ``numpy_block``'s (tests/test_layers_ref_host.py asserts it)"""
    name, k, s, e, cin, cout = case[:6]
    act = nn.relu6 if lite else nn.swish
    x = np.asarray(x).astype(dtype)
    t, us = x, []
    if e != 1:
        u = om._bn(P, name + '_expand_BN', om._conv1x1(P, name + '_expand', t, cin * e))
        us.append((name + '_expand_BN', u))
        t = act(u)
    u = om._bn(P, name + '_dw_BN', nn.depthwise(t, P.dw(name + '_dw', k, t.shape[-1]), stride=s, padding='same'))
    us.append((name + '_dw_BN', u))
    t = om._bn(P, name + '_project_BN', om._conv1x1(P, name + '_project', act(u), cout))
    return us, (t + x if is_residual(case) else t)


def relu6_margins(us64, us32):
    """-> [(what, the float64 run's smallest distance from 0 and from 6, 8 x the float32 run's largest deviation at that tensor)]"""
    out = []
    for (bn, u64), (bn32, u32) in zip(us64, us32):
        assert bn == bn32 and u64.dtype == np.float64 and u32.dtype == np.float32
        out.append(('ReLU6 of ' + bn, float(min(np.abs(u64).min(), np.abs(u64 - 6).min())), 8 * float(np.abs(u32 - u64).max())))
    return out


def torch_block(P, case, x, lite, dtype, f=None):
    """the torch oracle's block (oracle.torch_ref._Net.mbconv, se = 0) in ``dtype`` (a torch dtype) -> {'y': NHWC array}; with f
    (NHWC, the functional) also the gradients of (y * f).sum(): 'x' NHWC, and 'expand' / 'project' [1, 1, cin, cout] and 'dw'
    [k, k, C], the Keras layouts"""
    name, k, s, e, cin, cout = case[:6]
    net = torch_ref._Net(P, dtype)
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        y = net.mbconv(name, xt, k, s, e, cin, cout, 0, lite)
    out = {'y': y.permute(0, 2, 3, 1).contiguous().numpy()}
    if f is None:
        return out
    kernels = {key: t.requires_grad_() for key, t in net.cache.items() if key.endswith(('/k', '/dk'))}
    assert sorted(kernels) == sorted([name + '_dw/dk', name + '_project/k'] + ([name + '_expand/k'] if e != 1 else []))
    xt.requires_grad_()
    y = net.mbconv(name, xt, k, s, e, cin, cout, 0, lite)
    ft = torch.from_numpy(np.ascontiguousarray(f)).to(dtype).permute(0, 3, 1, 2)
    (y * ft).sum().backward()
    out['x'] = xt.grad.permute(0, 2, 3, 1).contiguous().numpy()
    for part in ('expand', 'project'):
        t = kernels.get('%s_%s/k' % (name, part))
        if t is not None:
            out[part] = t.grad.permute(2, 3, 1, 0).contiguous().numpy()      # [cout, cin, 1, 1] -> [1, 1, cin, cout]
    out['dw'] = kernels[name + '_dw/dk'].grad.squeeze(1).permute(1, 2, 0).contiguous().numpy()      # [C, 1, k, k] -> [k, k, C]
    return out


# ----------------------------------------------------------------------------- the RFCR module on the model's own taps
RFCR_MODELS = ('mobilenetv2x75', 'efficientnetb0')
RFCR_HW, CLASSES = (96, 96), 20


def rfcr_case(model_name):
    """-> dict, computed once and left unchanged: P (a ParamStore whose ``values`` is complete for ``yolov3_body``), taps (the NumPy
    oracle's b1 .. b4 on 2 synthetic images at 96 x 96, float32), want64 / want32 (oracle.model.rfcr_module on these taps)"""
    key = ('rfcr', model_name)
    if key not in _shared:
        P = fresh_store()
        x = params.synthetic_images(BATCH, RFCR_HW[0], RFCR_HW[1])
        om.yolov3_body(P, x, model_name, 3, CLASSES)
        taps = [np.ascontiguousarray(t, np.float32) for t in om.backbone_taps(P, x, model_name)]
        want64 = om.rfcr_module(P, [t.astype(np.float64) for t in taps])
        want32 = om.rfcr_module(P, taps)
        assert all(w.dtype == np.float64 for w in want64) and all(w.dtype == np.float32 for w in want32)
        _shared[key] = dict(P=P, taps=taps, want64=want64, want32=want32)
    return _shared[key]


def product_net(model_name, values):
    """the product's graph of ``model_name`` at 96 x 96 with ``values`` as its weights (no device is touched)"""
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3.model import yolov3_body
    net = yolov3_body(L.Input(shape=[RFCR_HW[0], RFCR_HW[1], 3]), model_name, 3, num_classes=CLASSES)
    net.set_weights(values)
    return net


# ----------------------------------------------------------------------------- MobileNetV2 x0.75's first three blocks
MBV2_IMAGES = ((64, 64), (50, 38))
MBV2_CHAIN = ((0, 1, 1, False, 'block_0_out'), (1, 2, 6, False, 'block_1_out'), (2, 1, 6, True, 'block_2_add'))      # (block, stride, expand, residual, output)


def mbv2_case(hw):
    """-> dict, computed once: P, acts64 / acts32 (oracle.model.mobilenet_v2(alpha 0.75, last_block 2) on 2 synthetic images)"""
    key = ('mbv2',) + tuple(hw)
    if key not in _shared:
        P = fresh_store()
        x = params.synthetic_images(BATCH, hw[0], hw[1])
        acts64 = om.mobilenet_v2(P, x.astype(np.float64), 0.75, last_block=2)
        acts32 = om.mobilenet_v2(P, x, 0.75, last_block=2)
        _shared[key] = dict(P=P, acts64=acts64, acts32=acts32)
    return _shared[key]
