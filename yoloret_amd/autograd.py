"""The backward operators of csrc/convgrad.hip and csrc/headtrain.hip behind ``torch.autograd``: a stack of bias-free 1x1
convolutions, depthwise convolutions and frozen BatchNorm + activation on top of ``yolov3_features`` trains with ``YoloLoss.call``
(itself an autograd Function) and ``runtime.adam_step``.

    linear1x1(x, wt)                        x [..., cin], wt [cout, round_up(cin, 4)] (pad columns 0) -> [..., cout]; cin, cout <= 256
    conv1x1(x, wt)                          the same at any width up to 1024 (csrc/linearwide.hip); linear1x1 itself where both are <= 256
    depthwise(x, w, stride=1, padding='same')   x [B, H, W, C], w [k * k, C] (the Keras kernel [k, k, C, 1] reshaped), k in {3, 5}
    conv3x3(x, w, stride=1, padding='same')     the network entry (csrc/stemgrad.hip): x [B, H, W, cin], w [9 * cin, cout] (the Keras kernel
                                            [3, 3, cin, cout] reshaped), cin in 1..4, cout in 1..64; differentiable in the image too
    frozen_bn_act(z, scale, shift, act)     act in {None, 'relu6', 'swish'}; scale and shift are frozen: they never get a gradient
    batchnorm_act(z, gamma, beta, moving_mean, moving_var, momentum, eps, act)   BatchNorm in training mode (csrc/bntrain.hip): batch
                                            statistics, gradients for z, gamma and beta, the moving statistics updated in place
    fold_batchnorm(gamma, beta, moving_mean, moving_var, eps) -> (scale, shift) for frozen_bn_act: how a trained layer is evaluated
    maxpool(x, k=2), upsample2(x)           Keras MaxPooling2D((k, k)), k in {2, 4}, and UpSampling2D() (csrc/fusegrad.hip)
    weighted_sum(xs, alpha)                 the reference's WeightedSum of four maps, alpha float32 [4], differentiable in all five
    concat(xs)                              Keras Concatenate() over the channels
    rfcr_module(b1, b2, b3, b4, params, training=True), rfcr_parameters(model, device)   the RFCR module (model.py:146-168) of these
    squeeze_excite(x, w1, b1, w2, b2)       the squeeze-excite block (efficientnet.py:406-438; csrc/segrad.hip): x [B, H, W, C], w1 [C, R],
                                            b1 [R], w2 [R, C], b2 [C] -> x * sigmoid(swish(mean(x) w1 + b1) w2 + b2), differentiable in all five
    head_block(x, params, training=True, wide=False), head_block_parameters(model, name, device)   a head block (model.py:91-115) of
                                            these; wide=True: its 1x1 convolutions through conv1x1
    detector_neck(b1, b2, b3, b4, params, training=True), neck_parameters(model, device), neck_weights(params)   everything yolov3_body
                                            runs behind the backbone (model.py:226-340), its parameters, and their way back into the model
    mobilenetv2_stem / mobilenetv2_block / mobilenetv2_backbone(images, params, training=True), mobilenetv2_parameters(model, device),
    backbone_weights(params)                the MobileNetV2 backbone (code/yolo3/model.py:180-190) of these operators, trained like everything else
    detector(images, params, training=True), detector_parameters(model, device), detector_weights(params)   the backbone plus the neck: images -> logits

Written the way ``_YoloLossFunction`` of yolo3/model.py is: forward and backward are calls of the C entries, only what backward needs
is saved, a gradient is computed only for an input that requires one (the others are None and their kernel is not launched).  float32
CUDA tensors only; there is no fallback.  Workspaces of the two-stage weight gradients are cached per device and size."""
import numpy as np
import torch

from . import runtime as rt

_workspaces = {}


def _workspace(dev, nbytes):
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), int(nbytes))
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=dev)
    return ws


def _f32(g):
    return g.to(torch.float32).contiguous()


class _Linear(torch.autograd.Function):
    """The body of ``_Linear1x1`` and ``_LinearWide``.  A subclass names its four functions of ``runtime``: the forward, the input
    gradient, the weight gradient and its workspace size.  They are looked up there at every call."""
    entries = None

    @classmethod
    def forward(cls, ctx, x, wt):
        ctx.save_for_backward(x, wt)
        return getattr(rt, cls.entries[0])(x, wt)

    @classmethod
    def backward(cls, ctx, dy):
        _, dgrad, wgrad, workspace_bytes = (getattr(rt, name) for name in cls.entries)
        x, wt = ctx.saved_tensors
        dy = _f32(dy)
        dx = dwt = None
        if ctx.needs_input_grad[0]:
            dx = dgrad(dy, wt, x.shape[-1])
        if ctx.needs_input_grad[1]:
            pixels, cin, cout = x.numel() // x.shape[-1], x.shape[-1], wt.shape[0]
            dwt = wgrad(x, dy, workspace=_workspace(x.device, workspace_bytes(pixels, cin, cout)))
        return dx, dwt


class _Linear1x1(_Linear):
    entries = ('linear_forward', 'linear_dgrad', 'linear_wgrad', 'linear_wgrad_workspace_bytes')


class _LinearWide(_Linear):
    entries = ('linear_wide_forward', 'linear_wide_dgrad', 'linear_wide_wgrad', 'linear_wide_wgrad_workspace_bytes')


class _Depthwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.padding = stride, padding
        return rt.depthwise_forward(x, w, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _f32(dy)
        k = 3 if w.shape[0] == 9 else 5
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = rt.depthwise_dgrad(dy, w, x.shape[1:3], ctx.stride, ctx.padding)
        if ctx.needs_input_grad[1]:
            b, oh, ow, c = dy.shape
            dw = rt.depthwise_wgrad(x, dy, k, ctx.stride, ctx.padding,
                                    workspace=_workspace(x.device, rt.depthwise_wgrad_workspace_bytes(b, oh, ow, c, k)))
        return dx, dw, None, None


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.padding = stride, padding
        return rt.conv3x3_forward(x, w, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _f32(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = rt.conv3x3_dgrad(dy, w, x.shape[1:3], ctx.stride, ctx.padding)
        if ctx.needs_input_grad[1]:
            b, oh, ow, cout = dy.shape
            dw = rt.conv3x3_wgrad(x, dy, ctx.stride, ctx.padding,
                                  workspace=_workspace(x.device, rt.conv3x3_wgrad_workspace_bytes(b, oh, ow, x.shape[3], cout)))
        return dx, dw, None, None


class _FrozenBnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, scale, shift, act):
        ctx.act = act
        if rt._bn_act_id(act) == 0:      # the derivative of the affine alone does not read u
            ctx.save_for_backward(scale)
            return rt.bn_act_forward(z, scale, shift, act)
        a, u = rt.bn_act_forward(z, scale, shift, act, keep_u=True)
        ctx.save_for_backward(scale, u)
        return a

    @staticmethod
    def backward(ctx, da):
        saved = ctx.saved_tensors
        dz = None
        if ctx.needs_input_grad[0]:
            dz = rt.bn_act_backward(_f32(da), saved[1] if len(saved) > 1 else None, saved[0], ctx.act)
        return dz, None, None, None


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gamma, beta, moving_mean, moving_var, momentum, eps, act):
        pixels, c = z.numel() // z.shape[-1], z.shape[-1]
        a, mean, invstd = rt.bn_train_forward(z, gamma, beta, eps, momentum, act, moving_mean, moving_var,
                                              workspace=_workspace(z.device, rt.bn_train_workspace_bytes(pixels, c)))
        ctx.act = act
        ctx.save_for_backward(z, gamma, beta, mean, invstd)
        return a

    @staticmethod
    def backward(ctx, da):
        z, gamma, beta, mean, invstd = ctx.saved_tensors
        if not any(ctx.needs_input_grad[:3]):
            return (None,) * 8
        pixels, c = z.numel() // z.shape[-1], z.shape[-1]
        dz, dgamma, dbeta = rt.bn_train_backward(_f32(da), z, gamma, beta, mean, invstd, ctx.act, need_dz=ctx.needs_input_grad[0],
                                                 workspace=_workspace(z.device, rt.bn_train_workspace_bytes(pixels, c)))
        return (dz, dgamma if ctx.needs_input_grad[1] else None, dbeta if ctx.needs_input_grad[2] else None, None, None, None, None, None)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        ctx.save_for_backward(x)
        return rt.maxpool_forward(x, k)

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        return (rt.maxpool_backward(_f32(dy), x, ctx.k) if ctx.needs_input_grad[0] else None), None


class _UpSample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):      # (nothing saved: the gradient reads dy alone)
        return rt.upsample2_forward(x)

    @staticmethod
    def backward(ctx, dy):
        return rt.upsample2_backward(_f32(dy)) if ctx.needs_input_grad[0] else None


class _WeightedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, x0, x1, x2, x3):
        xs = (x0, x1, x2, x3)
        ctx.alpha_grad = alpha.requires_grad
        ctx.save_for_backward(alpha, *(xs if ctx.alpha_grad else ()))      # d x_i reads alpha and dy only
        return rt.wsum_forward(xs, alpha)

    @staticmethod
    def backward(ctx, dy):
        alpha, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        need, need_alpha = tuple(ctx.needs_input_grad[1:]), ctx.needs_input_grad[0]
        if not (need_alpha or any(need)):
            return (None,) * 5
        dy = _f32(dy)
        ws = None
        if need_alpha:
            ws = _workspace(dy.device, rt.wsum_workspace_bytes(dy.numel() // dy.shape[-1], dy.shape[-1]))
        dxs, dalpha = rt.wsum_backward(dy, xs if need_alpha else None, alpha, need=need, need_alpha=need_alpha, workspace=ws)
        return (dalpha,) + tuple(dxs)


class _SqueezeExcite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        b, h, w, c = x.shape
        y, m, z1, g = rt.se_forward(x, w1, b1, w2, b2, workspace=_workspace(x.device, rt.se_workspace_bytes(b, h * w, c, w1.shape[1])))
        ctx.save_for_backward(x, w1, w2, m, z1, g)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, m, z1, g = ctx.saved_tensors
        need_dx, need_params = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:])
        if not (need_dx or need_params):
            return (None,) * 5
        b, h, w, c = x.shape
        dx, dw1, db1, dw2, db2 = rt.se_backward(_f32(dy), x, w1, w2, m, z1, g, need_dx=need_dx, need_params=need_params,
                                                workspace=_workspace(x.device, rt.se_workspace_bytes(b, h * w, c, w1.shape[1])))
        return (dx,) + tuple(gr if need else None for gr, need in zip((dw1, db1, dw2, db2), ctx.needs_input_grad[1:]))


class _Concat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *xs):
        ctx.widths = [x.shape[-1] for x in xs]
        out = torch.empty(tuple(xs[0].shape[:-1]) + (sum(ctx.widths),), dtype=torch.float32, device=xs[0].device)
        at = 0
        for x, c in zip(xs, ctx.widths):
            out.narrow(-1, at, c).copy_(x)
            at += c
        return out

    @staticmethod
    def backward(ctx, dy):
        grads, at = [], 0
        for need, c in zip(ctx.needs_input_grad, ctx.widths):
            grads.append(dy.narrow(-1, at, c) if need else None)      # views: the consumers make them contiguous
            at += c
        return tuple(grads)


def linear1x1(x, wt):
    """A bias-free 1x1 convolution, differentiable in x (``runtime.linear_dgrad``) and wt (``runtime.linear_wgrad``: pad columns +0)."""
    return _Linear1x1.apply(x.contiguous(), wt.contiguous())


def conv1x1(x, wt):
    """A bias-free 1x1 convolution of any width up to 1024 channels on either side, differentiable in x and wt.  Where cin and cout are
    both at most 256 it IS ``linear1x1``: the same entries and the same bytes.  Otherwise the three wide entries
    (``runtime.linear_wide_forward`` / ``_dgrad`` / ``_wgrad``: pad columns of the weight gradient +0)."""
    if x.shape[-1] <= 256 and wt.shape[0] <= 256:
        return linear1x1(x, wt)
    return _LinearWide.apply(x.contiguous(), wt.contiguous())


def depthwise(x, w, stride=1, padding='same'):
    """A k x k depthwise convolution, differentiable in x and w.  padding: 'same' (the Keras rule) or (top, left, bottom, right)."""
    padding = padding if isinstance(padding, str) else tuple(int(v) for v in padding)
    return _Depthwise.apply(x.contiguous(), w.contiguous(), int(stride), padding)


def conv3x3(x, w, stride=1, padding='same'):
    """The dense 3 x 3 convolution every backbone starts with (MobileNetV2's Conv1, EfficientNet's stem_conv; csrc/stemgrad.hip), differentiable
    in x - the image: what an adversarial loss needs - and in w.  x [B, H, W, cin], w [9 * cin, cout] (the Keras kernel [3, 3, cin, cout]
    reshaped), cin in 1..4, cout in 1..64.  padding: 'same' (the Keras rule) or (top, left, bottom, right)."""
    padding = padding if isinstance(padding, str) else tuple(int(v) for v in padding)
    return _Conv3x3.apply(x.contiguous(), w.contiguous(), int(stride), padding)


def frozen_bn_act(z, scale, shift, act=None):
    """Inference-mode BatchNorm (per-channel scale and shift) + activation, differentiable in z only."""
    if scale.requires_grad or shift.requires_grad:
        raise ValueError('frozen_bn_act: scale and shift are frozen here (BatchNorm in training mode is batchnorm_act)')
    return _FrozenBnAct.apply(z.contiguous(), scale, shift, act)


def batchnorm_act(z, gamma, beta, moving_mean=None, moving_var=None, momentum=0.9, eps=1e-3, act=None):
    """BatchNorm in training mode + activation (Keras' BatchNormalization called with training=True, then ``act``): z [..., C] is
    normalised with the mean and the biased variance of the batch, differentiable in z, gamma and beta.  moving_mean / moving_var
    (both or neither; they must not require a gradient) are updated IN PLACE during the forward:
    moving -= (moving - batch value) * (1 - momentum), the variance the unbiased one, as Keras' fused path stores it."""
    for t in (moving_mean, moving_var):
        if t is not None and t.requires_grad:
            raise ValueError('batchnorm_act: the moving statistics are updated in place and take no gradient')
    return _BatchNormAct.apply(z.contiguous(), gamma, beta, moving_mean, moving_var, float(momentum), float(eps), act)


def fold_batchnorm(gamma, beta, moving_mean, moving_var, eps=1e-3):
    """-> (scale, shift), float32 tensors on gamma's device for ``frozen_bn_act``: the inference-mode form of a trained layer,
    scale = gamma / sqrt(moving_var + eps), shift = beta - moving_mean * scale, computed on the host in float64 as the plan compiler
    folds a BatchNormalization.  Copies the four vectors to the host: it SYNCHRONISES with the device."""
    g, b, m, v = (t.detach().to('cpu', torch.float64) for t in (gamma, beta, moving_mean, moving_var))
    scale = g / torch.sqrt(v + float(eps))
    shift = b - m * scale
    return scale.to(torch.float32).to(gamma.device), shift.to(torch.float32).to(gamma.device)


def maxpool(x, k=2):
    """Keras MaxPooling2D((k, k)), k in {2, 4}: x [B, H, W, C] -> [B, H // k, W // k, C], differentiable in x (``runtime.maxpool_backward``:
    the gradient goes to the first maximum of each window)."""
    return _MaxPool.apply(x.contiguous(), int(k))


def upsample2(x):
    """Keras UpSampling2D(): x [B, H, W, C] -> [B, 2H, 2W, C], nearest neighbour, differentiable in x."""
    return _UpSample2.apply(x.contiguous())


def weighted_sum(xs, alpha):
    """The reference's WeightedSum (model.py:117-137): xs four maps of one shape, alpha float32 [4] -> sum_i alpha[i] xs[i], differentiable
    in every map and in alpha (the maps are saved only when alpha requires a gradient: d xs[i] = alpha[i] dy does not read them)."""
    if len(xs) != 4:
        raise ValueError('weighted_sum: exactly four maps, as the reference\'s layer (%d given)' % len(xs))
    return _WeightedSum.apply(alpha, *(x.contiguous() for x in xs))


def concat(xs):
    """Keras Concatenate() over the channels: one allocation and one strided copy per source; backward hands each source that requires
    a gradient its slice of dy as a view."""
    xs = list(xs)
    for x in xs:
        if x.dtype != torch.float32 or x.shape[:-1] != xs[0].shape[:-1] or x.device != xs[0].device:
            raise ValueError('concat: float32 tensors of one shape but for the channels, on one device')
    return _Concat.apply(*xs)


def squeeze_excite(x, w1, b1, w2, b2):
    """The squeeze-excite block (efficientnet.py:406-438): x [B, H, W, C]; w1 [C, R] and b1 [R], the Keras <name>_se_reduce kernel
    [1, 1, C, R] reshaped and its bias; w2 [R, C] and b2 [C], <name>_se_expand -> x * g, g = sigmoid(swish(mean_hw(x) w1 + b1) w2 + b2),
    differentiable in all five (``runtime.se_backward``).  Only x, w1, w2 and the three small tensors of the forward (the mean, the
    reduced pre-activation and the gate) are saved; when no parameter requires a gradient the batch sums are skipped, when x does not,
    the pass over the map that writes its gradient."""
    return _SqueezeExcite.apply(x.contiguous(), w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous())


# ----------------------------------------------------------------------------- parameters: the layouts, each way, and BatchNorm in a module
_BN_LEAVES = (('gamma', True), ('beta', True), ('moving_mean', False), ('moving_variance', False))      # (leaf, trained)


def _param(a, device, grad=True):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device).requires_grad_(grad)


def _pack_wt(kernel):
    """Keras [1, 1, cin, cout] -> wt [cout, round_up(cin, 4)], pad columns 0"""
    k = np.asarray(kernel, np.float32)
    cin, cout = k.shape[-2], k.shape[-1]
    wt = np.zeros((cout, (cin + 3) // 4 * 4), np.float32)
    wt[:, :cin] = k.reshape(cin, cout).T
    return wt


def _unpack_wt(wt, cin):
    """wt [cout, round_up(cin, 4)] (host) -> Keras [1, 1, cin, cout]"""
    return np.ascontiguousarray(wt[:, :cin].T).reshape(1, 1, cin, wt.shape[0])


def _pack_dw(kernel):
    """Keras [k, k, C, 1] -> [k * k, C]"""
    dw = np.asarray(kernel, np.float32)
    return dw.reshape(dw.shape[0] * dw.shape[1], -1)


def _unpack_dw(w):
    """[k * k, C] (host) -> [k, k, C], as the model holds a depthwise kernel"""
    k = int(round(w.shape[0] ** .5))
    return w.reshape(k, k, w.shape[1]).copy()


def _bn_parameters(host, name, device):
    """The four vectors of the Keras BatchNormalization ``name`` -> {leaf: tensor}, in ``_BN_LEAVES``' order"""
    return {leaf: _param(np.asarray(host['%s/%s' % (name, leaf)], np.float32).reshape(-1), device, grad) for leaf, grad in _BN_LEAVES}


def _bn_act(z, stats, momentum, eps, act, training):
    """BatchNorm + activation in a module; stats: its four tensors in ``_BN_LEAVES``' order.  training: on the statistics of the batch,
    the moving ones updated in place (``batchnorm_act``); otherwise folded (``fold_batchnorm`` + ``frozen_bn_act``)."""
    if training:
        return batchnorm_act(z, *stats, momentum=momentum, eps=eps, act=act)
    return frozen_bn_act(z, *fold_batchnorm(*stats, eps=eps), act=act)


def _host_arrays(flat):
    """[(key, tensor)] -> {key: float32 ndarray}: one copy to the host, of all tensors flattened into one"""
    host = torch.cat([t.detach().reshape(-1).to(torch.float32) for _, t in flat]).cpu().numpy()
    arrays, at = {}, 0
    for key, t in flat:
        arrays[key] = host[at:at + t.numel()].reshape(tuple(t.shape))
        at += t.numel()
    return arrays


def _keras_weights(flat, cin):
    """[(Keras layer name [+ '/' + leaf], tensor in the operators' layout)] -> {Keras name/leaf: float32 ndarray as ``model.get_weights()``
    holds it}; cin: {name of every 1x1 convolution: its input channels} (the packed layout rounds them up to 4)."""
    out = {}
    for key, a in _host_arrays(flat).items():
        if key in cin:                                            # a 1x1 kernel
            out[key + '/kernel'] = _unpack_wt(a, cin[key])
        elif key == 'Conv1':                                      # [9 * cin, cout] -> [3, 3, cin, cout]
            out[key + '/kernel'] = a.reshape(3, 3, a.shape[0] // 9, a.shape[1]).copy()
        elif key.endswith(('_dw', 'depthwise')):                  # a depthwise kernel of the neck or of the backbone
            out[key + '/depthwise_kernel'] = _unpack_dw(a)
        elif key.endswith(('_se_reduce', '_se_expand')):          # [cin, cout] -> [1, 1, cin, cout]
            out[key + '/kernel'] = a.reshape(1, 1, a.shape[0], a.shape[1]).copy()
        else:                                                     # a bias, alpha, or a BatchNorm's vector: the name is the Keras name
            out[key] = a.copy()
    return out


RFCR_BN_MOMENTUM, RFCR_BN_EPS = 0.99, 1e-3      # tf.keras.layers.BatchNormalization() as model.py:24,29 calls it: the Keras defaults
RFCR_CONVS = ('rfcr_b1c', 'rfcr_b2c', 'rfcr_b3c', 'rfcr_b4c')
RFCR_BNS = ('rfcr_sep_dw_BN', 'rfcr_sep_pw_BN')


def rfcr_parameters(model, device):
    """The parameters of ``model``'s RFCR module (``yolov3_body``'s layer names) as float32 tensors on ``device``, in the layouts the
    operators take -> {name: tensor}:
        'rfcr_b1c' .. 'rfcr_b4c', 'rfcr_sep_pw'   Keras [1, 1, cin, cout] -> wt [cout, round_up(cin, 4)], pad columns 0
        'rfcr_wsum/alpha'                         [4]
        'rfcr_sep_dw'                             Keras [5, 5, C, 1] -> [25, C]
        '<bn>/gamma', '<bn>/beta', '<bn>/moving_mean', '<bn>/moving_variance' for <bn> in 'rfcr_sep_dw_BN', 'rfcr_sep_pw_BN'
    ``requires_grad`` is set on everything the reference trains (train.py:150-171 trains all that lies behind the backbone); the moving
    statistics take no gradient: ``rfcr_module(training=True)`` updates them in place."""
    host = model.get_weights()
    if host is None:
        raise ValueError('rfcr_parameters: the model has no weights (set_weights / load_weights)')
    out = {name: _param(_pack_wt(host[name + '/kernel']), device) for name in RFCR_CONVS + ('rfcr_sep_pw',)}
    out['rfcr_wsum/alpha'] = _param(np.asarray(host['rfcr_wsum/alpha'], np.float32).reshape(4), device)
    out['rfcr_sep_dw'] = _param(_pack_dw(host['rfcr_sep_dw/depthwise_kernel']), device)
    for bn in RFCR_BNS:
        for leaf, t in _bn_parameters(host, bn, device).items():
            out['%s/%s' % (bn, leaf)] = t
    return out


def rfcr_module(b1, b2, b3, b4, params, training=True):
    """The RFCR module (model.py:146-168) on the backbone's taps b1 [B, G, G, .], b2 [B, 2G, 2G, .], b3 [B, 4G, 4G, .] and b4, the
    already 4x-pooled fourth tap [B, 2G, 2G, .] as ``yolov3_body`` passes it; params: ``rfcr_parameters``' dictionary ->
    (b1, b2, b3) with the fused map's 96 channels concatenated behind each tap.  training: the two BatchNorms of the separable
    convolution run on the statistics of the batch and update their moving statistics in place (``batchnorm_act``); otherwise they
    are folded (``fold_batchnorm`` + ``frozen_bn_act``: no gradient for gamma and beta, one host synchronisation per BatchNorm)."""
    p = params
    b1c, b2c, b3c, b4c = (linear1x1(t, p[name]) for t, name in zip((b1, b2, b3, b4), RFCR_CONVS))
    bc = weighted_sum([upsample2(b1c), b2c, maxpool(b3c, 2), b4c], p['rfcr_wsum/alpha'])

    def bn_relu6(z, bn):
        return _bn_act(z, [p['%s/%s' % (bn, leaf)] for leaf, _ in _BN_LEAVES], RFCR_BN_MOMENTUM, RFCR_BN_EPS, 'relu6', training)
    bc = bn_relu6(depthwise(bc, p['rfcr_sep_dw'], 1, 'same'), RFCR_BNS[0])
    bc = bn_relu6(linear1x1(bc, p['rfcr_sep_pw']), RFCR_BNS[1])
    return concat([b1, maxpool(bc, 2)]), concat([b2, bc]), concat([b3, upsample2(bc)])


HEAD_BLOCKS = ('td1', 'td2', 'td3', 'bu3', 'bu2', 'bu1')
HEAD_BN_MOMENTUM, HEAD_BN_EPS = 0.99, 1e-3      # efficientnet.py's get_model_params defaults (batch_norm_momentum, batch_norm_epsilon)
HEAD_CONVS = ('_conv', '_mb_project', '_y')
HEAD_BNS = ('_conv_BN', '_mb_dw_BN', '_mb_project_BN')


def head_block_parameters(model, name, device):
    """The parameters of ``model``'s head block ``name`` (one of 'td1', 'td2', 'td3', 'bu3', 'bu2', 'bu1': ``yolov3_body``'s
    make_last_layers_efficientnet_lite, model.py:91-115) as float32 tensors on ``device``, in the layouts the operators take ->
    {key: tensor}, the keys without the block's name:
        '_conv', '_mb_project', '_y'      Keras [1, 1, cin, cout] -> wt [cout, round_up(cin, 4)], pad columns 0
        '_mb_dw'                          Keras [3, 3, F, 1] -> [9, F]
        '_mb_se_reduce', '_mb_se_expand'  Keras [1, 1, F, R] -> [F, R] and [1, 1, R, F] -> [R, F]; '<se>/bias' [R] and [F]
        '<bn>/gamma', '<bn>/beta', '<bn>/moving_mean', '<bn>/moving_variance' for <bn> in '_conv_BN', '_mb_dw_BN', '_mb_project_BN'
    and 'name', the block's name (a string).  The top-down blocks 'td1' .. 'td3' have no '_y': with the PANet pass ``yolov3_body``
    discards their y convolutions (model.py:240-241) and the model holds no such layer.  ``requires_grad`` is set on everything the reference trains (train.py:150-171 trains
    all that lies behind the backbone); the moving statistics take no gradient: ``head_block(training=True)`` updates them in place."""
    if name not in HEAD_BLOCKS:
        raise ValueError('head_block_parameters: name must be one of %s, not %r' % (', '.join(HEAD_BLOCKS), name))
    host = model.get_weights()
    if host is None:
        raise ValueError('head_block_parameters: the model has no weights (set_weights / load_weights)')
    out = {'name': name}
    for conv in HEAD_CONVS:
        if conv == '_y' and name + '_y/kernel' not in host:      # a top-down block: yolov3_body discards its y (model.py:240-241)
            continue
        out[conv] = _param(_pack_wt(host[name + conv + '/kernel']), device)
    out['_mb_dw'] = _param(_pack_dw(host[name + '_mb_dw/depthwise_kernel']), device)
    for se in ('_mb_se_reduce', '_mb_se_expand'):
        k = np.asarray(host[name + se + '/kernel'], np.float32)
        out[se] = _param(k.reshape(k.shape[-2], k.shape[-1]), device)
        out[se + '/bias'] = _param(np.asarray(host[name + se + '/bias'], np.float32).reshape(-1), device)
    for bn in HEAD_BNS:
        for leaf, t in _bn_parameters(host, name + bn, device).items():
            out['%s/%s' % (bn, leaf)] = t
    return out


def head_block(x, params, training=True, wide=False):
    """A head block (model.py:91-115, make_last_layers_efficientnet_lite) on x [B, H, W, cin]; params: ``head_block_parameters``'
    dictionary -> (x_out, y): the 1x1 convolution to F channels + BatchNorm + ReLU6; the MBConv with expand ratio 1 - depthwise 3 x 3
    + BatchNorm + Swish, ``squeeze_excite``, the 1x1 projection to O channels + BatchNorm, no residual because F != O -; and
    y = the 1x1 convolution '_y' of x_out (None for a top-down block, whose parameters hold no '_y').  training: the three BatchNorms run on the statistics of the batch and update their moving
    statistics in place (``batchnorm_act``, momentum 0.99, eps 1e-3); otherwise they are folded (``fold_batchnorm`` +
    ``frozen_bn_act``: no gradient for gamma and beta, one host synchronisation per BatchNorm).
    wide=False: the 1x1 convolutions are ``linear1x1``, which takes cin, cout <= 256, so 'bu3' (its input is td3's output, F = 128)
    runs for every model and 'td3' where its concatenated input is at most 256 wide (MobileNetV2 x0.75: 128 + 24 + 96 = 248); the wider
    blocks raise ``linear_forward``'s own error.  wide=True: they are ``conv1x1`` (up to 1024 channels on either side): every block of
    every model runs, the narrow ones on the same entries and with the same bytes as before."""
    p = params
    lin = conv1x1 if wide else linear1x1

    def bn_act(z, bn, act):
        return _bn_act(z, [p['%s/%s' % (bn, leaf)] for leaf, _ in _BN_LEAVES], HEAD_BN_MOMENTUM, HEAD_BN_EPS, act, training)
    t = bn_act(lin(x, p['_conv']), '_conv_BN', 'relu6')
    t = bn_act(depthwise(t, p['_mb_dw'], 1, 'same'), '_mb_dw_BN', 'swish')
    t = squeeze_excite(t, p['_mb_se_reduce'], p['_mb_se_reduce/bias'], p['_mb_se_expand'], p['_mb_se_expand/bias'])
    x_out = bn_act(lin(t, p['_mb_project']), '_mb_project_BN', None)
    return x_out, (lin(x_out, p['_y']) if '_y' in p else None)


LINK_CONVS = ('block_20', 'block_24', 'bu3_down', 'bu2_down')
LINK_BN_MOMENTUM, LINK_BN_EPS = 0.9, 1e-3      # model.py:248-250: BatchNormalization(momentum=0.9), the Keras epsilon


def neck_parameters(model, device):
    """Everything ``yolov3_body`` holds behind the backbone as float32 tensors on ``device``, in the layouts the operators take ->
        'rfcr'                       ``rfcr_parameters(model, device)``
        'td1', 'td2', 'td3', 'bu3', 'bu2', 'bu1'   ``head_block_parameters(model, name, device)``
        'block_20', 'block_24', 'bu3_down', 'bu2_down'   the link convolutions (model.py:248-250, 283-323): {'_conv': wt [cout,
                                     round_up(cin, 4)], '_BN/gamma', '_BN/beta', '_BN/moving_mean', '_BN/moving_variance'}
        'cin'                        {Keras name of every 1x1 convolution: its input channels} (integers, for ``neck_weights``)
    ``requires_grad`` is set on everything the reference trains (train.py:150-171); the moving statistics take no gradient:
    ``detector_neck(training=True)`` updates them in place."""
    host = model.get_weights()
    if host is None:
        raise ValueError('neck_parameters: the model has no weights (set_weights / load_weights)')
    out = {'rfcr': rfcr_parameters(model, device)}
    for name in HEAD_BLOCKS:
        out[name] = head_block_parameters(model, name, device)
    convs = list(RFCR_CONVS) + ['rfcr_sep_pw'] + [name + c for name in HEAD_BLOCKS for c in HEAD_CONVS if name + c + '/kernel' in host]
    convs += [name + '_conv' for name in LINK_CONVS]
    out['cin'] = {c: int(np.shape(host[c + '/kernel'])[-2]) for c in convs}      # the layout rounds a row up to 4: neck_weights needs these
    for name in LINK_CONVS:
        out[name] = {'_conv': _param(_pack_wt(host[name + '_conv/kernel']), device)}
        for leaf, t in _bn_parameters(host, name + '_BN', device).items():
            out[name]['_BN/' + leaf] = t
    return out


def detector_neck(b1, b2, b3, b4, params, training=True, num_anchors=3):
    """Everything ``yolov3_body`` runs behind the backbone (model.py:226-340) on the backbone's taps b1 [B, G, G, .], b2 [B, 2G, 2G, .],
    b3 [B, 4G, 4G, .] and b4, the already 4x-pooled fourth tap, as ``rfcr_module`` takes them; params: ``neck_parameters``' dictionary
    -> [y1, y2, y3], the logits [B, G, G, num_anchors, O / num_anchors] of strides 32, 16 and 8.  The order: ``rfcr_module``; the
    top-down pass td1 -> block_20 -> up-sample + concat -> td2 -> block_24 -> up-sample + concat -> td3 (their y convolutions do not
    exist: model.py:240-241); the bottom-up pass bu3 -> bu3_down -> max-pool + concat -> bu2 -> bu2_down -> max-pool + concat -> bu1.
    training: every BatchNorm runs on the statistics of the batch and updates its moving statistics in place (momentum 0.9 in the four
    link convolutions, model.py:248-250; 0.99 in the head blocks and the RFCR module); otherwise they are folded (no gradient for gamma
    and beta).  Differentiable in the taps and in every parameter that requires a gradient."""
    p = params

    def link(x, name):
        q = p[name]
        return _bn_act(conv1x1(x, q['_conv']), [q['_BN/' + leaf] for leaf, _ in _BN_LEAVES], LINK_BN_MOMENTUM, LINK_BN_EPS, 'relu6', training)

    def head(x, name):
        return head_block(x, p[name], training, wide=True)
    b1, b2, b3 = rfcr_module(b1, b2, b3, b4, p['rfcr'], training)
    c1, _ = head(b1, 'td1')
    c2, _ = head(concat([upsample2(link(c1, 'block_20')), b2]), 'td2')
    c3, _ = head(concat([upsample2(link(c2, 'block_24')), b3]), 'td3')
    x, y3 = head(c3, 'bu3')
    x, y2 = head(concat([maxpool(link(x, 'bu3_down'), 2), c2]), 'bu2')
    x, y1 = head(concat([maxpool(link(x, 'bu2_down'), 2), c1]), 'bu1')
    return [y.reshape(y.shape[0], y.shape[1], y.shape[2], num_anchors, y.shape[3] // num_anchors) for y in (y1, y2, y3)]


def neck_weights(params):
    """The inverse of ``neck_parameters`` -> {Keras layer name/leaf: float32 ndarray in the layout ``model.get_weights()`` holds it in}, so that
    ``w = model.get_weights(); w.update(neck_weights(params)); model.set_weights(w)`` ships what was trained.  (The channels a packed
    1x1 weight's rows take are ``params['cin']``, which ``neck_parameters`` records: the layout itself rounds them up to 4.)  One copy
    to the host, of all tensors flattened into one: it SYNCHRONISES with the device."""
    flat = list(params['rfcr'].items())      # (Keras layer name + leaf in the operators' naming, tensor)
    for name in HEAD_BLOCKS + LINK_CONVS:
        flat.extend((name + k, v) for k, v in params[name].items() if isinstance(v, torch.Tensor))
    return _keras_weights(flat, params['cin'])


# ----------------------------------------------------------------------------- the MobileNetV2 backbone and the whole detector
MBV2_BN_MOMENTUM, MBV2_BN_EPS = 0.9, 1e-3      # code/yolo3/model.py:180,193 through override.py:207-227 (momentum 0.9); the Keras epsilon of MobileNetV2
MBV2_STRIDES = (1, 2, 1, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1, 2, 1, 1)      # blocks 0..15 of keras.applications.MobileNetV2 (oracle/model.py:59-88)
MBV2_TAPS = (15, 12, 5, 2)                      # block_15_add, block_12_add, block_5_add, block_2_add (model.py:186-190); the last is max-pooled by 4


def _mbv2_prefix(block):
    return 'expanded_conv_' if block == 0 else 'block_%d_' % block


def mobilenetv2_parameters(model, device):
    """The parameters of ``model``'s MobileNetV2 backbone up to block 15 as float32 tensors on ``device``, in the layouts the operators
    take, keyed by the Keras layer name -> {name: tensor}:
        'Conv1'                                   Keras [3, 3, 3, F] -> [27, F] (``conv3x3``)
        '<p>expand', '<p>project'                 Keras [1, 1, cin, cout] -> wt [cout, round_up(cin, 4)], pad columns 0 (``conv1x1``); <p> is
                                                  'expanded_conv_' (block 0, which has no expand convolution) or 'block_<n>_'
        '<p>depthwise'                            Keras [3, 3, C, 1] -> [9, C]
        '<bn>/gamma', '<bn>/beta', '<bn>/moving_mean', '<bn>/moving_variance' for <bn> in 'bn_Conv1', '<p>expand_BN', '<p>depthwise_BN', '<p>project_BN'
        'cin'                                     {Keras name of every 1x1 convolution: its input channels} (integers, for ``backbone_weights``)
    ``requires_grad`` is set on every kernel, gamma and beta - the reference trains every layer (code/train.py:150-216) -; the moving
    statistics take no gradient: ``mobilenetv2_backbone(training=True)`` updates them in place."""
    host = model.get_weights()
    if host is None:
        raise ValueError('mobilenetv2_parameters: the model has no weights (set_weights / load_weights)')
    if 'Conv1/kernel' not in host:
        raise ValueError('mobilenetv2_parameters: the model has no Conv1/kernel: not a MobileNetV2 backbone (the EfficientNet backbones are not built: '
                         'their training forward draws a drop-connect mask)')

    def bn(name):
        for leaf, t in _bn_parameters(host, name, device).items():
            out['%s/%s' % (name, leaf)] = t
    k = np.asarray(host['Conv1/kernel'], np.float32)
    if k.ndim != 4 or k.shape[:2] != (3, 3) or not 1 <= k.shape[2] <= 4 or not 1 <= k.shape[3] <= 64:
        raise ValueError('mobilenetv2_parameters: Conv1/kernel has shape %s, expected [3, 3, 1..4, 1..64]' % (k.shape,))
    out = {'Conv1': _param(k.reshape(9 * k.shape[2], k.shape[3]), device), 'cin': {}}
    bn('bn_Conv1')
    for block in range(16):
        p = _mbv2_prefix(block)
        for conv in ('expand', 'project'):
            if conv == 'expand' and p + 'expand/kernel' not in host:      # block 0
                continue
            out[p + conv] = _param(_pack_wt(host[p + conv + '/kernel']), device)
            out['cin'][p + conv] = int(np.shape(host[p + conv + '/kernel'])[-2])
            bn(p + conv + '_BN')
        out[p + 'depthwise'] = _param(_pack_dw(host[p + 'depthwise/depthwise_kernel']), device)
        bn(p + 'depthwise_BN')
    return out


def _mbv2_bn_act(z, params, bn, act, training):
    return _bn_act(z, [params['%s/%s' % (bn, leaf)] for leaf, _ in _BN_LEAVES], MBV2_BN_MOMENTUM, MBV2_BN_EPS, act, training)


def mobilenetv2_stem(images, params, training=True):
    """MobileNetV2's entry on images [B, H, W, 3]: Conv1 (3 x 3, stride 2, 'same'; ``conv3x3``) -> bn_Conv1 -> ReLU6 -> [B, H / 2, W / 2, F].
    params: ``mobilenetv2_parameters``' dictionary.  training: the BatchNorm runs on the statistics of the batch and updates its moving
    statistics in place (``batchnorm_act``, momentum 0.9, eps 1e-3); otherwise it is folded (``fold_batchnorm`` + ``frozen_bn_act``)."""
    return _mbv2_bn_act(conv3x3(images, params['Conv1'], 2, 'same'), params, 'bn_Conv1', 'relu6', training)


def mobilenetv2_block(x, params, block, training=True):
    """MobileNetV2's inverted-residual block ``block`` (0..15; oracle/model.py:59-88) on x [B, H, W, cin]: [1x1 expand -> BN -> ReLU6] ->
    3 x 3 depthwise, 'same', stride ``MBV2_STRIDES[block]`` -> BN -> ReLU6 -> 1x1 project -> BN [-> + x where the stride is 1 and the
    widths agree].  Block 0 ('expanded_conv_') has no expand convolution; the widths and the expansion are those of the parameters'
    shapes.  The 1x1 convolutions are ``conv1x1`` (up to 1024 channels on either side).  training: as ``mobilenetv2_stem``."""
    if not 0 <= int(block) <= 15:
        raise ValueError('mobilenetv2_block: block must be 0..15, not %r' % (block,))
    p, stride = _mbv2_prefix(int(block)), MBV2_STRIDES[int(block)]
    t = x
    if p + 'expand' in params:
        t = _mbv2_bn_act(conv1x1(t, params[p + 'expand']), params, p + 'expand_BN', 'relu6', training)
    t = _mbv2_bn_act(depthwise(t, params[p + 'depthwise'], stride, 'same'), params, p + 'depthwise_BN', 'relu6', training)
    t = _mbv2_bn_act(conv1x1(t, params[p + 'project']), params, p + 'project_BN', None, training)
    if stride == 1 and t.shape[-1] == x.shape[-1]:
        t = t + x
    return t


def mobilenetv2_backbone(images, params, training=True):
    """images [B, H, W, 3] -> (b1, b2, b3, b4), the taps as ``detector_neck`` takes them: block_15_add [B, H / 32, W / 32, .],
    block_12_add [B, H / 16, W / 16, .], block_5_add [B, H / 8, W / 8, .] and maxpool(block_2_add, 4) [B, H / 16, W / 16, .]
    (model.py:186-190).  Differentiable in the images and in every parameter that requires a gradient."""
    x = mobilenetv2_stem(images, params, training)
    taps = {}
    for block in range(16):
        x = mobilenetv2_block(x, params, block, training)
        if block in MBV2_TAPS:
            taps[block] = x
    return taps[15], taps[12], taps[5], maxpool(taps[2], 4)


def backbone_weights(params):
    """The inverse of ``mobilenetv2_parameters`` -> {Keras layer name/leaf: float32 ndarray in the layout ``model.get_weights()`` holds it in},
    in ``neck_weights``' manner.  One copy to the host: it SYNCHRONISES with the device."""
    return _keras_weights([(k, v) for k, v in params.items() if isinstance(v, torch.Tensor)], params['cin'])


def detector_parameters(model, device):
    """-> {'backbone': ``mobilenetv2_parameters(model, device)``, 'neck': ``neck_parameters(model, device)``}: every tensor of ``yolov3_body``."""
    return {'backbone': mobilenetv2_parameters(model, device), 'neck': neck_parameters(model, device)}


def detector(images, params, training=True, num_anchors=3):
    """``yolov3_body`` on images [B, H, W, 3], differentiable end to end: ``mobilenetv2_backbone`` -> ``detector_neck`` -> [y1, y2, y3], the
    logits [B, G, G, num_anchors, .] of strides 32, 16 and 8.  params: ``detector_parameters``' dictionary."""
    return detector_neck(*mobilenetv2_backbone(images, params['backbone'], training), params['neck'], training, num_anchors)


def detector_weights(params):
    """The inverse of ``detector_parameters``: ``backbone_weights`` and ``neck_weights`` in one dictionary for ``model.set_weights``."""
    out = backbone_weights(params['backbone'])
    out.update(neck_weights(params['neck']))
    return out
