"""The backward operators of csrc/convgrad.hip and csrc/headtrain.hip behind ``torch.autograd``: a stack of bias-free 1x1
convolutions, depthwise convolutions and frozen BatchNorm + activation on top of ``yolov3_features`` trains with ``YoloLoss.call``
(itself an autograd Function) and ``runtime.adam_step``.

    linear1x1(x, wt)                        x [..., cin], wt [cout, round_up(cin, 4)] (pad columns 0) -> [..., cout]
    depthwise(x, w, stride=1, padding='same')   x [B, H, W, C], w [k * k, C] (the Keras kernel [k, k, C, 1] reshaped), k in {3, 5}
    frozen_bn_act(z, scale, shift, act)     act in {None, 'relu6', 'swish'}; scale and shift are frozen: they never get a gradient
    batchnorm_act(z, gamma, beta, moving_mean, moving_var, momentum, eps, act)   BatchNorm in training mode (csrc/bntrain.hip): batch
                                            statistics, gradients for z, gamma and beta, the moving statistics updated in place
    fold_batchnorm(gamma, beta, moving_mean, moving_var, eps) -> (scale, shift) for frozen_bn_act: how a trained layer is evaluated
    maxpool(x, k=2), upsample2(x)           Keras MaxPooling2D((k, k)), k in {2, 4}, and UpSampling2D() (csrc/fusegrad.hip)
    weighted_sum(xs, alpha)                 the reference's WeightedSum of four maps, alpha float32 [4], differentiable in all five
    concat(xs)                              Keras Concatenate() over the channels
    rfcr_module(b1, b2, b3, b4, params, training=True), rfcr_parameters(model, device)   the RFCR module (model.py:146-168) of these

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


class _Linear1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wt):
        ctx.save_for_backward(x, wt)
        return rt.linear_forward(x, wt)

    @staticmethod
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        dy = _f32(dy)
        dx = dwt = None
        if ctx.needs_input_grad[0]:
            dx = rt.linear_dgrad(dy, wt, x.shape[-1])
        if ctx.needs_input_grad[1]:
            pixels, cin, cout = x.numel() // x.shape[-1], x.shape[-1], wt.shape[0]
            dwt = rt.linear_wgrad(x, dy, workspace=_workspace(x.device, rt.linear_wgrad_workspace_bytes(pixels, cin, cout)))
        return dx, dwt


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


def depthwise(x, w, stride=1, padding='same'):
    """A k x k depthwise convolution, differentiable in x and w.  padding: 'same' (the Keras rule) or (top, left, bottom, right)."""
    padding = padding if isinstance(padding, str) else tuple(int(v) for v in padding)
    return _Depthwise.apply(x.contiguous(), w.contiguous(), int(stride), padding)


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

    def dev(a, grad=True):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device).requires_grad_(grad)
    out = {}
    for name in RFCR_CONVS + ('rfcr_sep_pw',):
        k = np.asarray(host[name + '/kernel'], np.float32)
        cin, cout = k.shape[-2], k.shape[-1]
        wt = np.zeros((cout, (cin + 3) // 4 * 4), np.float32)
        wt[:, :cin] = k.reshape(cin, cout).T
        out[name] = dev(wt)
    out['rfcr_wsum/alpha'] = dev(np.asarray(host['rfcr_wsum/alpha'], np.float32).reshape(4))
    dw = np.asarray(host['rfcr_sep_dw/depthwise_kernel'], np.float32)
    out['rfcr_sep_dw'] = dev(dw.reshape(dw.shape[0] * dw.shape[1], -1))
    for bn in RFCR_BNS:
        for p, grad in (('gamma', True), ('beta', True), ('moving_mean', False), ('moving_variance', False)):
            out['%s/%s' % (bn, p)] = dev(np.asarray(host['%s/%s' % (bn, p)], np.float32).reshape(-1), grad)
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
        stats = [p['%s/%s' % (bn, k)] for k in ('gamma', 'beta', 'moving_mean', 'moving_variance')]
        if training:
            return batchnorm_act(z, *stats, momentum=RFCR_BN_MOMENTUM, eps=RFCR_BN_EPS, act='relu6')
        return frozen_bn_act(z, *fold_batchnorm(*stats, eps=RFCR_BN_EPS), act='relu6')
    bc = bn_relu6(depthwise(bc, p['rfcr_sep_dw'], 1, 'same'), RFCR_BNS[0])
    bc = bn_relu6(linear1x1(bc, p['rfcr_sep_pw']), RFCR_BNS[1])
    return concat([b1, maxpool(bc, 2)]), concat([b2, bc]), concat([b3, upsample2(bc)])
