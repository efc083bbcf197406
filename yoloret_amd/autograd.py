"""The backward operators of csrc/convgrad.hip and csrc/headtrain.hip behind ``torch.autograd``: a stack of bias-free 1x1
convolutions, depthwise convolutions and frozen BatchNorm + activation on top of ``yolov3_features`` trains with ``YoloLoss.call``
(itself an autograd Function) and ``runtime.adam_step``.

    linear1x1(x, wt)                        x [..., cin], wt [cout, round_up(cin, 4)] (pad columns 0) -> [..., cout]
    depthwise(x, w, stride=1, padding='same')   x [B, H, W, C], w [k * k, C] (the Keras kernel [k, k, C, 1] reshaped), k in {3, 5}
    frozen_bn_act(z, scale, shift, act)     act in {None, 'relu6', 'swish'}; scale and shift are frozen: they never get a gradient
    batchnorm_act(z, gamma, beta, moving_mean, moving_var, momentum, eps, act)   BatchNorm in training mode (csrc/bntrain.hip): batch
                                            statistics, gradients for z, gamma and beta, the moving statistics updated in place
    fold_batchnorm(gamma, beta, moving_mean, moving_var, eps) -> (scale, shift) for frozen_bn_act: how a trained layer is evaluated

Written the way ``_YoloLossFunction`` of yolo3/model.py is: forward and backward are calls of the C entries, only what backward needs
is saved, a gradient is computed only for an input that requires one (the others are None and their kernel is not launched).  float32
CUDA tensors only; there is no fallback.  Workspaces of the two-stage weight gradients are cached per device and size."""
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
