"""The definition of the backward operators of yoloret_amd/csrc/convgrad.hip, written from the formulas, not from the kernels.

UNPINNED BY THE REFERENCE: the reference project has no backward code of its own (TensorFlow's GradientTape differentiates its Keras
layers), and TensorFlow is not available where this is tested.  What is stated here is what tf.nn.conv2d / depthwise_conv2d /
relu6 / swish and an inference-mode BatchNormalization differentiate to, restated with torch on the CPU:

* the convolutions: ``torch.autograd`` over ``torch.nn.functional.conv2d`` (this test tree only; the product never imports it), in
  float64 - the yardstick - or float32, whose deviation from float64 on the same inputs is E_ref of the rounding bars
  (max |device - ref64| / max |ref64| <= 4 E_ref + 2^-24, the project's margin for another summation order);
* the padding: Keras 'same' (out = ceil(n / stride), total = max((out - 1) stride + k - n, 0), the smaller half in front) and
  MobileNetV2's explicit pad in front of a stride-2 'valid' convolution (keras.applications correct_pad: front = k // 2 - (1 - n % 2),
  back = k // 2);
* frozen BatchNorm + activation: u = z scale + shift; dz = da act'(u) scale with ReLU6' = [0 < u < 6], both strict (TensorFlow's
  Relu6Grad; torch.clamp's own backward passes the gradient AT 0 and 6, so the derivative is written out, not taken from autograd),
  Swish' = sg (1 + u (1 - sg)); masked elements are +0.

Layouts are the device's: maps [B, H, W, C], taps w [k * k, C] (the Keras kernel [k, k, C, 1] reshaped), 1x1 weights w [cout, cin]."""
import numpy as np
import torch
import torch.nn.functional as F

DT = {np.float64: torch.float64, np.float32: torch.float32, 'float64': torch.float64, 'float32': torch.float32}


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=DT[dtype], requires_grad=grad)


def rel_err(got, ref64):
    ref64 = np.asarray(ref64, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref64)) / np.max(np.abs(ref64)))


def pack_wt(w):
    """[cout, cin] -> Wt [cout, round_up(cin, 4)] float32, pad columns 0."""
    w = np.asarray(w, np.float32)
    out = np.zeros((w.shape[0], (w.shape[1] + 3) // 4 * 4), np.float32)
    out[:, :w.shape[1]] = w
    return out


# ----------------------------------------------------------------------------- padding
def same_pads(n, k, stride):
    out = -(-n // stride)
    total = max((out - 1) * stride + k - n, 0)
    return total // 2, total - total // 2, out


def mobilenet_pads(n, k):
    """correct_pad of keras.applications.mobilenet_v2, then a stride-2 'valid' convolution"""
    front, back = k // 2 - (1 - n % 2), k // 2
    return front, back, (n + front + back - k) // 2 + 1


def geometry(h, w, k, stride, padding):
    """padding 'same' | 'mobilenet' | (top, left, bottom, right) -> ((top, left, bottom, right), (oh, ow))"""
    if padding == 'same':
        (pt, pb, oh), (pl, pr, ow) = same_pads(h, k, stride), same_pads(w, k, stride)
    elif padding == 'mobilenet':
        assert stride == 2
        (pt, pb, oh), (pl, pr, ow) = mobilenet_pads(h, k), mobilenet_pads(w, k)
    else:
        pt, pl, pb, pr = padding
        oh, ow = (h + pt + pb - k) // stride + 1, (w + pl + pr - k) // stride + 1
    return (pt, pl, pb, pr), (oh, ow)


# ----------------------------------------------------------------------------- the 1x1 convolution
def _linear(x, w):
    """x [P, cin], w [cout, cin] torch -> [P, cout] through conv2d"""
    p, cin = x.shape
    return F.conv2d(x.t().reshape(1, cin, p, 1), w.reshape(w.shape[0], cin, 1, 1)).reshape(w.shape[0], p).t()


def linear(x, w, dtype=np.float64):
    return _linear(_t(x, dtype), _t(w, dtype)).numpy()


def linear_grads(x, w, dy, dtype=np.float64):
    """-> (dx [P, cin], dw [cout, cin]) of sum(linear(x, w) * dy)"""
    xt, wt = _t(x, dtype, True), _t(w, dtype, True)
    dx, dw = torch.autograd.grad(_linear(xt, wt), (xt, wt), _t(dy, dtype))
    return dx.numpy(), dw.numpy()


# ----------------------------------------------------------------------------- the depthwise convolution
def _depthwise(x, w, k, stride, pads):
    """x [B, H, W, C], w [k * k, C] torch -> [B, OH, OW, C]"""
    c = x.shape[3]
    pt, pl, pb, pr = pads
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w.t().reshape(c, 1, k, k), stride=stride, groups=c).permute(0, 2, 3, 1)


def depthwise(x, w, k, stride, padding, dtype=np.float64):
    pads, _ = geometry(x.shape[1], x.shape[2], k, stride, padding)
    return _depthwise(_t(x, dtype), _t(w, dtype), k, stride, pads).numpy()


def depthwise_grads(x, w, dy, k, stride, padding, dtype=np.float64):
    """-> (dx [B, H, W, C], dw [k * k, C]) of sum(depthwise(x, w) * dy)"""
    pads, _ = geometry(x.shape[1], x.shape[2], k, stride, padding)
    xt, wt = _t(x, dtype, True), _t(w, dtype, True)
    dx, dw = torch.autograd.grad(_depthwise(xt, wt, k, stride, pads), (xt, wt), _t(dy, dtype))
    return dx.numpy(), dw.numpy()


# ----------------------------------------------------------------------------- frozen BatchNorm + activation
def _act(u, act):
    if act == 'relu6':
        return torch.clamp(u, 0.0, 6.0)
    if act == 'swish':
        return u * torch.sigmoid(u)
    assert act in (None, 'none')
    return u


def _bn_act(z, scale, shift, act):
    return _act(z * scale + shift, act)


def bn_act(z, scale, shift, act, dtype=np.float64):
    """-> (a, u)"""
    u = _t(z, dtype) * _t(scale, dtype) + _t(shift, dtype)
    return _act(u, act).numpy(), u.numpy()


def act_prime(u, act):
    """torch -> torch; the derivative written out (see the module text for ReLU6 at 0 and 6)"""
    if act == 'relu6':
        return ((u > 0) & (u < 6)).to(u.dtype)
    if act == 'swish':
        sg = torch.sigmoid(u)
        return sg * (1 + u * (1 - sg))
    assert act in (None, 'none')
    return torch.ones_like(u)


def bn_act_backward(da, u, scale, act, dtype=np.float64):
    da, u, scale = _t(da, dtype), _t(u, dtype), _t(scale, dtype)
    if act == 'relu6':
        return torch.where((u > 0) & (u < 6), da * scale, torch.zeros_like(da)).numpy()
    return ((da * act_prime(u, act)) * scale).numpy()


# ----------------------------------------------------------------------------- data
def ints(rng, shape):
    """integers in [-4, 4] as float32: products are at most 16 in magnitude, every partial sum an integer far below 2^24"""
    return rng.integers(-4, 5, shape).astype(np.float32)


def padded(a, ld):
    """[..., C] -> [..., ld] with NaN in the pad columns"""
    out = np.full(a.shape[:-1] + (ld,), np.nan, np.float32)
    out[..., :a.shape[-1]] = a
    return out
