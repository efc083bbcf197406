"""The definition of the fusing operators of yoloret_amd/csrc/fusegrad.hip - max-pooling, nearest-neighbour up-sampling, the WeightedSum of
four maps - and of the RFCR module built from them, written from the formulas, not from the kernels.

UNPINNED BY THE REFERENCE: the reference project has no backward code of its own (TensorFlow's GradientTape differentiates its Keras
layers), and TensorFlow is not available where this is tested.  What is stated here:

* MaxPooling2D((k, k)): stride k, 'valid'; the window is scanned in row-major order and a later element replaces the running maximum
  only when it is strictly greater, so the FIRST maximum wins a tie; its position receives dy, every other position of the window and
  the trailing strip (rows >= (H // k) k, columns >= (W // k) k) receive +0.  This is TensorFlow's MaxPoolGrad as restated from memory;
  torch.max_pool2d follows the same rule, which the float64 restatement below relies on.
* UpSampling2D(): y[2i + a][2j + b] = x[i][j]; dx[i][j] = ((dy[2i][2j] + dy[2i][2j + 1]) + dy[2i + 1][2j]) + dy[2i + 1][2j + 1].
* WeightedSum (model.py:117-137): y = ((a0 x0 + a1 x1) + a2 x2) + a3 x3, each product rounded; dx_i = a_i dy; dalpha_i = sum dy x_i.

Two restatements, as in tests/convgrad_ref.py and tests/bntrain_ref.py:
* float32 with NumPy, every operation in the order include/yoloret_hip.h gives, one rounding each.  d alpha's sum runs SEQUENTIALLY over
  the (pixel, channel) pairs from +0 (``seq_dot``): the least accurate order a correct kernel could use, so its deviation from float64,
  E_ref, is an honest yardstick (max |device - ref64| / max |ref64| <= 4 E_ref + 2^-24); ``ordered_dot`` is the same sum in the DEVICE'S
  order (the header of fusegrad.hip restated): what the device must return bit for bit on arbitrary data;
* float64 with torch on the CPU - the yardstick: ``torch.autograd`` over ``torch.nn.functional`` (this test tree only; the product never
  imports it), for each operator and for the whole RFCR module (model.py:146-168)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import bntrain_ref, convgrad_ref as cref
from tests.convgrad_ref import ints, padded, rel_err      # noqa: F401  (shared helpers: nothing mutable)

F32 = np.float32
WS_THREADS = 1024          # lanes of a stage-1 workgroup of the weighted sum's backward
BN_MOMENTUM, BN_EPS = 0.99, 1e-3


# ----------------------------------------------------------------------------- float32, the operation order of the library
def _windows(x, k):
    """[B, H, W, C] -> [B, OH, OW, k * k, C], the window's elements in row-major order"""
    b, h, w, c = x.shape
    oh, ow = h // k, w // k
    v = x[:, :oh * k, :ow * k].reshape(b, oh, k, ow, k, c).transpose(0, 1, 3, 2, 4, 5)
    return v.reshape(b, oh, ow, k * k, c)


def _scan(win):
    """the forward's scan over axis 3 -> (maximum, index of its first occurrence), written as the loop it is"""
    m = win[:, :, :, 0].copy()
    at = np.zeros(m.shape, np.int64)
    for i in range(1, win.shape[3]):
        later = win[:, :, :, i] > m          # strictly greater: -0 does not replace +0, nor +0 -0
        m = np.where(later, win[:, :, :, i], m)
        at = np.where(later, i, at)
    return m, at


def maxpool32(x, k):
    x = np.ascontiguousarray(x, F32)
    return _scan(_windows(x, k))[0]


def maxpool_backward32(dy, x, k):
    x, dy = np.ascontiguousarray(x, F32), np.ascontiguousarray(dy, F32)
    b, h, w, c = x.shape
    oh, ow = h // k, w // k
    _, at = _scan(_windows(x, k))
    hit = at[:, :, :, None, :] == np.arange(k * k)[None, None, None, :, None]
    dwin = np.where(hit, dy[:, :, :, None, :], F32(0)).astype(F32)          # [B, OH, OW, k * k, C]
    dx = np.zeros((b, h, w, c), F32)          # +0, the trailing strip included
    dx[:, :oh * k, :ow * k] = dwin.reshape(b, oh, ow, k, k, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, oh * k, ow * k, c)
    return dx


def upsample32(x):
    x = np.ascontiguousarray(x, F32)
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


def upsample_backward32(dy):
    dy = np.ascontiguousarray(dy, F32)
    s1 = dy[:, 0::2, 0::2] + dy[:, 0::2, 1::2]
    s2 = s1 + dy[:, 1::2, 0::2]
    out = s2 + dy[:, 1::2, 1::2]
    assert out.dtype == F32
    return out


def wsum32(xs, alpha):
    xs = [np.ascontiguousarray(x, F32) for x in xs]
    a = np.ascontiguousarray(alpha, F32)
    t = [a[i] * xs[i] for i in range(4)]
    out = ((t[0] + t[1]) + t[2]) + t[3]
    assert out.dtype == F32
    return out


def wsum_dx32(dy, alpha):
    dy, a = np.ascontiguousarray(dy, F32), np.ascontiguousarray(alpha, F32)
    return [a[i] * dy for i in range(4)]


def _seq(rows):
    """[n, m] float32 -> [m]: the rows added one after the other from +0, each addition rounded to float32"""
    rows = np.ascontiguousarray(rows, F32)
    return np.cumsum(np.concatenate([np.zeros((1, rows.shape[1]), F32), rows]), axis=0, dtype=F32)[-1]


def seq_dot(dy, x):
    """sum over all (pixel, channel) pairs of the rounded products, sequentially in memory order from +0 -> a float32 scalar"""
    prod = (np.ascontiguousarray(dy, F32) * np.ascontiguousarray(x, F32)).reshape(-1, 1)
    return _seq(prod)[0]


def ordered_dot(dy, x, chunk, threads=WS_THREADS):
    """d alpha_i in the order of fusegrad.hip's header; dy, x [P, C] float32, chunk = yr_wsum_chunk(P, C).  Range j is the pixels
    [j chunk, min((j + 1) chunk, P)); its pairs are numbered e = (p - j chunk) C + c and lane t = e % threads owns them; a lane adds its
    rounded products in increasing e from +0; a wave's 64 lane sums fold as halves: lanes [0, 32) + [32, 64), then [0, 16) + [16, 32) of
    that, down to one value (the butterfly l ^ 32, 16, .., 1 seen from lane 0; float addition is commutative, so every lane holds these
    bits); the waves are added in index order, the first term wave 0's own; the ranges in index order, the first term range 0's own.
    (A range is padded with +0 products to whole steps of ``threads`` pairs, which changes no bit: a sum that starts from +0 never
    is -0.)"""
    dy, x = np.ascontiguousarray(dy, F32), np.ascontiguousarray(x, F32)
    p, c = dy.shape
    chunk = int(chunk)
    prod = (dy * x).reshape(-1)
    slabs = []
    for p0 in range(0, p, chunk):
        e = prod[p0 * c:min(p0 + chunk, p) * c]
        steps = -(-e.size // threads)
        rows = np.zeros((steps * threads,), F32)
        rows[:e.size] = e
        v = _seq(rows.reshape(steps, threads)).reshape(threads // 64, 64)          # lane sums, [wave, lane]
        n = 64
        while n > 1:
            n //= 2
            v = v[:, :n] + v[:, n:2 * n]
        waves = v[:, 0]
        s = waves[0]
        for w in waves[1:]:
            s = F32(s + w)
        slabs.append(s)
    s = slabs[0]
    for t in slabs[1:]:
        s = F32(s + t)
    return F32(s)


# ----------------------------------------------------------------------------- float64 (or float32) with torch: autograd
def _t(a, dtype=np.float64, grad=False):
    return cref._t(a, dtype, grad)


def _maxpool(x, k):
    """torch [B, H, W, C] -> [B, H // k, W // k, C]"""
    return F.max_pool2d(x.permute(0, 3, 1, 2), k).permute(0, 2, 3, 1)


def _upsample(x):
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='nearest').permute(0, 2, 3, 1)


def _wsum(xs, alpha):
    return alpha[0] * xs[0] + alpha[1] * xs[1] + alpha[2] * xs[2] + alpha[3] * xs[3]


def maxpool_grads64(x, dy, k):
    """-> (y, dx) of sum(maxpool(x) * dy) in float64"""
    xt = _t(x, grad=True)
    y = _maxpool(xt, k)
    dx, = torch.autograd.grad(y, xt, _t(dy))
    return y.detach().numpy(), dx.numpy()


def upsample_grads64(x, dy):
    xt = _t(x, grad=True)
    y = _upsample(xt)
    dx, = torch.autograd.grad(y, xt, _t(dy))
    return y.detach().numpy(), dx.numpy()


def wsum_grads64(xs, alpha, dy):
    """-> (y, [dx_i], dalpha) in float64"""
    xt, at = [_t(x, grad=True) for x in xs], _t(alpha, grad=True)
    y = _wsum(xt, at)
    g = torch.autograd.grad(y, xt + [at], _t(dy))
    return y.detach().numpy(), [v.numpy() for v in g[:4]], g[4].numpy()


# ----------------------------------------------------------------------------- the RFCR module (model.py:146-168)
RFCR_CONVS = ('rfcr_b1c', 'rfcr_b2c', 'rfcr_b3c', 'rfcr_b4c')
RFCR_TRAINED = RFCR_CONVS + ('rfcr_wsum/alpha', 'rfcr_sep_dw', 'rfcr_sep_dw_BN/gamma', 'rfcr_sep_dw_BN/beta', 'rfcr_sep_pw', 'rfcr_sep_pw_BN/gamma',
                             'rfcr_sep_pw_BN/beta')
RFCR_MOVING = ('rfcr_sep_dw_BN/moving_mean', 'rfcr_sep_dw_BN/moving_variance', 'rfcr_sep_pw_BN/moving_mean', 'rfcr_sep_pw_BN/moving_variance')


def rfcr_ref_params(host, dtype, grad=True):
    """{name: array} in the layouts of ``autograd.rfcr_parameters`` (1x1 weights [cout, round_up(cin, 4)]; ``_lin`` takes the first cin
    columns, so the pad columns' gradient is 0) -> {name: torch tensor of ``dtype``}, the trained ones requiring a gradient"""
    return {k: torch.tensor(np.asarray(v, np.float64), dtype=cref.DT[dtype], requires_grad=grad and k in RFCR_TRAINED) for k, v in host.items()}


def _lin(x, w):
    """x [B, H, W, cin], w [cout, >= cin] torch -> [B, H, W, cout]"""
    cin = x.shape[-1]
    return cref._linear(x.reshape(-1, cin), w[:, :cin]).reshape(tuple(x.shape[:-1]) + (w.shape[0],))


def _bn_relu6(z, p, bn, record):
    """BatchNorm on the batch statistics + ReLU6 (torch.clamp: the cases keep every u away from the kinks) -> a; records (u, mean, var, N)"""
    shape = z.shape
    u, _, mean, var, _ = bntrain_ref._forward64(z.reshape(-1, shape[-1]), p[bn + '/gamma'], p[bn + '/beta'], BN_EPS)
    if record is not None:
        record[bn] = (u.detach().numpy(), mean.detach().numpy(), var.detach().numpy(), u.shape[0])
    return torch.clamp(u, 0.0, 6.0).reshape(shape)


def rfcr_module(b1, b2, b3, b4, p, record=None):
    """torch tensors (any float dtype) -> (o1, o2, o3), BatchNorm in training mode.  record: a dict that receives, detached, the two
    BatchNorms' (u, mean, var, N) under their names, and 'pool_b3c' / 'pool_bc': the inputs of the two max-poolings."""
    b1c, b2c, b3c, b4c = (_lin(t, p[n]) for t, n in zip((b1, b2, b3, b4), RFCR_CONVS))
    bc = _wsum([_upsample(b1c), b2c, _maxpool(b3c, 2), b4c], p['rfcr_wsum/alpha'])
    bc = _bn_relu6(cref._depthwise(bc, p['rfcr_sep_dw'], 5, 1, (2, 2, 2, 2)), p, 'rfcr_sep_dw_BN', record)
    bc = _bn_relu6(_lin(bc, p['rfcr_sep_pw']), p, 'rfcr_sep_pw_BN', record)
    if record is not None:
        record['pool_b3c'], record['pool_bc'] = b3c.detach().numpy(), bc.detach().numpy()
    return torch.cat([b1, _maxpool(bc, 2)], -1), torch.cat([b2, bc], -1), torch.cat([b3, _upsample(bc)], -1)


def top_two_gap(x, k=2):
    """[B, H, W, C] -> per window the gap between its two largest values, [B, OH, OW, C], and both of them"""
    win = np.sort(_windows(np.asarray(x), k), axis=3)
    return win[:, :, :, -1] - win[:, :, :, -2], win[:, :, :, -1], win[:, :, :, -2]
