"""The definition of the squeeze-excite block of yoloret_amd/csrc/segrad.hip (reference yolo3/efficientnet.py:406-438), forward and
backward, written from the formulas of include/yoloret_hip.h, not from the kernels.

UNPINNED BY THE REFERENCE: the reference project has no backward code of its own (TensorFlow's GradientTape differentiates its Keras
layers), and TensorFlow is not available where this is tested.  What is stated here are TensorFlow's autodiff rules for reduce_mean,
Conv2D + bias, x sigmoid(x), sigmoid and Multiply.

Two restatements, as in tests/bntrain_ref.py and tests/fusegrad_ref.py:
* float32 with NumPy, every operation one rounding in the header's order; the sigmoid is the library's pinned one (oracle/cpost.py's
  yro_sigmoid: the same steps as yr_sigmoid).  With a ``chunk`` every sum is taken in the order csrc/segrad.hip documents - what the
  device must return bit for bit on arbitrary data, and the restatement whose deviation from float64 is E_ref in
  max |device - ref64| / max |ref64| <= 4 E_ref + 2^-24; with ``chunk=None`` every sum is taken SEQUENTIALLY in index order from +0 (the
  bias first where there is one), the plainest order a float32 chain on the CPU would use (tests/selayers_ref.host_head);
* float64 with NumPy by the same formulas (``forward64`` / ``backward64``), and, independently, ``torch.autograd`` over the obvious
  composition (``grads_torch``; this test tree only - the product never imports torch.nn.functional)."""
import numpy as np
import torch

from oracle import cpost
from tests import bntrain_ref
from tests.convgrad_ref import ints, padded, rel_err      # noqa: F401  (shared helpers: nothing mutable)

F32 = np.float32
SE_THREADS, SE_CB, SE_FC_THREADS = 256, 64, 1024          # lanes of a map-pass workgroup, channels of one at most, lanes of a small kernel


# ----------------------------------------------------------------------------- the layout of the map passes
def cb_of(c):
    """channels per block: C is cut into ceil(C / 64) blocks of equal size (the last may be smaller)"""
    nb = -(-int(c) // SE_CB)
    return -(-int(c) // nb)


def pp_of(c):
    """pixels in flight: the lanes of a workgroup that share a channel"""
    return SE_THREADS // cb_of(c)


# ----------------------------------------------------------------------------- float32 pieces
def sigmoid32(u):
    """the library's sigmoid: 1 / (1 + expf(-u)) with the pinned expf, element by element through the C oracle"""
    u = np.ascontiguousarray(u, F32)
    L = cpost.lib()
    return np.array([L.yro_sigmoid(float(v)) for v in u.ravel()], F32).reshape(u.shape)


def swish32(u):
    return u * sigmoid32(u)


def swish_grad32(u):
    """tc_swish_grad: sg * (1 + u * (1 - sg)), four operations in this order"""
    sg = sigmoid32(u)
    t1 = F32(1) - sg
    t2 = u * t1
    t3 = F32(1) + t2
    return sg * t3


def _seq(rows):
    """[n, ...] float32 -> [...]: the rows added one after the other from +0, each addition rounded to float32"""
    rows = np.ascontiguousarray(rows, F32)
    return np.cumsum(np.concatenate([np.zeros((1,) + rows.shape[1:], F32), rows]), axis=0, dtype=F32)[-1]


def pixel_sum32(t, chunk):
    """[B, N, C] float32 -> [B, C]: per image the two-stage sum in the device's order (tests/bntrain_ref.ordered_sum with the ranges of
    ``chunk`` pixels and PP = pp_of(C) lanes a channel); chunk None: sequentially over the pixels"""
    t = np.ascontiguousarray(t, F32)
    if chunk is None:
        return _seq(t.transpose(1, 0, 2))
    return np.stack([bntrain_ref.ordered_sum(img, chunk, pp_of(t.shape[2])) for img in t])


def fc32(v, w, bias, device=True):
    """`fc` of segrad.hip's header: v [B, I], w [I, O], bias [O] -> [B, O].  device: OL = min(O, 1024), KS = 1024 // OL slices of
    SL = ceil(I / KS) inputs, each added in order from +0 (a slice past I is +0), then bias + the slices in order; else bias + the
    products in order"""
    v, w, bias = (np.ascontiguousarray(a, F32) for a in (v, w, bias))
    i_n, o_n = w.shape
    prod = v[:, :, None] * w[None, :, :]          # [B, I, O], each product rounded
    assert prod.dtype == F32
    out = np.broadcast_to(bias, (v.shape[0], o_n)).astype(F32)
    if not device:
        for i in range(i_n):
            out = out + prod[:, i]
        return out
    ol = min(o_n, SE_FC_THREADS)
    ks = SE_FC_THREADS // ol
    sl = -(-i_n // ks)
    for k in range(ks):
        out = out + _seq(prod[:, k * sl:min((k + 1) * sl, i_n)].transpose(1, 0, 2))
    assert out.dtype == F32
    return out


def fct32(v, w, device=True):
    """`fct` of segrad.hip's header: v [B, I], w [O, I] -> [B, O].  device: lane l of 64 adds the products i = l, l + 64, ... in order
    from +0, the lane sums fold as halves ([0, 32) + [32, 64), then the halves of that, down to one: the butterfly seen from lane 0);
    else the products in order from +0"""
    v, w = np.ascontiguousarray(v, F32), np.ascontiguousarray(w, F32)
    o_n, i_n = w.shape
    prod = v[:, None, :] * w[None, :, :]          # [B, O, I]
    if not device:
        return _seq(prod.transpose(2, 0, 1))
    steps = -(-i_n // 64)
    rows = np.zeros((v.shape[0], o_n, steps * 64), F32)          # (padded with +0 products: a sum that starts from +0 never is -0)
    rows[:, :, :i_n] = prod
    lanes = _seq(rows.reshape(v.shape[0], o_n, steps, 64).transpose(2, 0, 1, 3))          # [B, O, 64]
    n = 64
    while n > 1:
        n //= 2
        lanes = lanes[..., :n] + lanes[..., n:2 * n]
    assert lanes.dtype == F32
    return lanes[..., 0]


def batch_sum32(terms):
    """[B, ...] -> [...]: in increasing b, the first term image 0's own"""
    terms = np.ascontiguousarray(terms, F32)
    out = terms[0].copy()
    for t in terms[1:]:
        out = out + t
    return out


# ----------------------------------------------------------------------------- float32, the operation order of the library
def forward32(x, w1, b1, w2, b2, chunk=None):
    """x [B, H, W, C] -> {y, m, z1, h, g} float32.  chunk: yr_se_chunk(B, H * W, C) for the device's order; None: order 'seq'"""
    x, w1, b1, w2, b2 = (np.ascontiguousarray(a, F32) for a in (x, w1, b1, w2, b2))
    b, hh, ww, c = x.shape
    n = hh * ww
    dev = chunk is not None
    m = pixel_sum32(x.reshape(b, n, c), chunk) / F32(n)
    z1 = fc32(m, w1, b1, dev)
    h = swish32(z1)
    g = sigmoid32(fc32(h, w2, b2, dev))
    out = {'y': x * g[:, None, None, :], 'm': m, 'z1': z1, 'h': h, 'g': g}
    assert all(v.dtype == F32 for v in out.values())
    return out


def backward32(dy, x, w1, w2, m, z1, g, chunk=None):
    """-> {dx, dw1, db1, dw2, db2, dg} float32; m, z1, g as the forward returned them"""
    dy, x, w1, w2, m, z1, g = (np.ascontiguousarray(a, F32) for a in (dy, x, w1, w2, m, z1, g))
    b, hh, ww, c = x.shape
    n = hh * ww
    dev = chunk is not None
    dg = pixel_sum32((dy * x).reshape(b, n, c), chunk)
    t = F32(1) - g
    u = g * t
    dz2 = dg * u
    h = swish32(z1)
    dh = fct32(dz2, w2, dev)
    dz1 = dh * swish_grad32(z1)
    q = fct32(dz1, w1, dev) / F32(n)
    out = {'dx': dy * g[:, None, None, :] + q[:, None, None, :], 'dg': dg,
           'db2': batch_sum32(dz2), 'dw2': batch_sum32(h[:, :, None] * dz2[:, None, :]),
           'db1': batch_sum32(dz1), 'dw1': batch_sum32(m[:, :, None] * dz1[:, None, :])}
    assert all(v.dtype == F32 for v in out.values())
    return out


# ----------------------------------------------------------------------------- float64 by the same formulas
def _sig64(u):
    return 1.0 / (1.0 + np.exp(-u))


def forward64(x, w1, b1, w2, b2):
    x, w1, b1, w2, b2 = (np.asarray(a, np.float64) for a in (x, w1, b1, w2, b2))
    m = x.mean(axis=(1, 2))
    z1 = b1 + m @ w1
    h = z1 * _sig64(z1)
    g = _sig64(b2 + h @ w2)
    return {'y': x * g[:, None, None, :], 'm': m, 'z1': z1, 'h': h, 'g': g}


def backward64(dy, x, w1, w2, m, z1, g):
    """the header's formulas in float64, from the given m, z1, g (float64 or the device's float32 ones)"""
    dy, x, w1, w2, m, z1, g = (np.asarray(a, np.float64) for a in (dy, x, w1, w2, m, z1, g))
    n = x.shape[1] * x.shape[2]
    dg = (dy * x).sum(axis=(1, 2))
    dz2 = dg * (g * (1.0 - g))
    sg = _sig64(z1)
    h = z1 * sg
    dz1 = (dz2 @ w2.T) * (sg * (1.0 + z1 * (1.0 - sg)))
    q = (dz1 @ w1.T) / n
    return {'dx': dy * g[:, None, None, :] + q[:, None, None, :], 'dg': dg, 'db2': dz2.sum(0), 'dw2': h.T @ dz2, 'db1': dz1.sum(0), 'dw1': m.T @ dz1}


# ----------------------------------------------------------------------------- torch.autograd over the obvious composition
def se_torch(x, w1, b1, w2, b2):
    """torch tensors of any float dtype: x [B, H, W, C] -> x * sigmoid(swish(mean(x) w1 + b1) w2 + b2)"""
    s = x.mean(dim=(1, 2))
    s = s @ w1 + b1
    s = s * torch.sigmoid(s)
    s = torch.sigmoid(s @ w2 + b2)
    return x * s[:, None, None, :]


def grads_torch(x, w1, b1, w2, b2, dy, dtype=torch.float64):
    """-> {y, dx, dw1, db1, dw2, db2} of sum(se(x) * dy), NumPy arrays of ``dtype``"""
    ts = [torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=True) for a in (x, w1, b1, w2, b2)]
    y = se_torch(*ts)
    gr = torch.autograd.grad(y, ts, torch.tensor(np.asarray(dy, np.float64), dtype=dtype))
    out = {'y': y.detach().numpy()}
    out.update({k: v.numpy() for k, v in zip(('dx', 'dw1', 'db1', 'dw2', 'db2'), gr)})
    return out


# ----------------------------------------------------------------------------- data
def se_case(b, hh, ww, c, r, seed=0, exact=False):
    """-> (x, dy, w1, b1, w2, b2) float32.  exact: x and dy small integers (every product and every partial sum over the pixels an
    integer below 2^24: m * N and dg are exact in any order); else normals, the kernels scaled like trained ones (1 / sqrt(fan-in))"""
    rng = np.random.default_rng(1000003 * seed + 7919 * c + 131 * r + 17 * hh + ww + 100000 * b)
    if exact:
        x, dy = ints(rng, (b, hh, ww, c)), ints(rng, (b, hh, ww, c))
    else:
        x = (rng.uniform(-.5, .5, (1, 1, 1, c)) + rng.standard_normal((b, hh, ww, c))).astype(F32)
        dy = rng.standard_normal((b, hh, ww, c)).astype(F32)
    w1 = (rng.standard_normal((c, r)) / np.sqrt(c)).astype(F32) * F32(2)
    w2 = (rng.standard_normal((r, c)) / np.sqrt(r)).astype(F32) * F32(2)
    b1, b2 = rng.uniform(-1, 1, r).astype(F32), rng.uniform(-1, 1, c).astype(F32)
    return x, dy, w1, b1, w2, b2
