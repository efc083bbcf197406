"""The definition of BatchNorm (+ activation) in training mode (yoloret_amd/csrc/bntrain.hip), written from the formulas, not from the kernels.

UNPINNED BY THE REFERENCE: TensorFlow is not available where this is tested.  What is stated here is what Keras' BatchNormalization
(fused=True, the default for a 4-D input) computes when called with training=True, and what TensorFlow's FusedBatchNormGrad returns:

* forward on rows z [P, C], N = P:  mean = sum_p z / N;  var = sum_p (z - mean)^2 / N (the biased variance, deviations about the finished
  mean);  invstd = 1 / sqrt(var + eps);  xhat = (z - mean) * invstd;  u = xhat * gamma + beta;  a = act(u);
* the moving statistics: moving -= (moving - batch value) * (1 - momentum), where the batch value of the variance is the UNBIASED one,
  var * N / max(N - 1, 1) (the fused kernel's second output is Bessel-corrected, and that is what the layer's default path stores);
* backward: g = da * act'(u) with ReLU6' = [0 < u < 6], both strict (TensorFlow's Relu6Grad; torch.clamp's own backward passes the
  gradient AT 0 and 6, so the derivative is written out), Swish' = sg (1 + u (1 - sg));  dbeta = sum_p g;  dgamma = sum_p g xhat;
  dz = ((g - dbeta / N) - xhat dgamma / N) gamma invstd.

Two restatements:
* float64 with torch on the CPU - the yardstick.  The gradients are ``torch.autograd`` over the written-out forward up to u, fed with
  g = da * act'(u) (so the batch statistics are differentiated by autograd, the activation by the rule above);
* float32 with NumPy, every operation in the order the header of the library gives, one rounding each.  Its per-channel sums run
  SEQUENTIALLY in pixel order from +0 (the last row of a float32 cumsum): the least accurate order a correct kernel could use, so its
  deviation from float64, E_ref, is an honest yardstick for any chunking (max |device - ref64| / max |ref64| <= 4 E_ref + 2^-24).  On
  data whose sums are exact in any order it is what the device must return bit for bit.
* the same float32 text with the sums in the DEVICE'S order (``ordered_sum``, the layout paragraph of bntrain.hip restated): what the
  device must return bit for bit on arbitrary data.  ``forward32`` / ``backward32`` take the summation as an argument (``sums=``), so
  nothing else is stated twice."""
import numpy as np
import torch

from tests.convgrad_ref import _act, act_prime, ints, padded, rel_err      # noqa: F401  (shared helpers: nothing mutable)

F32 = np.float32


def bessel(n):
    """(float)((double)N / (double)max(N - 1, 1))"""
    return F32(np.float64(n) / np.float64(max(n - 1, 1)))


# ----------------------------------------------------------------------------- float64
def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def _forward64(z, gamma, beta, eps):
    """torch [P, C] -> (u, xhat, mean, var, invstd), attached to the graph"""
    n = z.shape[0]
    mean = z.sum(0) / n
    var = ((z - mean) ** 2).sum(0) / n
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * invstd
    return xhat * gamma + beta, xhat, mean, var, invstd


def forward64(z, gamma, beta, eps=1e-3, act=None):
    """-> {a, u, xhat, mean, var, invstd} as float64 arrays"""
    u, xhat, mean, var, invstd = _forward64(_t(z), _t(gamma), _t(beta), float(eps))
    return {k: v.numpy() for k, v in (('a', _act(u, act)), ('u', u), ('xhat', xhat), ('mean', mean), ('var', var), ('invstd', invstd))}


def moving64(moving_mean, moving_var, mean, var, n, momentum):
    d = 1.0 - float(momentum)
    mm, mv = np.asarray(moving_mean, np.float64), np.asarray(moving_var, np.float64)
    unbiased = np.asarray(var, np.float64) * (float(n) / float(max(n - 1, 1)))
    return mm - (mm - np.asarray(mean, np.float64)) * d, mv - (mv - unbiased) * d


def backward64(da, z, gamma, beta, eps=1e-3, act=None):
    """-> (dz, dgamma, dbeta) of sum(act(batchnorm(z)) * da): autograd through the statistics, the activation's derivative written out"""
    zt, gt, bt = _t(z, True), _t(gamma, True), _t(beta, True)
    u = _forward64(zt, gt, bt, float(eps))[0]
    g = _t(da) * act_prime(u.detach(), act)
    dz, dgamma, dbeta = torch.autograd.grad(u, (zt, gt, bt), g)
    return dz.numpy(), dgamma.numpy(), dbeta.numpy()


# ----------------------------------------------------------------------------- float32, the operation order of the library
def seq_sum(x):
    """[P, C] float32 -> [C]: rows added one after the other, in order, from +0, each addition rounded to float32"""
    x = np.ascontiguousarray(x, F32)
    return np.cumsum(np.concatenate([np.zeros((1, x.shape[1]), F32), x]), axis=0, dtype=F32)[-1]


def ordered_sum(x, chunk, pp):
    """[P, C] float32 -> [C] in the order of bntrain.hip's layout paragraph: slab j is the range [j chunk, min((j + 1) chunk, P)); pixel p
    of it belongs to lane po = (p - j chunk) % pp; a lane adds its pixels in increasing p from +0; the lanes of a channel are added in the
    order po = 0 .. pp - 1 from +0; the slabs in index order from +0.  Every addition is one float32 rounding (three ``seq_sum``s: a range
    is padded with +0 rows to whole steps of pp pixels, which changes no bit - a sum that starts from +0 never is -0)."""
    x = np.ascontiguousarray(x, F32)
    p, c = x.shape
    chunk, pp = int(chunk), int(pp)
    assert p >= 1 and chunk >= 1 and pp >= 1
    chunk = min(chunk, p)          # (one range either way)
    slabs, steps = -(-p // chunk), -(-chunk // pp)
    rows = np.zeros((slabs, steps * pp, c), F32)
    full = p // chunk
    rows[:full, :chunk] = x[:full * chunk].reshape(full, chunk, c)
    if full < slabs:
        rows[full, :p - full * chunk] = x[full * chunk:]
    lanes = seq_sum(rows.reshape(slabs, steps, pp * c).transpose(1, 0, 2).reshape(steps, slabs * pp * c))           # [slabs * pp * c]
    slab = seq_sum(lanes.reshape(slabs, pp, c).transpose(1, 0, 2).reshape(pp, slabs * c))                            # [slabs * c]
    return seq_sum(slab.reshape(slabs, c))


def device_order(c, chunk):
    """-> the ``sums=`` of ``forward32`` / ``backward32`` for C = c channels and the chunk the library reports: pp = 1024 // min(C, 64)"""
    pp = 1024 // min(int(c), 64)
    return lambda x: ordered_sum(x, chunk, pp)


def _sigmoid32(u):
    return F32(1) / (F32(1) + np.exp(-u, dtype=F32))


def _act32(u, act):
    if act == 'relu6':
        return np.minimum(np.maximum(u, F32(0)), F32(6))
    if act == 'swish':
        return u * _sigmoid32(u)
    assert act in (None, 'none')
    return u


def _xhat_u32(z, mean, invstd, gamma, beta):
    xhat = (z - mean[None, :]) * invstd[None, :]
    return xhat, xhat * gamma[None, :] + beta[None, :]


def forward32(z, gamma, beta, eps=1e-3, momentum=0.9, act=None, moving_mean=None, moving_var=None, sums=seq_sum):
    """-> {a, u, xhat, mean, var, invstd[, moving_mean, moving_var]} as float32 arrays (the moving statistics are returned, not changed);
    sums: the per-channel summation [P, C] -> [C] (``seq_sum``, or ``device_order(C, chunk)`` for the device's own order)"""
    z, gamma, beta = (np.ascontiguousarray(v, F32) for v in (z, gamma, beta))
    n = z.shape[0]
    fn = F32(n)
    mean = sums(z) / fn
    d = z - mean[None, :]
    var = sums(d * d) / fn
    invstd = F32(1) / np.sqrt(var + F32(eps))
    xhat, u = _xhat_u32(z, mean, invstd, gamma, beta)
    out = {'a': _act32(u, act), 'u': u, 'xhat': xhat, 'mean': mean, 'var': var, 'invstd': invstd}
    if moving_mean is not None:
        mm, mv = np.ascontiguousarray(moving_mean, F32), np.ascontiguousarray(moving_var, F32)
        k = F32(1) - F32(momentum)
        out['moving_mean'] = mm - (mm - mean) * k
        out['moving_var'] = mv - (mv - var * bessel(n)) * k
    assert all(v.dtype == F32 for v in out.values())
    return out


def act_grad32(da, u, act):
    """g = da * act'(u)"""
    if act == 'relu6':
        return np.where((u > 0) & (u < 6), da, F32(0))
    if act == 'swish':
        sg = _sigmoid32(u)
        t1 = F32(1) - sg
        t2 = u * t1
        t3 = F32(1) + t2
        return da * (sg * t3)
    assert act in (None, 'none')
    return da


def backward32(da, z, gamma, beta, mean, invstd, act=None, sums=seq_sum):
    """-> (dz, dgamma, dbeta) as float32 arrays; mean and invstd as the forward returned them; sums as in ``forward32``"""
    da, z, gamma, beta, mean, invstd = (np.ascontiguousarray(v, F32) for v in (da, z, gamma, beta, mean, invstd))
    fn = F32(z.shape[0])
    xhat, u = _xhat_u32(z, mean, invstd, gamma, beta)
    g = act_grad32(da, u, act)
    dbeta = sums(g)
    dgamma = sums(g * xhat)
    mg, mgx = dbeta / fn, dgamma / fn
    dz = ((g - mg[None, :]) - xhat * mgx[None, :]) * (gamma * invstd)[None, :]
    assert dz.dtype == F32 and dgamma.dtype == F32 and dbeta.dtype == F32
    return dz, dgamma, dbeta


def fold64(gamma, beta, moving_mean, moving_var, eps=1e-3):
    """the inference-mode form: scale = gamma / sqrt(var + eps), shift = beta - mean * scale"""
    g, b, m, v = (np.asarray(t, np.float64) for t in (gamma, beta, moving_mean, moving_var))
    scale = g / np.sqrt(v + float(eps))
    return scale, b - m * scale
