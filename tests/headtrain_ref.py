"""The yardsticks of the output-layer training kernels (yoloret_amd/csrc/headtrain.hip), written from the formulas, not from the kernels.

* ``wgrad64`` / ``forward64``: NumPy float64 ``dy.T @ x`` and ``x @ w.T``; ``rel_err`` is max |got - ref| / max |ref|, the unit of the
  rounding bars (4 x the same figure of NumPy's float32 product + 2^-24).
* ``adam_step``: Keras Adam's dense update (TF 2.x OptimizerV2, no amsgrad) in float32, one IEEE operation per line in the order the
  kernel documents.  TensorFlow is not available where this is tested: this restatement is the definition.
      m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) (g g);  w = w - alpha m / (sqrt(v) + eps),  alpha = f32(lr sqrt(1 - b2^t) / (1 - b1^t))
* ``cosine_lr``: tf.keras.experimental.CosineDecay(lr, epochs)(epoch) with alpha = 0."""
import math

import numpy as np

F = np.float32


def pack_wt(w):
    """[cout, cin] -> Wt [cout, round_up(cin, 4)] float32, pad columns 0."""
    w = np.asarray(w, np.float32)
    out = np.zeros((w.shape[0], (w.shape[1] + 3) // 4 * 4), np.float32)
    out[:, :w.shape[1]] = w
    return out


def wgrad64(x, dy):
    """x [P, cin], dy [P, cout] -> [cout, cin] float64."""
    return np.asarray(dy, np.float64).T @ np.asarray(x, np.float64)


def forward64(x, w):
    """x [P, cin], w [cout, cin] -> [P, cout] float64."""
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64).T


def rel_err(got, ref64):
    ref64 = np.asarray(ref64, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref64)) / np.max(np.abs(ref64)))


def adam_alpha(lr, t, beta1=.9, beta2=.999):
    return F(float(lr) * math.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t))


def adam_step(w, m, v, g, alpha, beta1=.9, beta2=.999, eps=1e-8):
    """float32 arrays -> (w, m, v) after one step; nothing is modified in place."""
    w, m, v, g = (np.asarray(a, np.float32) for a in (w, m, v, g))
    alpha, b1, b2, eps = F(alpha), F(beta1), F(beta2), F(eps)
    omb1, omb2 = F(1) - b1, F(1) - b2
    with np.errstate(under='ignore'):
        m1 = b1 * m
        m2 = omb1 * g
        mn = m1 + m2
        v1 = b2 * v
        gg = g * g
        v2 = omb2 * gg
        vn = v1 + v2
        num = alpha * mn
        den = np.sqrt(vn) + eps
        wn = w - num / den
    assert wn.dtype == np.float32 and mn.dtype == np.float32 and vn.dtype == np.float32
    return wn, mn, vn


def adam_step64(w, m, v, g, lr, t, beta1=.9, beta2=.999, eps=1e-8):
    """The same update in float64 (for the CPU restatement of a training run)."""
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    alpha = lr * math.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    return w - alpha * m / (np.sqrt(v) + eps), m, v


def cosine_lr(lr, epoch, epochs):
    return lr * 0.5 * (1.0 + math.cos(math.pi * epoch / epochs))


def int_case(seed, pixels, cin, cout, x_ld=None, dy_ld=None):
    """Integers in [-4, 4] as float32: every product is at most 16 in magnitude, so every partial sum over P pixels is an integer
    of magnitude <= 16 P: exact in float32, in any order, for up to 2^20 pixels (16 P <= 2^24).
    -> (x [P, x_ld], dy [P, dy_ld]) with NaN in the pad columns."""
    rng = np.random.default_rng(seed)
    x_ld, dy_ld = x_ld or cin, dy_ld or cout
    x = np.full((pixels, x_ld), np.nan, np.float32)
    dy = np.full((pixels, dy_ld), np.nan, np.float32)
    x[:, :cin] = rng.integers(-4, 5, (pixels, cin))
    dy[:, :cout] = rng.integers(-4, 5, (pixels, cout))
    return x, dy
