"""The definition of the 3 x 3 entry-convolution operators of yoloret_amd/csrc/stemgrad.hip (yr_conv3x3_forward / _dgrad / _wgrad), written
from the order the header documents, not from the kernels.

Layouts are the device's: maps [B, H, W, C]; the weight w [9 * cin, cout] is the Keras kernel [3, 3, cin, cout] reshaped, row
r = (ky * 3 + kx) * cin + ci.  ``geometry`` is tests/convgrad_ref.geometry with k = 3.

* ``forward64`` / ``grads64``: float64, by patches (the yardstick; pinned against oracle.nn.conv2d and torch's conv2d with its autograd
  in tests/test_stemgrad_host.py).
* ``forward32`` / ``dgrad32`` / ``wgrad32``: float32 in THE ORDER of include/yoloret_hip.h, one ``fma32`` (tests/sefc_ref.py: float32(a * b + c)
  with one rounding) per term, every chain from +0, a padded tap SKIPPED (no operation: the chain keeps its bits).
    forward  for ky, for kx, for ci:                       acc = fma(x, w[r][co], acc)
    dgrad    for ky, for kx (those that meet an output pixel), for co:   acc = fma(dy, w[r][co], acc)
    wgrad    chunks of ``wgrad_chunk`` rows of the B * OH output rows; in a chunk, pixels i = 0, 1, .. in (row, column) order; partial sum
             s of ``wgrad_sets(cout)`` takes i = s, s + NS, ..: acc = fma(dy, x, acc); the partial sums are added ((s0 + s1) + s2) + s3,
             then the chunks' slabs in index order, the first term the slab itself."""
import numpy as np

from tests.convgrad_ref import geometry as _geometry, rel_err      # noqa: F401  (rel_err: the unit of the rounding bars)
from tests.sefc_ref import fma32

F32 = np.float32
MIN_PIXELS, MAX_CHUNKS = 256, 2048      # SG_MIN_PIXELS, SG_MAX_CHUNKS of csrc/stemgrad.hip


def geometry(h, w, stride, padding):
    """padding 'same' | (top, left, bottom, right) -> ((top, left, bottom, right), (oh, ow))"""
    return _geometry(h, w, 3, stride, padding)


def wgrad_chunk(b, oh, ow):
    """output rows per chunk: at least 256 pixels, at most 2048 chunks"""
    return max(-(-MIN_PIXELS // ow), -(-(b * oh) // MAX_CHUNKS))


def wgrad_sets(cout):
    """partial sums per chunk: 256 lanes over sets of round_up(9 * ceil(cout / 4), 64)"""
    items = 9 * (-(-cout // 4))
    return 256 // (-(-items // 64) * 64)


def _taps(h, w, stride, pads, oh, ow):
    """per tap t = ky * 3 + kx -> (iy [oh], ix [ow], valid [oh, ow])"""
    pt, pl = pads[0], pads[1]
    out = []
    for ky in range(3):
        for kx in range(3):
            iy, ix = np.arange(oh) * stride - pt + ky, np.arange(ow) * stride - pl + kx
            vy, vx = (iy >= 0) & (iy < h), (ix >= 0) & (ix < w)
            out.append((np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1), vy[:, None] & vx[None, :]))
    return out


def patches(x, stride, padding, dtype=np.float64):
    """x [B, H, W, cin] -> (P [B, OH, OW, 9, cin] with 0 at padded taps, valid [OH, OW, 9])"""
    x = np.asarray(x, dtype)
    b, h, w, cin = x.shape
    pads, (oh, ow) = geometry(h, w, stride, padding)
    p = np.zeros((b, oh, ow, 9, cin), dtype)
    valid = np.zeros((oh, ow, 9), bool)
    for t, (iy, ix, v) in enumerate(_taps(h, w, stride, pads, oh, ow)):
        p[:, :, :, t, :] = x[:, iy][:, :, ix] * v[None, :, :, None]
        valid[:, :, t] = v
    return p, valid


# ----------------------------------------------------------------------------- float64
def forward64(x, w, stride, padding):
    p, _ = patches(x, stride, padding)
    return p.reshape(p.shape[:3] + (-1,)) @ np.asarray(w, np.float64)


def grads64(x, w, dy, stride, padding):
    """-> (dx [B, H, W, cin], dw [9 * cin, cout]) of sum(forward(x, w) * dy)"""
    x, w, dy = (np.asarray(a, np.float64) for a in (x, w, dy))
    b, h, wd, cin = x.shape
    pads, (oh, ow) = geometry(h, wd, stride, padding)
    p, _ = patches(x, stride, padding)
    dw = p.reshape(-1, 9 * cin).T @ dy.reshape(-1, dy.shape[-1])
    dp = (dy @ w.T).reshape(b, oh, ow, 9, cin)
    dx = np.zeros_like(x)
    for t, (iy, ix, v) in enumerate(_taps(h, wd, stride, pads, oh, ow)):
        oys, oxs = np.nonzero(v)
        np.add.at(dx, (slice(None), iy[oys], ix[oxs]), dp[:, oys, oxs, t, :])
    return dx, dw


# ----------------------------------------------------------------------------- float32, in the documented order
def forward32(x, w, stride, padding):
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    b, h, wd, cin = x.shape
    pads, (oh, ow) = geometry(h, wd, stride, padding)
    acc = np.zeros((b, oh, ow, w.shape[1]), F32)
    for t, (iy, ix, v) in enumerate(_taps(h, wd, stride, pads, oh, ow)):
        xv = x[:, iy][:, :, ix]
        for ci in range(cin):
            new = fma32(xv[..., ci, None], w[t * cin + ci][None, None, None, :], acc)
            acc = np.where(v[None, :, :, None], new, acc)
    return acc


def dgrad32(dy, w, hw, stride, padding):
    dy, w = np.asarray(dy, F32), np.asarray(w, F32)
    b, oh, ow, cout = dy.shape
    h, wd = hw
    cin = w.shape[0] // 9
    pads, (eh, ew) = geometry(h, wd, stride, padding)
    assert (eh, ew) == (oh, ow)
    acc = np.zeros((b, h, wd, cin), F32)
    for ky in range(3):
        for kx in range(3):
            ny, nx = np.arange(h) + pads[0] - ky, np.arange(wd) + pads[1] - kx
            vy, vx = (ny >= 0) & (ny % stride == 0) & (ny // stride < oh), (nx >= 0) & (nx % stride == 0) & (nx // stride < ow)
            v = (vy[:, None] & vx[None, :])[None, :, :, None]
            g = dy[:, np.clip(ny // stride, 0, oh - 1)][:, :, np.clip(nx // stride, 0, ow - 1)]      # [b, h, wd, cout]
            wt = w[(ky * 3 + kx) * cin:(ky * 3 + kx + 1) * cin]                                     # [cin, cout]
            for co in range(cout):
                acc = np.where(v, fma32(g[..., co, None], wt[None, None, None, :, co], acc), acc)
    return acc


def wgrad_slabs32(x, dy, stride, padding):
    """-> the chunks' slabs [nchunks, 9 * cin, cout]"""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    b, oh, ow, cout = dy.shape
    cin = x.shape[3]
    p, valid = patches(x, stride, padding, F32)
    p = p.reshape(b * oh * ow, 9 * cin)
    v = np.broadcast_to(np.repeat(valid, cin, axis=2)[None], (b, oh, ow, 9 * cin)).reshape(b * oh * ow, 9 * cin)
    g = dy.reshape(b * oh * ow, cout)
    chunk, ns = wgrad_chunk(b, oh, ow), wgrad_sets(cout)
    rows = b * oh
    nchunks = -(-rows // chunk)
    first = np.arange(nchunks) * chunk * ow
    last = np.minimum((np.arange(nchunks) + 1) * chunk, rows) * ow
    acc = np.zeros((nchunks, ns, 9 * cin, cout), F32)
    j = 0
    while True:
        i = first[:, None] + np.arange(ns)[None, :] + j * ns       # [nchunks, ns]
        live = i < last[:, None]
        if not live.any():
            break
        ic = np.minimum(i, b * oh * ow - 1)
        new = fma32(g[ic][:, :, None, :], p[ic][:, :, :, None], acc)
        acc = np.where((live[:, :, None] & v[ic])[..., None], new, acc)
        j += 1
    slab = acc[:, 0]
    for s in range(1, ns):
        slab = slab + acc[:, s]
    assert slab.dtype == F32
    return slab


def wgrad32(x, dy, stride, padding):
    slabs = wgrad_slabs32(x, dy, stride, padding)
    out = slabs[0]
    for s in slabs[1:]:
        out = out + s
    assert out.dtype == F32
    return out


def padded(a, ld):
    """[..., C] -> [..., ld] with NaN in the pad columns"""
    out = np.full(a.shape[:-1] + (ld,), np.nan, np.float32)
    out[..., :a.shape[-1]] = a
    return out
