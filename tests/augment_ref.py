"""NumPy float32 restatement of the reference's training data transform (test infrastructure only):
code/yolo3/utils.py:170-237, get_random_data(train=True), then :258-293 - geometry from ten draws, resize / crop / pad, flip,
random_hue, random_saturation, adjust_gamma, random_contrast, clip, and the boxes.

Every value is an np.float32 and every operation one float32 operation in TensorFlow's order; NumPy neither contracts nor
reassociates.  tests/test_augment_host.py pins the functions by answers derived by hand.

TensorFlow is not available to this project.  ``adjust_hue`` and ``adjust_saturation`` below are TF 2.x's fused CPU kernels as
best restated from memory, so THIS TEXT IS THE DEFINITION UNDER TEST, not TensorFlow: parity with TensorFlow's bytes is unpinned,
as it is for the oracle.  Choices made here:
  * the 2/6 and 4/6 offsets of the RGB -> HSV hue are float32 quotients, F(2) / F(6) and F(4) / F(6) (not doubles rounded
    afterwards, which gives the same two float32 values, and not a double sum);
  * the wrap of the hue into [0, 6) adds 6 while negative first, then subtracts 6 while >= 6 (so -tiny + 6 == 6.0 wraps to 0);
  * fmod2 does the same with 2;
  * the channel mean of adjust_contrast is a float32 sum over the canvas (NumPy's pairwise order) divided by float32(H * W); the
    summation order is not part of the contract, the device result is compared with the float64 evaluation below.
random_jpeg_quality (on by default in the reference), val, noise, blur and zoom_in are not restated."""
import numpy as np

from tests import valdata_ref as vr

F = np.float32
DRAWS = ('j1', 'j2', 'scale', 'dx', 'dy', 'flip', 'hue', 'sat', 'gamma', 'contrast')
DEFAULTS = dict(jitter=.3, min_scale=.25, max_scale=2., hue=.5, sat=.5, min_gamma=.8, max_gamma=2., cont=.1)
HUE, SAT, GAMMA, CONTRAST, NOFLIP = 1, 2, 4, 8, 16


def uniform(u, lo, hi):
    """tf.random.uniform([], lo, hi) from the unit draw u: the bounds reach TF as Python doubles and are rounded to float32 once."""
    lo, hi = F(lo), F(hi)
    return F(lo + F(F(u) * F(hi - lo)))


def geometry(ih, iw, size, draws, stages=HUE | SAT | GAMMA | CONTRAST, **params):
    """-> dict with the fields of yr_augment_geom (without src_off): :171-181, the truncations of :183-198, the draws of :212-227."""
    p = dict(DEFAULTS, **params)
    u = [F(d) for d in draws]
    h, w = F(size[0]), F(size[1])
    H, W = int(size[0]), int(size[1])
    jlo, jhi = 1.0 - p['jitter'], 1.0 + p['jitter']
    new_ar = F(F(w / h) * F(uniform(u[0], jlo, jhi) / uniform(u[1], jlo, jhi)))
    scale = uniform(u[2], p['min_scale'], p['max_scale'])
    ratio = F(scale * new_ar) if new_ar < 1 else F(scale / new_ar)
    ratio = ratio if ratio > 1 else F(1)
    if new_ar < 1:
        nw, nh = F(ratio * h), F(scale * h)
    else:
        nw, nh = F(scale * w), F(ratio * w)
    dx = uniform(u[3], 0.0, F(w - nw))
    dy = uniform(u[4], 0.0, F(h - nh))
    g = dict(ih=int(ih), iw=int(iw), rh=int(nh), rw=int(nw), nh_f=nh, nw_f=nw, dy_f=dy, dx_f=dx, clamped=int(ratio == 1))
    if g['rh'] <= 0 or g['rw'] <= 0:
        raise ValueError('the resized image truncates to zero size')
    g['py'], g['px'] = int(max(dy, F(0))), int(max(dx, F(0)))
    if nw > w or nh > h:
        g['cy'], g['cx'] = int(max(-dy, F(0))), int(max(-dx, F(0)))
        g['wh'], g['ww'] = min(H, g['rh']), min(W, g['rw'])
        if g['cy'] + g['wh'] > g['rh'] or g['cx'] + g['ww'] > g['rw']:
            raise ValueError('crop_to_bounding_box would fail')
    else:
        g['cy'] = g['cx'] = 0
        g['wh'], g['ww'] = g['rh'], g['rw']
    if g['py'] + g['wh'] > H or g['px'] + g['ww'] > W:
        raise ValueError('pad_to_bounding_box would fail')
    g['flip'] = int(not (stages & NOFLIP) and u[5] < F(0.5))
    g['hue6'] = F(uniform(u[6], -p['hue'], p['hue']) * F(6)) if stages & HUE else F(0)
    g['sat'] = uniform(u[7], 1.0 - p['sat'], 1.0 + p['sat']) if stages & SAT else F(1)
    g['gamma'] = uniform(u[8], p['min_gamma'], p['max_gamma']) if stages & GAMMA else F(1)
    g['cont'] = uniform(u[9], 1.0 - p['cont'], 1.0 + p['cont']) if stages & CONTRAST else F(1)
    return g


def window_kind(g, size):
    """'pad', 'crop_x', 'crop_y' or 'crop_xy': which sides of the resized image exceed the canvas (:201-206)."""
    cx, cy = g['nw_f'] > F(size[1]), g['nh_f'] > F(size[0])
    return 'crop_xy' if cx and cy else 'crop_x' if cx else 'crop_y' if cy else 'pad'


def canvas(img_u8, size, g):
    """uint8 [ih,iw,3] -> float32 [H,W,3]: resize to (rh, rw) with valdata_ref.resize_pad's arithmetic, crop, pad (:182-206), flip (:212-217)."""
    H, W = int(size[0]), int(size[1])
    res = vr.resize_pad(img_u8, (g['rh'], g['rw']), (g['rh'], g['rw'], 0, 0), clip=False)
    win = res[g['cy']:g['cy'] + g['wh'], g['cx']:g['cx'] + g['ww']]
    out = np.zeros((H, W, 3), F)
    out[g['py']:g['py'] + g['wh'], g['px']:g['px'] + g['ww']] = win
    if g['flip']:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def _wrap(x, period):
    x = x.copy()
    p = F(period)
    while (x < 0).any():
        x = np.where(x < 0, x + p, x).astype(F)
    while (x >= p).any():
        x = np.where(x >= p, x - p, x).astype(F)
    return x


def adjust_hue(img, delta6):
    """img float32 [...,3], delta6 = delta * 6 (float32)."""
    img = np.asarray(img, F)
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    rg = r < g
    cat = np.where(rg, np.where(b < r, 1, np.where(b > g, 3, 2)), np.where(b < g, 0, np.where(b > r, 4, 5)))
    vmax = np.choose(cat, [r, g, g, b, b, r])
    vmid = np.choose(cat, [g, r, b, g, r, b])
    vmin = np.choose(cat, [b, b, r, r, g, g])
    rng = (vmax - vmin).astype(F)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = ((vmid - vmin).astype(F) / rng).astype(F)
    odd = (cat & 1) == 1
    h = (cat.astype(F) + np.where(odd, F(1) - ratio, ratio).astype(F)).astype(F)
    h = np.where(vmax == vmin, F(0), h).astype(F)
    h = _wrap((h + F(delta6)).astype(F), 6)
    cat = h.astype(np.int64)
    ratio = (h - cat.astype(F)).astype(F)
    ratio = np.where((cat & 1) == 1, F(1) - ratio, ratio).astype(F)
    vmid = (vmin + (ratio * rng).astype(F)).astype(F)
    out = np.stack([np.choose(cat, [vmax, vmid, vmin, vmin, vmid, vmax]),
                    np.choose(cat, [vmid, vmax, vmax, vmid, vmin, vmin]),
                    np.choose(cat, [vmin, vmin, vmid, vmax, vmax, vmid])], axis=-1)
    assert out.dtype == F
    return out


def adjust_saturation(img, factor):
    img = np.asarray(img, F)
    factor = F(factor)
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    rng = (v - np.minimum(np.minimum(r, g), b)).astype(F)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(v > 0, (rng / v).astype(F), F(0)).astype(F)
        norm = (F(1) / (F(6) * rng).astype(F)).astype(F)
        h = np.where(r == v, (norm * (g - b).astype(F)).astype(F),
                     np.where(g == v, ((norm * (b - r).astype(F)).astype(F) + F(2) / F(6)).astype(F),
                              ((norm * (r - g).astype(F)).astype(F) + F(4) / F(6)).astype(F))).astype(F)
    h = np.where(rng <= 0, F(0), h).astype(F)
    h = np.where(h < 0, h + F(1), h).astype(F)
    s = np.minimum(F(1), np.maximum(F(0), (s * factor).astype(F)))
    c = (s * v).astype(F)
    m = (v - c).astype(F)
    dh = (h * F(6)).astype(F)
    x = (c * (F(1) - np.abs(_wrap(dh, 2) - F(1)).astype(F)).astype(F)).astype(F)
    i = dh.astype(np.int64)
    z = np.zeros_like(c)
    sel = np.clip(i, 0, 6)
    rr = np.choose(sel, [c, x, z, z, x, c, z])
    gg = np.choose(sel, [x, c, c, x, z, z, z])
    bb = np.choose(sel, [z, z, x, c, c, x, z])
    out = np.stack([(rr + m).astype(F), (gg + m).astype(F), (bb + m).astype(F)], axis=-1)
    assert out.dtype == F
    return out


def pre_gamma(img_u8, size, g, stages):
    """The float32 canvas through hue and saturation: what adjust_gamma sees."""
    x = canvas(img_u8, size, g)
    if stages & HUE:
        x = adjust_hue(x, g['hue6'])
    if stages & SAT:
        x = adjust_saturation(x, g['sat'])
    return x


def clip01(x):
    return np.maximum(np.minimum(x, x.dtype.type(1)), x.dtype.type(0))


def gamma_contrast(x, g, stages, dtype=F):
    """adjust_gamma (gain 1, no clip), random_contrast with the per-channel mean over the whole canvas after gamma, the final clip
    (:277); evaluated in ``dtype`` from the float32 pre-gamma tensor.  -> (image, channel means or None)."""
    T = np.dtype(dtype).type
    x = np.asarray(x, F).astype(T)
    mean = None
    if stages & GAMMA:
        x = np.power(x, T(g['gamma']))
    if stages & CONTRAST:
        mean = (x.sum(axis=(0, 1), dtype=T) / T(x.shape[0] * x.shape[1])).astype(T)
        x = ((x - mean) * T(g['cont']) + mean).astype(T)
    assert x.dtype == np.dtype(dtype)
    return clip01(x), mean


def image(img_u8, size, g, stages, dtype=F):
    return gamma_contrast(pre_gamma(img_u8, size, g, stages), g, stages, dtype)[0]


def map_boxes(boxes, g, size, max_boxes=20):
    """boxes float32 [n,5] rows (xmin, ymin, xmax, ymax, label) in source pixels -> (out [max_boxes,5], kept, info): :208-211 with the
    untruncated floats, :212-217 the flip with w (not w - 1), then :258-293 as valdata_ref.map_boxes."""
    boxes = np.asarray(boxes, F).reshape(-1, 5)
    ihf, iwf, wf = F(g['ih']), F(g['iw']), F(size[1])
    xmax, ymax = F(int(size[1]) - 1), F(int(size[0]) - 1)
    x0 = boxes[:, 0] * g['nw_f'] / iwf + g['dx_f']
    x1 = boxes[:, 2] * g['nw_f'] / iwf + g['dx_f']
    y0 = boxes[:, 1] * g['nh_f'] / ihf + g['dy_f']
    y1 = boxes[:, 3] * g['nh_f'] / ihf + g['dy_f']
    if g['flip']:
        x0, x1 = wf - x1, wf - x0
    raw = np.stack([x0, y0, x1, y1], axis=1)

    def clip(v, hi):
        return np.maximum(np.minimum(v, hi), F(0))
    x0, x1, y0, y1 = clip(x0, xmax), clip(x1, xmax), clip(y0, ymax), clip(y1, ymax)
    assert x0.dtype == F and y1.dtype == F
    bw, bh = x1 - x0, y1 - y0
    keep = np.logical_and(bw > 1, bh > 1)
    rows = np.stack([x0, y0, x1, y1, boxes[:, 4]], axis=1)[keep]
    info = {'passed': int(keep.sum()), 'w': bw, 'h': bh, 'raw': raw, 'keep': keep}
    rows = rows[:max_boxes]
    out = np.zeros((max_boxes, 5), F)
    out[:rows.shape[0]] = rows
    return out, rows.shape[0], info
