"""NumPy float32 restatement of the reference's validation data transform (test infrastructure only):
code/yolo3/utils.py:239-295, get_random_data(train=False, zoom_in=False) - geometry, resize with a given geometry, pad, clip,
box mapping, filter, cap - and of letterbox_image's geometry (utils.py:76-79) for comparison.

Every value is an np.float32 and every operation one float32 operation in TensorFlow's order; NumPy neither contracts nor
reassociates.  tests/test_valdata_host.py pins the functions by answers derived by hand."""
import numpy as np

F = np.float32


def validate_geometry(ih, iw, size):
    """-> (nh, nw, dy, dx, nh_f, nw_f, dy_f, dx_f): :152-155 casts to float32, :239-242, then :247-250 truncate (tf.cast to int32)."""
    h, w = F(size[0]), F(size[1])
    ihf, iwf = F(ih), F(iw)
    m = np.minimum(w / iwf, h / ihf)
    nh_f = ihf * m
    nw_f = iwf * m
    dx_f = (w - nw_f) / F(2)
    dy_f = (h - nh_f) / F(2)
    return int(nh_f), int(nw_f), int(dy_f), int(dx_f), nh_f, nw_f, dy_f, dx_f


def letterbox_geometry(ih, iw, size):
    """-> (nh, nw, dy, dx) of letterbox_image: the ratio in float64, truncated sizes, floor-divided offsets (:76-79)."""
    h, w = int(size[0]), int(size[1])
    r = min(w / iw, h / ih)
    nh, nw = int(float(ih) * r), int(float(iw) * r)
    return nh, nw, (h - nh) // 2, (w - nw) // 2


def resize_pad(img_u8, size, geom, clip):
    """uint8 [ih,iw,3] -> float32 [h,w,3]: decode_image(dtype=float32) = u8 * (1/255), tf.image.resize to (nh, nw) (bilinear, half-pixel
    centres, no antialias), pad_to_bounding_box(dy, dx) with zeros, optionally clip_by_value(0, 1) (:277)."""
    ih, iw = img_u8.shape[:2]
    h, w = int(size[0]), int(size[1])
    nh, nw, dy, dx = geom
    f = img_u8.astype(F) * F(1.0 / 255.0)
    sy, sx = F(ih) / F(nh), F(iw) / F(nw)
    fy = (np.arange(nh, dtype=F) + F(0.5)) * sy - F(0.5)
    fx = (np.arange(nw, dtype=F) + F(0.5)) * sx - F(0.5)
    y0 = np.maximum(np.floor(fy).astype(np.int64), 0)
    y1 = np.minimum(np.ceil(fy).astype(np.int64), ih - 1)
    x0 = np.maximum(np.floor(fx).astype(np.int64), 0)
    x1 = np.minimum(np.ceil(fx).astype(np.int64), iw - 1)
    ly = (fy - np.floor(fy)).astype(F)[:, None, None]
    lx = (fx - np.floor(fx)).astype(F)[None, :, None]
    tl, tr = f[y0][:, x0], f[y0][:, x1]
    bl, br = f[y1][:, x0], f[y1][:, x1]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    res = (top + (bot - top) * ly).astype(F)
    if clip:
        res = np.maximum(np.minimum(res, F(1)), F(0))
    out = np.zeros((h, w, 3), F)
    out[dy:dy + nh, dx:dx + nw] = res
    return out


def validate_image(img_u8, size):
    nh, nw, dy, dx = validate_geometry(img_u8.shape[0], img_u8.shape[1], size)[:4]
    return resize_pad(img_u8, size, (nh, nw, dy, dx), clip=True)


def map_boxes(boxes, ih, iw, size, max_boxes=20):
    """boxes float32 [n,5] rows (xmin, ymin, xmax, ymax, label) in source pixels -> (out [max_boxes,5] float32, the kept rows in
    front and zeros behind; kept; info): :253-256 with the untruncated float32 geometry, :258-273 clip, :289-291 filter, :292-293 cap.
    info counts the branches: rows dropped by width, by height (with a passing width), kept before the cap."""
    boxes = np.asarray(boxes, F).reshape(-1, 5)
    _, _, _, _, nh_f, nw_f, dy_f, dx_f = validate_geometry(ih, iw, size)
    ihf, iwf = F(ih), F(iw)
    xmax, ymax = F(int(size[1]) - 1), F(int(size[0]) - 1)

    def clip(v, hi):
        return np.maximum(np.minimum(v, hi), F(0))
    x0 = clip(boxes[:, 0] * nw_f / iwf + dx_f, xmax)
    x1 = clip(boxes[:, 2] * nw_f / iwf + dx_f, xmax)
    y0 = clip(boxes[:, 1] * nh_f / ihf + dy_f, ymax)
    y1 = clip(boxes[:, 3] * nh_f / ihf + dy_f, ymax)
    assert x0.dtype == F and y1.dtype == F
    bw, bh = x1 - x0, y1 - y0
    keep = np.logical_and(bw > 1, bh > 1)
    rows = np.stack([x0, y0, x1, y1, boxes[:, 4]], axis=1)[keep]
    info = {'drop_w': int((~(bw > 1)).sum()), 'drop_h': int(((bw > 1) & ~(bh > 1)).sum()), 'passed': int(keep.sum()), 'w': bw, 'h': bh}
    rows = rows[:max_boxes]
    out = np.zeros((max_boxes, 5), F)
    out[:rows.shape[0]] = rows
    return out, rows.shape[0], info
