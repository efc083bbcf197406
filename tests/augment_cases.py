"""The inputs the augmentation tests share (tests/test_augment_host.py, tests/test_gpu_augment.py): five sources of different
sizes, three canvases, one row of ten draws per image and the boxes.  Everything is built once and left unchanged.

Sources: 5x7 random; 9x4 greys with black pixels (range == 0 in both colour kernels); 13x13 saturated primaries and secondaries in
2x2 patches (ties r == g == v, and ties between the patches under the bilinear resize); 20x3 random; 61x45 random with a black
block.  Canvases: 8x12 (24 quads: one partly filled workgroup per image), 36x52 and 52x36 (468 quads: two workgroups per image,
the second partly filled).  The first five draws of a row are the geometry sets the host test pins by hand."""
import numpy as np

from tests import augment_ref as ar

F = np.float32
SOURCES = [(5, 7), (9, 4), (13, 13), (20, 3), (61, 45)]
CANVASES = [(8, 12), (36, 52), (52, 36)]
# j1, j2, scale, dx, dy | flip, hue, sat, gamma, contrast
DRAWS = np.array([[.5, .5, .1, .3, .6, .2, .10, .20, .00, .10],
                  [.5, .5, .9, .3, .6, .7, .90, .80, .50, .90],
                  [.1, .9, .3, .5, .5, .4, .50, .50, .99, .50],
                  [.0, .0, .0, .0, .0, .9, .30, .05, .30, .00],
                  [.5, .5, .1, .3, .6, .1, .75, .95, .70, .99]], F)
DRAWS.setflags(write=False)
MAX_IN = 40
_cache = {}


def images():
    if 'img' not in _cache:
        rs = np.random.RandomState(21)
        imgs = [rs.randint(0, 256, size=d + (3,)).astype(np.uint8) for d in SOURCES]
        grey = rs.randint(0, 256, size=SOURCES[1]).astype(np.uint8)
        grey[::3, ::2] = 0
        imgs[1] = np.repeat(grey[:, :, None], 3, axis=2)
        colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
        patch = colours[rs.randint(0, 8, size=(7, 7))]
        imgs[2] = np.repeat(np.repeat(patch, 2, axis=0), 2, axis=1)[:13, :13].copy()
        imgs[4][10:30, 5:25] = 0
        for im in imgs:
            im.setflags(write=False)
        _cache['img'] = imgs
    return _cache['img']


def geometries(size, stages):
    """The restatement's geometry of the five images on one canvas."""
    key = ('geo', size, stages)
    if key not in _cache:
        _cache[key] = [ar.geometry(d[0], d[1], size, DRAWS[i], stages) for i, d in enumerate(SOURCES)]
    return _cache[key]


def coverage():
    """What the draws reach over all canvases: window kinds, flip values, the ratio clamp on and off."""
    kinds, flips, clamps = set(), set(), set()
    for size in CANVASES:
        for g in geometries(size, 0):
            kinds.add(ar.window_kind(g, size))
            flips.add(g['flip'])
            clamps.add(g['clamped'])
    return kinds, flips, clamps


def boxes(size):
    """-> (boxes [5,MAX_IN,5], counts [5]): random rows on every image, and some made for one branch each -
    image 0 (flipped): a row whose mapped xmin lies in [0, 1), so that the flip moves its xmax beyond W - 1, across the clip edge;
    image 1 (cropped on both axes on every canvas): a row inside the source that is more than 1 wide after the mapping and at most 1
    wide once the crop has cut it (it is clipped to the canvas);
    image 2: 30 rows that pass the filter (the cap at 20);
    image 3: box_count 0 (its rows must not be read as boxes)."""
    key = ('boxes', size)
    if key in _cache:
        return _cache[key]
    rs = np.random.RandomState(33)
    geo = geometries(size, 0)
    out = np.zeros((len(SOURCES), MAX_IN, 5), F)
    counts = np.array([MAX_IN, MAX_IN, 30, 0, MAX_IN], np.int32)

    def src_x(g, x):      # the source abscissa that maps near canvas abscissa x (before the flip)
        return (x - float(g['dx_f'])) * g['iw'] / float(g['nw_f'])

    def src_y(g, y):
        return (y - float(g['dy_f'])) * g['ih'] / float(g['nh_f'])
    for i, (ih, iw) in enumerate(SOURCES):
        g = geo[i]
        rows = []
        if i == 0:
            rows.append([src_x(g, 0.5), src_y(g, 1), src_x(g, 6), src_y(g, size[0] - 2), 4])
        if i == 2:
            for k in range(30):
                rows.append([src_x(g, 1 + 0.1 * k), src_y(g, 1), src_x(g, size[1] - 3 - 0.1 * k), src_y(g, size[0] - 2), k % 20])
        if i == 1:
            rows.append([src_x(g, -9), src_y(g, 1), src_x(g, 0.5), src_y(g, size[0] - 2), 9])
        while len(rows) < MAX_IN:
            x = np.sort(rs.uniform(-0.2 * iw, 1.2 * iw, 2))
            y = np.sort(rs.uniform(-0.2 * ih, 1.2 * ih, 2))
            rows.append([x[0], y[0], x[1], y[1], rs.randint(0, 20)])
        out[i] = np.asarray(rows[:MAX_IN], F)
    out.setflags(write=False)
    _cache[key] = (out, counts)
    return _cache[key]
