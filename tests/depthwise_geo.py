"""The launch geometry of the three inference depthwise kernel families, restated in plain Python, and the case tables of
tests/test_gpu_depthwise_forms.py built from it.

  dwp_geometry    == dwp_geometry() + launch_dwp_t() in yoloret_amd/csrc/depthwise_lds.hip   (LDS-tiled form, a walker per run of tiles)
  dwq_geometry    == dwq_geometry() / dwq_quanta() in yoloret_amd/csrc/depthwise_walk.hip    (row-walking form, 5 x 5)
  dw_se_geometry  == dw_se_geometry() in yoloret_amd/csrc/depthwise.hip                       (squeeze-excite form of dw_kernel)
  dw_instance     == the choice at the end of launch_depthwise_t() in depthwise.hip

Integer arithmetic only, the same operations in the same order as the sources.  tests/test_depthwise_geo_host.py pins this file
(against yoloret_amd.compiler where the compiler restates the same functions, and the class counts of the tables); the GPU tests
assert the kernel name every launch reports against what this file predicts.
"""
import collections
import functools

DWP_MAX_R = 6
DWP_SLOTS = 3 * 256          # walkers of one generation (launch_dwp_t)
DW_BIG_LANES = 1 << 21       # launch_depthwise_t: stride-2 3 x 3 maps with at least this many lanes take 2-row patches

Dwp = collections.namedtuple('Dwp', 'tw th R nband nbig ntx nty')
Dwq = collections.namedtuple('Dwq', 'nblk spb U ni nw Q nq')


def round_up(v, m):
    return (v + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------- dwp_kernel (depthwise_lds.hip)
def dwp_geometry(h, w, k=3, se=False):
    """Output tile tw x th, rows per band R (the template argument), bands, bands of R rows (the others have R - 1), tiles along x / y."""
    halo = k - 1
    cap = 192 if se else 208
    row_cost, in_cost, round_cost, tile_cost = k * k * 4 + 21, 3 * (4 + halo), 12, 60
    best, geo = 0, None
    for tw in range(8, 33, 8):
        cols, nstrip = tw + halo, tw // 4
        th = cap // cols - halo
        if th < 1:
            continue
        if th > h:
            th = h
        nty = (h + th - 1) // th
        th = (h + nty - 1) // nty
        ntx = (w + tw - 1) // tw
        nband = 8 // nstrip
        if nband > th:
            nband = th
        r = (th + nband - 1) // nband
        if r > DWP_MAX_R:
            continue
        npix = (th + halo) * cols
        rounds = (npix + 31) // 32
        cost = (ntx * nty) * (row_cost * r + in_cost * (r + halo) + round_cost * rounds + tile_cost)
        if best == 0 or cost < best:
            best = cost
            geo = Dwp(tw, th, r, nband, th - nband * (r - 1), ntx, nty)
    assert geo is not None, (h, w, k, se)
    return geo


def dwp_class(g):
    return g[:5]


def dwp_runs(b, c, g):
    """[(first, end)] tile positions (image-major, then tile row, then tile column) of every walker of one 64-channel chunk."""
    ncc = ((c + 7) // 8 + 7) // 8
    nq = b * g.ntx * g.nty
    G = DWP_SLOTS // ncc
    if G < 1:
        G = 1
    if G > nq:
        G = nq
    return [(i * nq // G, (i + 1) * nq // G) for i in range(G)]


def dwp_run_facts(b, c, g):
    """What the walkers of a launch do: the set of run lengths, whether some run passes from one tile row to the next inside an
    image, whether some run passes from one image to the next."""
    lengths, row_cross, image_cross = set(), False, False
    per_image = g.ntx * g.nty
    for q0, q1 in dwp_runs(b, c, g):
        lengths.add(q1 - q0)
        for q in range(q0 + 1, q1):
            if q % per_image == 0:
                image_cross = True
            elif q % g.ntx == 0:
                row_cross = True
    return lengths, row_cross, image_cross


def dwp_tile_regions(h, w, g):
    """[(y0, y1, x0, x1)] of the rows of the squeeze-excite sums, in row order (tile row major)."""
    return [(ty * g.th, min(h, (ty + 1) * g.th), tx * g.tw, min(w, (tx + 1) * g.tw)) for ty in range(g.nty) for tx in range(g.ntx)]


# ---------------------------------------------------------------------------------------------------- dwq_kernel (depthwise_walk.hip)
def dwq_quanta(h, k=5):
    q = h // 10
    if q < 1:
        q = 1
    if q > 8:
        q = 8
    Q = round_up((h + q - 1) // q, k)
    return Q, (h + Q - 1) // Q


def dwq_geometry(h, w, b, k=5, se=False):
    """Column blocks, strips per block, pixel groups of an LDS row, images and waves per workgroup, rows per quantum, quanta."""
    halo = k - 1
    strips = (w + 3) // 4
    wave_cap = 12 if k == 5 else 16
    nblk = (strips + 7) // 8
    spb = (strips + nblk - 1) // nblk
    colsp = round_up(spb * 4 + halo, 8)
    U = colsp // 8
    per_cu, sel_ni, sel_nw = 0, 0, 0
    for ni in (1, 2):
        if ni * spb > 8 or ni > b:
            break
        nw = (ni * spb + 1) // 2
        if (k * ni * U + nw - 1) // nw > 10:
            continue
        lds = k * ni * colsp * 32 * 8 + (2 * 256 * 8 if se else 0)
        pc = 160 * 1024 // lds
        if pc > wave_cap // nw:
            pc = wave_cap // nw
        if ni == 1 or pc * nw >= per_cu * sel_nw:
            sel_ni, sel_nw, per_cu = ni, nw, pc
    assert per_cu >= 1, (h, w, b)
    Q, nq = dwq_quanta(h, k)
    return Dwq(nblk, spb, U, sel_ni, sel_nw, Q, nq)


def dwq_segments(h, w, b, c, k=5, se=False):
    """(quanta per segment, segments per image) a launch cuts the rows into - the one choice that depends on the batch and on the
    channels (the sums do not: one row per quantum whatever the segments).  The source compares costs in double precision:
    Python's float is the same type and the operations are written in the same order."""
    halo = k - 1
    g = dwq_geometry(h, w, b, k, se)
    colsp = round_up(g.spb * 4 + halo, 8)
    lds = k * g.ni * colsp * 32 * 8 + (2 * 256 * 8 if se else 0)
    per_cu = min(160 * 1024 // lds, (12 if k == 5 else 16) // g.nw)
    ncc = ((c + 7) // 8 + 7) // 8
    nig = (b + g.ni - 1) // g.ni
    slots, units = 256 * per_cu, ncc * nig * g.nblk
    row_cost, in_cost, seg_cost = k * k * 5 + 45, 30, 600
    best, sel = 0.0, None
    for qps in range(1, g.nq + 1):
        nseg = (g.nq + qps - 1) // qps
        if (nseg - 1) * qps >= g.nq:
            continue
        n = qps * g.Q if qps * g.Q < h else h
        gens = float(units * nseg) / float(slots)
        if gens < 1:
            gens = 1.0
        cost = gens * (float(n) * row_cost + halo * in_cost + seg_cost)
        if best == 0 or cost <= best:
            best, sel = cost, (qps, nseg)
    return sel


def dwq_class(g):
    return (g.spb, g.ni, g.nw, g.U)


def dwq_regions(h, w, g):
    """[(y0, y1, x0, x1)] of the rows of the squeeze-excite sums, in row order (column block major, then quantum)."""
    return [(qi * g.Q, min(h, (qi + 1) * g.Q), blk * g.spb * 4, min(w, (blk + 1) * g.spb * 4)) for blk in range(g.nblk) for qi in range(g.nq)]


def dwq_last_quantum(h, g):
    return h - (g.nq - 1) * g.Q


# ---------------------------------------------------------------------------------------------------- dw_kernel (depthwise.hip)
def dw_se_geometry(strips, c4):
    """(channel vectors per workgroup, workgroups per strip group, rows of the partial-sum buffer)."""
    cw = 32
    if c4 <= 256:
        busy_a = (256 // c4) * c4 * ((c4 + 31) // 32) * 32
        if busy_a >= c4 * 256:
            cw = c4
    return cw, (c4 + cw - 1) // cw, (strips + 256 // cw - 1) // (256 // cw)


def dw_instance(k, s, b, h, w, c, vec):
    """(K, S, XT, YT) launch_depthwise_t picks for the plain form of a map h x w (input) with c channels, `vec` channels per lane."""
    ho, wo = (h + s - 1) // s, (w + s - 1) // s
    big = b * ho * wo * ((c + vec - 1) // vec) >= DW_BIG_LANES
    if s == 1:
        return (k, 1, 4, 1)
    if k == 3:
        return (3, 2, 2, 2) if big else (3, 2, 2, 1)
    return (5, 2, 2, 1)


DW_INSTANCES = [(3, 1, 4, 1), (3, 2, 2, 1), (3, 2, 2, 2), (5, 1, 4, 1), (5, 2, 2, 1)]      # what a normal build can launch


# ---------------------------------------------------------------------------------------------------- kernel names (yr_last_kernel)
def act_variant(act):
    return {'relu6': 0, 'swish': 1}.get(act, 2)


def dwp_name(dt, k, act, se, r):
    return 'dwp_kernel<%s,%d,%d,%d,%d>' % (dt, k, act_variant(act), int(se), r)


def dwq_name(dt, k, act, se):
    return 'dwq_kernel<%s,%d,%d,%d>' % (dt, k, act_variant(act), int(se))


def dw_name(dt, inst, se=False):
    k, s, xt, yt = inst
    return 'dw_kernel<%d,%d,%d,%d,%s,%d>' % (k, s, xt, 1 if se else yt, dt, int(se))


# ---------------------------------------------------------------------------------------------------- case tables
SWEEP = 80           # the classes are those of the maps 1 .. SWEEP x 1 .. SWEEP
MAX_BYTES = 20 << 20         # no tensor of a case beyond this, but the one big-branch case of dw_kernel
MAX_BYTES_BIG = 150 << 20
DWP_C = 72                   # one whole 64-channel chunk + a chunk with one channel vector (72 = 9 x 8)
TAIL_C = 76                  # the same chunks, the last vector half filled (76 = 9 x 8 + 4)
WALK_C = 1024                # 16 chunks: 48 walkers per chunk


@functools.lru_cache(None)
def dwp_class_table(se):
    """{class: (smallest map, smallest map of at least 2 x 2 tiles whose last tile is cut short along x and along y, or None)} over
    the 3 x 3 maps of the sweep; 'smallest' by pixels, then by height."""
    single, multi = {}, {}
    for h in range(1, SWEEP + 1):
        for w in range(1, SWEEP + 1):
            g = dwp_geometry(h, w, 3, se)
            key = (h * w, h, w)
            cls = dwp_class(g)
            if cls not in single or key < single[cls]:
                single[cls] = key
            if g.ntx >= 2 and g.nty >= 2 and w % g.tw and h % g.th and (cls not in multi or key < multi[cls]):
                multi[cls] = key
    return {cls: (single[cls][1:], multi[cls][1:] if cls in multi else None) for cls in sorted(single)}


def dwp_class_cases(se):
    """[(class, (h, w) single tile, (h, w) ragged 2 x 2 or more)]"""
    return [(cls, a, b) for cls, (a, b) in dwp_class_table(se).items()]


# multi-tile walks: (h, w, batch) at WALK_C channels - the batches are chosen so that the conditions in
# tests/test_depthwise_geo_host.py hold (run lengths 1, 2, 3; both parities; runs across tile rows and images)
WALK_CASES = [(20, 36, 5), (20, 36, 13), (26, 26, 9)]

# dwq: (h, w, batch), each run in the plain and in the squeeze-excite form (whose LDS need, and with it the two-image choice, differs:
# ten classes each, eleven together).  All (spb, ni, nw, U) classes; last quanta of 1, 2, 3 and 4 rows (and whole ones); maps lower than the
# kernel (h < 5, h = 1); odd batches in the two-image classes (the second image slot of the last workgroup is empty).
DWQ_CASES = [
    (31, 3, 1),      # (1,1,1,1)  three quanta of 15 rows, the last one 1 row
    (4, 7, 1),       # (2,1,1,2)  h < 5
    (1, 8, 3),       # (2,2,2,2)  h = 1, odd batch
    (32, 6, 2),      # (2,2,2,2)  last quantum 2 rows, even batch
    (33, 10, 1),     # (3,1,2,2)  last quantum 3 rows
    (34, 12, 3),     # (3,2,3,2) plain, (3,1,2,2) squeeze-excite; last quantum 4 rows, odd batch
    (23, 13, 3),     # (4,1,2,3) plain, (4,2,4,3) squeeze-excite; odd batch; two quanta of 15: the last one 8 rows
    (9, 15, 1),      # (4,1,2,3) in both forms
    (7, 19, 1),      # (5,1,3,3)
    (21, 24, 2),     # (6,1,3,4)
    (32, 27, 1),     # (7,1,4,4)
    (3, 31, 2),      # (8,1,4,5)  widths 29 .. 32, h < 5
    (33, 66, 1),     # three column blocks of six strips (17 strips)
]

# dwq segments of several quanta: every case above (and every 5 x 5 op-level case with 64 .. 136 channels at batches up to 400) leaves
# the cost model at one quantum per segment - the workgroups do not fill the chip.  WALK_C channels on a one-strip map do:
# (h, w, batch) -> a whole image of three quanta (15 + 15 + 1 rows) in one segment; two segments of two quanta (the last 15 + 1 rows)
DWQ_SEG_CASES = [(31, 2, 127), (46, 1, 100)]

# dw_kernel, plain form: (k, s, h, w, batch) per instantiation, small; channels per type below.  Odd sizes, several workgroups.
DW_SMALL_CASES = [(3, 1, 11, 13, 3), (3, 2, 11, 13, 3), (3, 2, 8, 6, 9), (5, 1, 7, 9, 3), (5, 2, 11, 13, 3), (5, 2, 6, 8, 9)]
DW_SMALL_C = {'f32': 42, 'bf16': 44, 'f16': 52}        # below 64 (the 16-bit stride-1 maps stay on dw_kernel), with a channel tail
# the big branch: 129 x 131 -> 65 x 66 = 4290 output pixels, three channel vectors a pixel (with a tail); the smallest batch that
# reaches 2^21 lanes and the one below it
DW_BIG_HW = (129, 131)
DW_BIG_C = {'f32': 10, 'bf16': 20, 'f16': 18}
DW_BIG_DISTINCT = 5          # distinct images, repeated round robin


def dw_big_batches():
    ho, wo = (DW_BIG_HW[0] + 1) // 2, (DW_BIG_HW[1] + 1) // 2
    b = -(-DW_BIG_LANES // (ho * wo * 3))
    return b, b - 1


# dw_kernel, squeeze-excite form: (dt, k, s, h, w, c, batch): cw = C4 that divides 256, cw = C4 that does not, 32-vector blocks with
# ncb > 1 (and a ragged last block)
DW_SE_CASES = [('f32', 3, 1, 9, 11, 64, 3), ('f32', 3, 2, 11, 13, 10, 3), ('f32', 5, 1, 7, 6, 520, 2), ('f32', 5, 2, 9, 9, 160, 2),
               ('bf16', 3, 2, 11, 13, 100, 3), ('f16', 5, 2, 9, 7, 1100, 2), ('bf16', 3, 1, 6, 9, 44, 3), ('f16', 5, 1, 5, 5, 20, 2)]
