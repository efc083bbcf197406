"""The 4x4-max-pooled source of a POINTWISE op (YR_X_MAXPOOL4: the RFCR weighted sum reads block_2's map through it).

One op over [up2 | identity | identity | maxpool4] sources through yr_op_run, every source between red zones (a window tap
beyond the pooled map's B x h x w x ld elements would read the guard, and the two fence variants would then differ):
  * bit for bit the result of the SAME op fed the host-pooled map as an identity source - the window maximum is exact, so how the
    sixteen taps are fetched may not show in the result;
  * the same bits for every tile shape (one and several pixel tiles per wave, one and two k chunks in flight);
  * the NumPy oracle's conv over the concatenation at the pointwise tests' tolerance (3e-5 scaled).
Sizes: an 8 x 8 map -> 2 x 2 output (one window per output pixel, a single partial tile), a 20 x 28 map -> 5 x 7 (70 pixels: a full
64-row tile and a ragged one) and a 24 x 40 map -> 6 x 10.  An up-sampled source exists only for even output sizes (yr_op_run
refuses the op otherwise), so the 5 x 7 case reads its first source as an identity; the 6 x 10 case is the ragged one with the
up-sampled source in place.  The pooled source has 24 channels (six full quads, as in the network) or 20 (its last quad ends
the k space: the clamped k tail re-reads it).
"""
import zlib

import numpy as np
import pytest
import torch

from oracle import nn
from tests import fence
from tests.util import assert_close, from_dev, round_up, to_dev

pytestmark = pytest.mark.gpu

B = 2
COUT = 48
TOL = 3e-5                       # the pointwise tests' bar (tests/test_gpu_hoist.py)
CFGS = (0, 1, 8, 12, 19)         # heuristic | 256 x 16 | 64 x 16 (two chunks in flight) | 64 x 80 (the RFCR sum's shape) | 128 x 80 through a direct kernel's index


def _run(rt, dev, srcs, wt, h, w, cfg):
    """srcs: [(device tensor, channels, xform)]; -> [B, h, w, COUT] float32 (NumPy)"""
    op = rt.new_op(rt.OP_POINTWISE, 'none')
    op.h, op.w, op.cout, op.nsrc = h, w, COUT, len(srcs)
    op.cin = sum(c for _, c, _ in srcs)
    for i, (t, c, xf) in enumerate(srcs):
        op.src[i] = rt.make_src(t, c=c, xform=xf)
    op.wgt = wt.data_ptr()
    out = torch.full((B, h, w, round_up(COUT, 4)), float('nan'), dtype=torch.float32, device=dev)
    op.out, op.out_ld, op.k = out.data_ptr(), out.shape[3], cfg
    fence.run_op(op, B, writes=[out], reads=[t for t, _, _ in srcs] + [wt])
    torch.cuda.synchronize()
    return np.ascontiguousarray(from_dev(out, COUT))


@pytest.mark.parametrize('pc', [24, 20], ids=['c24', 'c20'])
@pytest.mark.parametrize('h,w,first', [(2, 2, 'up2'), (5, 7, 'identity'), (6, 10, 'up2')], ids=['2x2', '5x7', '6x10'])
def test_maxpool4_source_equals_the_host_pooled_identity_source(dev, h, w, first, pc):
    from yoloret_amd import runtime as rt
    rng = np.random.default_rng(zlib.crc32(repr((h, w, first, pc)).encode()))
    cs = [12, 16, 10, pc]
    fh, fw = (h // 2, w // 2) if first == 'up2' else (h, w)
    x0 = rng.standard_normal((B, fh, fw, cs[0])).astype(np.float32)
    x1 = rng.standard_normal((B, h, w, cs[1])).astype(np.float32)
    x2 = rng.standard_normal((B, h, w, cs[2])).astype(np.float32)
    x3 = rng.standard_normal((B, 4 * h, 4 * w, cs[3])).astype(np.float32)
    wy, wx = np.arange(4 * h)[:, None] // 4, np.arange(4 * w)[None, :] // 4
    x3[:, (wy + wx) % 2 == 1, :] -= 8.0                     # every other window lies below zero as a whole: maxima of mixed sign
    x3[x3 == 0] = 0.5                                       # ... and nonzero: the maximum has one bit pattern
    x3[:, ::4, ::4, : pc // 2] -= 4.0                       # windows whose first tap is the smallest ...
    x3[:, 3::4, 3::4, pc // 2:] += 4.0                      # ... and windows whose last tap is the largest
    pooled = nn.maxpool(x3, 4)
    assert (pooled != 0).all() and (pooled < 0).any() and (pooled > 0).any()
    cin = sum(cs)
    wk = (rng.standard_normal((cin, COUT)) * np.sqrt(2.0 / cin)).astype(np.float32)
    wt = np.zeros((COUT, sum(round_up(c, 4) for c in cs)), np.float32)      # k space: every source padded to whole quads
    kb = d = 0
    for c in cs:
        wt[:, kb:kb + c] = wk[d:d + c].T
        d += c
        kb += round_up(c, 4)
    ref = nn.pointwise(nn.concat([nn.upsample2(x0) if first == 'up2' else x0, x1, x2, pooled]), wk)

    wt_d = torch.from_numpy(wt).to(dev)
    t0, t1, t2, t3, tp = [to_dev(a, dev) for a in (x0, x1, x2, x3, pooled)]
    head = [(t0, cs[0], first), (t1, cs[1], 'identity'), (t2, cs[2], 'identity')]
    for cfg in CFGS:
        got = _run(rt, dev, head + [(t3, pc, 'maxpool4')], wt_d, h, w, cfg)
        want = _run(rt, dev, head + [(tp, pc, 'identity')], wt_d, h, w, cfg)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), 'pooled on the fly != host-pooled, cfg %d' % cfg
        if cfg == CFGS[0]:
            first_bits = got.view(np.uint32).copy()
            assert_close(got, ref, TOL, 'pooled-source conv %dx%d c%d' % (h, w, pc))
        else:
            assert np.array_equal(got.view(np.uint32), first_bits), 'tile shape %d rounds differently' % cfg
