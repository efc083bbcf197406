"""The walking head kernel's SHARED ROW (headwalk.hip, two k chunks and more): wave c % 4 of a workgroup fetches chunk c of a strip
row, cuts it into its float16 planes and hands them to all four waves through a double-buffered LDS row, one barrier per row.

Through the C-ABI against the NumPy oracle with the harness and the bar of tests/test_gpu_head.py (split form: 5e-5), map,
squeeze-excite sums and gate, on the smallest shapes at which the hand-over can go wrong:
  * 1, 2 and 3 output rows per segment: the first buffer alone, both buffers, the odd tail row of the two-row loop; 17 rows: two
    segments of 9 and 8 rows;
  * widths 14 (one full strip), 15 (a second strip of one live column) and 29 (a third one);
  * k spaces of 40 (a whole chunk + a masked one of 8 channels: waves 2 and 3 own nothing), 96 (three chunks), 128 behind a gate
    (four: every wave owns one), 5 and 7 chunks (a wave owns two; one cout tile per wave, two workgroups per strip segment);
  * two sources whose boundary lies inside the chunk table (40 + 24: a masked chunk in the middle; 64 + 64 with the up-sampled
    addend; 40 + 75; 128 + 75);
  * F = 128 (every wave owns tiles), batch 3."""
import numpy as np
import pytest
import torch

from tests import fence
from tests.test_gpu_head import run_head, walk_ok

pytestmark = pytest.mark.gpu

ID = 'identity'
CASES = [
    # (h, w, segs, F, pre, gated, R)
    (1, 15, [(40, ID)], 128, False, False, 8),
    (2, 14, [(96, ID)], 128, False, False, 8),
    (3, 29, [(128, ID)], 128, False, True, 8),
    (17, 15, [(40, ID), (24, ID)], 128, False, False, 8),
    (4, 14, [(64, ID), (64, ID)], 128, True, False, 8),
    (2, 30, [(40, ID), (75, ID)], 128, True, False, 8),
    (5, 15, [(128, ID), (75, ID)], 128, False, False, 8),
]


@pytest.mark.parametrize('case', CASES, ids=['%dx%d-k%s%s' % (c[0], c[1], '+'.join(str(s[0]) for s in c[2]), '-pre' if c[4] else '-gated' if c[5] else '') for c in CASES])
def test_shared_row(dev, case):
    h, w, segs, f, pre, gated, r = case
    assert walk_ok(segs, f, pre, gated, 'relu6') and sum((c + 31) // 32 for c, _ in segs) >= 2
    rng = np.random.default_rng(1000 * h + w)
    run_head(dev, rng, 3, h, w, segs, f, pre=pre, gated=gated, se=r, form='walk')


def test_shared_row_twice_on_the_same_buffers(dev, monkeypatch):
    """two launches of one op on the same buffers: map, sums and gate bit-equal (a row left in LDS, or planes read before the
    barrier, would differ from launch to launch)"""
    h, w, segs, f, pre, gated, r = CASES[2]
    snaps = []
    run_op = fence.run_op

    def run_and_keep(op, batch, writes, **kw):
        run_op(op, batch, writes=writes, **kw)
        torch.cuda.synchronize()
        snaps.append([t.clone() for t in writes[:3]])      # map, sums, gate

    monkeypatch.setattr(fence, 'run_op', run_and_keep)
    run_head(dev, np.random.default_rng(3), 3, h, w, segs, f, gated=gated, se=r, form='walk')
    assert len(snaps) == 2
    for a, b in zip(*snaps):
        assert torch.equal(a[..., :f].view(torch.int32), b[..., :f].view(torch.int32))
