"""yr_nms at every edge of the band kernel's three instantiations (256 lanes x 44 score slots up to 11 264 boxes, 512 x 50 up to
25 600, 1024 x 38 up to 38 400) against the C oracle: indices and counts bit for bit.

The band kernel keeps, per score slot, the score's histogram bin (16 bits; a sentinel for "not a candidate") and reads the score
itself again only for the members of a band.  What can go wrong with that is tested here: the last slot of the last lane (N at the
edge of an instantiation), a lane whose every slot is live and several bands deep, no candidate at all, scores AT the threshold
(not candidates), the top bin (score 1.0) and bin 0 (just above the threshold) next to the sentinel, runs of exact ties (the index
decides inside a bin) and one bin with more equal scores than a band holds (the second, problem-walking launch takes the problem).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cpost

pytestmark = pytest.mark.gpu

B, C, MAX_BOXES = 2, 3, 20
THR = np.float32(0.2)
IOU = 0.5
NS = [300, 11264, 11265, 25600, 25601, 38400]
CASES = ['all_live', 'none', 'at_threshold', 'top_and_bottom_bin', 'ties', 'overflow']


@functools.lru_cache(maxsize=None)
def _boxes(n):
    rng = np.random.default_rng(n)
    size = 416.0
    cy, cx = rng.uniform(0, size, (B, n)), rng.uniform(0, size, (B, n))
    h, w = rng.uniform(2, size / 2, (B, n)), rng.uniform(2, size / 2, (B, n))
    b = np.clip(np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 2), 0, size).astype(np.float32)
    return b


def _scores(case, n):
    rng = np.random.default_rng(CASES.index(case) * 100003 + n)
    above = np.nextafter(THR, np.float32(1))                  # the lowest candidate score: bin 0
    u = rng.random((B, C, n), dtype=np.float32)
    if case == 'all_live':                                    # every slot of every lane holds a candidate
        s = np.maximum(THR + np.float32(0.8) * u, above)
    elif case == 'none':                                      # below and AT the threshold
        s = np.minimum(THR * u * np.float32(1.25), THR)
    elif case == 'at_threshold':                              # every third score is the threshold itself
        s = u.copy()
        s[..., ::3] = THR
    elif case == 'top_and_bottom_bin':                        # 1.0 (bin 2047), the first float above the threshold (bin 0), the last slot
        s = THR * u
        at = rng.choice(n - 1, 80, replace=False)
        s[..., at[:40]] = 1.0
        s[..., at[40:]] = above
        s[..., n - 1] = 1.0
        s[:, 1, n - 1] = above
    elif case == 'ties':                                      # 52 distinct candidate scores: runs of equal scores in one bin
        s = np.round(u * 64) / np.float32(64)
    elif case == 'overflow':                                  # the top-scoring bin holds more equal scores than the widest band (1024)
        s = np.float32(0.9) * u
        k = min(n, 1100)
        at = np.sort(rng.choice(n, k, replace=False))
        s[..., at] = 0.9375
    return np.minimum(s, np.float32(1)).astype(np.float32)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('n', NS)
def test_band_kernel_picks_equal_the_c_oracle(dev, n, case):
    from yoloret_amd import runtime as rt
    boxes, scores = _boxes(n), _scores(case, n)               # (the boxes of a size are shared: nothing below writes to them)
    if case == 'all_live':
        assert (scores > THR).all()
    elif case == 'none':
        assert not (scores > THR).any() and (scores == THR).any()
    elif case == 'overflow':
        assert ((scores == np.float32(0.9375)).sum(axis=2) > min(n, 1024) - 1).all()
    idx, cnt = rt.nms(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), MAX_BOXES, float(THR), IOU)
    torch.cuda.synchronize()
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    for i in range(B):
        for k in range(C):
            ref = cpost.nms(boxes[i], scores[i, k], MAX_BOXES, IOU, float(THR))
            assert cnt[i, k] == len(ref), (n, case, i, k, int(cnt[i, k]), len(ref))
            assert np.array_equal(idx[i, k, :len(ref)], ref), (n, case, i, k)
            assert (idx[i, k, len(ref):] == -1).all()
