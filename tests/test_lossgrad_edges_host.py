"""Host side of tests/test_gpu_lossgrad_edges.py (no GPU): what makes tests/lossgrad_ref.py valid AT ties of Maximum / Minimum -
away from ties its selects give the bits of the torch.maximum / torch.minimum formulation, hand-derived answers hold at ties,
and the tie cases are ties in float32 and float64 alike -, and the conditions the random cases of the GPU file depend on: no
kink within 1e-5, and the number of listed boxes each chunk case is built for."""
import numpy as np
import pytest
import torch

from tests import loss_ref, lossgrad_ref
from tests.util import ANCHORS

R = {name: k for k, (name, _, _) in enumerate(lossgrad_ref.TIE_RELATIONS)}


# ----------------------------------------------------------------------------- selects == torch.maximum / torch.minimum away from ties
def _giou_parts_split_ties(b1, b2):
    """lossgrad_ref._giou_parts as it was before the selects: torch.maximum / torch.minimum, which split a tie evenly.  Kept
    for this comparison only."""
    zero = torch.zeros((), dtype=b1.dtype)
    b1_ymin, b1_xmin, b1_ymax, b1_xmax = b1.unbind(-1)
    b2_ymin, b2_xmin, b2_ymax, b2_xmax = b2.unbind(-1)
    b1_area = torch.maximum(zero, b1_xmax - b1_xmin) * torch.maximum(zero, b1_ymax - b1_ymin)
    b2_area = torch.maximum(zero, b2_xmax - b2_xmin) * torch.maximum(zero, b2_ymax - b2_ymin)
    raw_w = torch.minimum(b1_xmax, b2_xmax) - torch.maximum(b1_xmin, b2_xmin)
    raw_h = torch.minimum(b1_ymax, b2_ymax) - torch.maximum(b1_ymin, b2_ymin)
    inter = torch.maximum(zero, raw_w) * torch.maximum(zero, raw_h)
    union = b1_area + b2_area - inter
    iou = lossgrad_ref._div_no_nan(inter, union)
    enc_w = torch.maximum(zero, torch.maximum(b1_xmax, b2_xmax) - torch.minimum(b1_xmin, b2_xmin))
    enc_h = torch.maximum(zero, torch.maximum(b1_ymax, b2_ymax) - torch.minimum(b1_ymin, b2_ymin))
    enclose = enc_w * enc_h
    return {'iou': iou, 'giou': iou - lossgrad_ref._div_no_nan(enclose - union, enclose), 'raw_w': raw_w, 'raw_h': raw_h}


def _old_and_new(monkeypatch, y_true, logits, an, step, dtype):
    res, new = lossgrad_ref.loss_and_grad(y_true, logits, an, step, dtype=dtype)
    with monkeypatch.context() as mp:
        mp.setattr(lossgrad_ref, '_giou_parts', _giou_parts_split_ties)
        res_old, old = lossgrad_ref.loss_and_grad(y_true, logits, an, step, dtype=dtype)
    return res, new, res_old, old


def test_selects_give_the_bits_of_maximum_and_minimum_away_from_ties(monkeypatch):
    cases = lossgrad_ref.parity_cases() + [('disjoint scale %d' % s, s, l, y) for s, (l, y) in lossgrad_ref.disjoint_case().items()]
    for name, s, logits, y_true in cases:
        an, step = loss_ref.scale_anchors(ANCHORS, s), loss_ref.GRID_STEPS[s]
        for dtype in (np.float64, np.float32) if logits.size < 100000 else (np.float64,):      # (float32 too where it is cheap)
            res, new, res_old, old = _old_and_new(monkeypatch, y_true, logits, an, step, dtype)
            assert new.tobytes() == old.tobytes(), '%s %s: the gradients differ by %r' % (name, dtype.__name__, np.abs(new - old).max())
            for k in ('loss', 'giou', 'conf', 'cls', 'ignore_sum'):
                assert res[k] == res_old[k], (name, k)


def test_selects_differ_from_maximum_and_minimum_at_ties(monkeypatch):
    """(the comparison above is not vacuous) the cell whose label contains the prediction and shares its start on x: -1/3
    against the -5/18 of evenly split ties."""
    _, logits, y_true, an, step = lossgrad_ref.tie_grid_case()
    _, new, _, old = _old_and_new(monkeypatch, y_true, logits, an, step, np.float64)
    cell = (0, R['equal'], R['containing, shared start'], 0)
    print('shared start: select %r, torch.maximum %r' % (new[cell][0], old[cell][0]))
    assert new[cell][0] == pytest.approx(-1 / 3, rel=1e-12) and old[cell][0] == pytest.approx(-5 / 18, rel=1e-12)


# ----------------------------------------------------------------------------- hand-derived answers at ties
def test_known_answers_at_ties():
    """The derivations are in tests/lossgrad_ref.py (KNOWN_TIE_ANSWERS); in float64 they hold to 1e-12."""
    for (name, logits, y_true, an, step), (j, i), want in lossgrad_ref.known_tie_answers():
        _, g = lossgrad_ref.loss_and_grad(y_true, logits, an, step)
        row = g[0, j, i, 0]
        print('%s cell (%d, %d): %r' % (name, j, i, row))
        assert np.all(np.abs(row[:4] - want) <= 1e-12 * np.maximum(1, np.abs(want))), (name, j, i, row, want)
        assert row[4] == -0.5 and row[5] == -0.5


def test_tie_cases_are_ties_in_both_precisions():
    """pred_box and true_box of the float32 run equal those of the float64 run exactly after widening."""
    for name, logits, y_true, an, step in (lossgrad_ref.tie_grid_case(), lossgrad_ref.zero_size_case(), lossgrad_ref.threshold_case()):
        r64, _ = lossgrad_ref.loss_and_grad(y_true, logits, an, step, dtype=np.float64)
        r32, _ = lossgrad_ref.loss_and_grad(y_true, logits, an, step, dtype=np.float32)
        for k in ('pred_box', 'true_box', 'raw_w', 'raw_h'):
            assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64
            assert np.array_equal(r32[k].astype(np.float64), r64[k]), '%s: %s differs between float32 and float64' % (name, k)
        assert np.array_equal(r32['ignore_mask'], r64['ignore_mask']) and r32['ignore_sum'] == r64['ignore_sum'], name


def test_tie_grid_holds_every_pair_of_relations():
    name, logits, y_true, an, step = lossgrad_ref.tie_grid_case()
    assert logits.shape == (1, 16, 16, 1, 6) and int((y_true[..., 4] != 0).sum()) == 169 and len(lossgrad_ref.TIE_RELATIONS) == 13
    res, _ = lossgrad_ref.loss_and_grad(y_true, logits, an, step)
    u = lossgrad_ref.TIE_UNIT
    for j, (_, ylo, yhi) in enumerate(lossgrad_ref.TIE_RELATIONS):
        for i, (_, xlo, xhi) in enumerate(lossgrad_ref.TIE_RELATIONS):
            p, t = res['pred_box'][0, j, i, 0], res['true_box'][0, j, i, 0]
            assert np.array_equal(p, np.array([16 * j + 4, 16 * i + 4, 16 * j + 12, 16 * i + 12]) * u)
            assert np.array_equal(t - p[[0, 1, 0, 1]], np.array([ylo, xlo, yhi, xhi]) * u)
    # the relations are the 13 of two intervals: every sign pattern of (lo - 0, lo - 8, hi - 0, hi - 8) with lo < hi, once
    signs = {tuple(int(np.sign(v)) for v in (lo, lo - 8, hi, hi - 8)) for _, lo, hi in lossgrad_ref.TIE_RELATIONS}
    assert len(signs) == 13 and all(lo < hi for _, lo, hi in lossgrad_ref.TIE_RELATIONS)


def test_zero_size_case():
    name, logits, y_true, an, step = lossgrad_ref.zero_size_case()
    obj = y_true[..., 4] != 0
    assert int(obj.sum()) == 20
    assert np.all(y_true[0, 0, :5, 0, 2] == 0) and np.all(y_true[0, 0, :5, 0, 3] > 0)
    assert np.all(y_true[0, 1, :5, 0, 3] == 0) and np.all(y_true[0, 1, :5, 0, 2] > 0)
    assert np.all(y_true[0, 2:4, :5, 0, 2:4] == 0)
    res, g = lossgrad_ref.loss_and_grad(y_true, logits, an, step)
    assert np.isfinite(g).all() and np.abs(g[obj][:, :4]).max() > 0


def test_threshold_on_the_last_bit():
    """IoU of P with the label is 0.5 exactly: `best_iou < 0.5` is false (P drops out of the confidence term, gradient 0), and
    true for the next float32 above 0.5 (P is background: gradient sigmoid(0) - 0 = 0.5, one more cell counted)."""
    name, logits, y_true, an, step = lossgrad_ref.threshold_case()
    P, Q = lossgrad_ref.THRESHOLD_P, lossgrad_ref.THRESHOLD_Q
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    for dtype in (np.float64, np.float32):
        res, g = lossgrad_ref.loss_and_grad(y_true, logits, an, step, .5, dtype)
        assert res['best_iou'][0, P[0], P[1], 0] == 0.5 and res['best_iou'][0, Q[0], Q[1], 0] == 0
        best = res['best_iou'].copy()
        best[0, P[0], P[1], 0] = 0
        assert np.all(best == 0)
        assert g[0, P[0], P[1], 0, 4] == 0 and res['ignore_sum'] == 255
        res, g = lossgrad_ref.loss_and_grad(y_true, logits, an, step, above, dtype)
        assert g[0, P[0], P[1], 0, 4] == 0.5 and res['ignore_sum'] == 256


# ----------------------------------------------------------------------------- the random cases keep clear of every kink
def _assert_margins(case):
    name, logits, y_true, an, step = case
    m = lossgrad_ref.margins_of(logits, y_true, an, step)
    n = int((y_true[..., 4] != 0).sum())
    print('%-30s %4d boxes, margins: threshold %.2e, coordinates %.2e, intersection sides %.2e' % ((name, n) + m))
    assert min(m) > 1e-5, '%s: %r' % (name, m)
    return n


def test_chunk_cases_span_chunks_and_keep_clear_of_kinks():
    want = {'chunks B=2 seed 0': 332, 'chunks B=2 seed 1': 338, 'chunks B=2 seed 2': 342, 'chunks B=4 seed 0': 663,
            'chunks B=2 seed 0 cut to 257': 257, 'chunks B=2 seed 0 cut to 256': 256}
    cases = [lossgrad_ref.chunk_case(name) for name in lossgrad_ref.CHUNK_RECIPES]
    assert [c[0] for c in cases] == list(want)
    for case in cases:
        assert case[1].shape[1:] == (8, 12, 3, 8)
        assert _assert_margins(case) == want[case[0]]
    full, cut257, cut256 = cases[0][2], cases[4][2], cases[5][2]
    # the cut cases are the full one with the LAST object rows (raster order) cleared, and nothing else touched
    flat = lambda y: y.reshape(-1, y.shape[-1])
    idx = np.flatnonzero(flat(full)[:, 4] != 0)
    for cut, keep in ((cut257, 257), (cut256, 256)):
        assert np.array_equal(np.flatnonzero(flat(cut)[:, 4] != 0), idx[:keep])
        assert np.all(flat(cut)[idx[keep:]] == 0)
        rest = np.ones(len(flat(full)), bool)
        rest[idx[keep:]] = False
        assert np.array_equal(flat(cut)[rest], flat(full)[rest])


def test_edge_cases_have_their_shapes_and_keep_clear_of_kinks():
    shapes = {'row of 5 (C=0)': (2, 2, 3, 3, 5), 'row of 256 (C=251)': (2, 2, 3, 3, 256), 'row of 257 (C=252)': (2, 2, 3, 3, 257),
              'row of 305 (C=300)': (2, 2, 3, 3, 305), 'A=1': (2, 2, 3, 1, 25), 'A=2': (2, 2, 3, 2, 25), 'A=5': (2, 2, 3, 5, 25),
              'A=8': (2, 2, 3, 8, 25), 'total 3 (grid 1x1)': (1, 1, 1, 3, 25), 'total 256 (grid 8x8, A=4)': (1, 8, 8, 4, 25),
              'object flag 0.5': (2, 2, 3, 3, 25)}
    cases = [lossgrad_ref.edge_case(name) for name in lossgrad_ref.EDGE_RECIPES]
    assert [c[0] for c in cases] == list(shapes)
    for case in cases:
        name, logits, y_true, an, step = case
        assert logits.shape == shapes[name] and y_true.shape == shapes[name] and step == 32
        assert np.array_equal(an, ANCHORS[:logits.shape[3]])
        assert _assert_margins(case) >= 1
    assert np.prod(shapes['total 256 (grid 8x8, A=4)'][:4]) == 256
    flags = lossgrad_ref.edge_case('object flag 0.5')[2][..., 4]
    assert (flags == 0.5).sum() >= 1 and (flags == 1).sum() >= 1 and abs(int((flags == 0.5).sum()) - int((flags == 1).sum())) <= 1


def test_random_case_defaults_keep_their_bytes():
    """The defaulted arguments of loss_ref.random_case change nothing for the existing calls: naming scale 0's own anchors
    gives the case the default gives (same draws in the same order)."""
    a = loss_ref.random_case(7, 2, (64, 96), 20, ANCHORS, scales=(0,))[0]
    b = loss_ref.random_case(7, 2, (64, 96), 20, None, scales=(0,), slot_anchors=loss_ref.scale_anchors(ANCHORS, 0))[0]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # and a default case keeps the SHA-256 it has with loss_ref.random_case as of the commit before the argument existed
    # (computed from that commit's tests/loss_ref.py): a later change of the recipe's draws shows here
    import hashlib
    logits, y_true = loss_ref.random_case(0, 2, (64, 96), 80, ANCHORS)[2]
    assert hashlib.sha256(logits.tobytes() + y_true.tobytes()).hexdigest() == RANDOM_CASE_DIGEST


RANDOM_CASE_DIGEST = 'f0f37a4238126f1ec5fe1e4cac403f57b6b4910f8c5516ac45b5860e46b5b9ff'


def test_yolo_head_of_the_reference_with_other_slot_counts():
    """loss_ref.yolo_head against the scalar formulas of model.py:363-366 for A = 1, 2, 5, 8: slot k uses anchor k."""
    rs = np.random.RandomState(11)
    for a in (1, 2, 5, 8):
        feats = rs.randn(2, 2, 3, a, 7)
        an = ANCHORS[:a]
        _, xy, wh, conf = loss_ref.yolo_head(feats, an, (64, 96))
        assert xy.shape == (2, 2, 3, a, 2) and wh.shape == (2, 2, 3, a, 2) and conf.shape == (2, 2, 3, a, 1)
        for b, j, i, k in [(0, 0, 0, 0), (1, 1, 2, a - 1), (0, 1, 1, a // 2)]:
            f = feats[b, j, i, k]
            sig = lambda v: 1 / (1 + np.exp(-v))
            assert xy[b, j, i, k, 0] == pytest.approx((sig(f[0]) + i) / 3, rel=1e-14) and xy[b, j, i, k, 1] == pytest.approx((sig(f[1]) + j) / 2, rel=1e-14)
            assert wh[b, j, i, k, 0] == pytest.approx(np.exp(f[2]) * float(an[k, 0]) / 96, rel=1e-14)
            assert wh[b, j, i, k, 1] == pytest.approx(np.exp(f[3]) * float(an[k, 1]) / 64, rel=1e-14)
        # and the torch restatement decodes the same boxes
        y = np.zeros_like(feats)
        res, _ = lossgrad_ref.loss_and_grad(y, feats, an, 32)
        want = np.concatenate([(xy - wh / 2)[..., ::-1], (xy + wh / 2)[..., ::-1]], -1)
        assert np.allclose(res['pred_box'], want, rtol=0, atol=1e-14)      # (coordinates of order 1)
