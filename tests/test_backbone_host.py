"""Host side of the MobileNetV2 backbone operators (no GPU): the torch restatement of tests/backbone_ref.py against the NumPy oracle, the
parameter layouts and their way back, the refusals, and the committed seeds against THE SEED RULE."""
import numpy as np
import pytest
import torch

from oracle import model as om, params
from tests import backbone_ref as br, layers_ref as lr
from tests.util import ANCHORS


def _net():
    return lr.product_net(br.MODEL, br.values())


def test_restatement_chained_is_the_oracles_backbone():
    """the 17 units of ``torch_unit`` in float64, chained in inference mode on the oracle's images, give the oracle's taps"""
    host = br.host_parameters(br.values())
    x = params.synthetic_images(lr.BATCH, lr.RFCR_HW[0], lr.RFCR_HW[1]).astype(np.float64)
    _, taps64 = br.oracle_taps()
    t, outs = x, {}
    for unit in br.UNITS:
        t = br.torch_unit(host, unit, t, 'float64')['y']
        outs[unit] = t
    from oracle import nn
    got = [outs[15], outs[12], outs[5], nn.maxpool(outs[2], 4)]
    for g, w in zip(got, taps64):
        assert g.shape == w.shape and np.abs(g - w).max() <= 1e-11 * max(1.0, np.abs(w).max())
    assert br.STRIDES == tuple(s for _, s, _ in om.MBV2_BLOCKS[:16])


def test_parameters_and_their_way_back():
    from yoloret_amd import autograd as ag
    net = _net()
    par = ag.detector_parameters(net, 'cpu')
    host = br.host_parameters(br.values())
    b = par['backbone']
    assert sorted(k for k in b if k != 'cin') == sorted(host)
    for k, v in host.items():
        assert tuple(b[k].shape) == v.shape and np.array_equal(b[k].detach().numpy(), v), k
        assert b[k].requires_grad == (not br.is_moving(k)), k
    assert b['cin']['block_13_expand'] == host['block_12_project'].shape[0] and 'expanded_conv_expand' not in b
    assert (ag.MBV2_STRIDES, ag.MBV2_BN_MOMENTUM, ag.MBV2_BN_EPS) == (br.STRIDES, br.BN_MOMENTUM, br.BN_EPS)
    back, have = ag.detector_weights(par), net.get_weights()
    assert set(back) == set(have) and len(have) == 392
    for k, v in have.items():
        assert back[k].shape == tuple(np.shape(v)) and np.array_equal(back[k], np.asarray(v, np.float32)), k
    assert set(ag.backbone_weights(b)) | set(ag.neck_weights(par['neck'])) == set(have)


def test_refusals_name_what_is_missing():
    from yoloret_amd import autograd as ag, layers as L
    from yoloret_amd.yolo3.model import yolov3_body
    from yoloret_amd.yolo3.train import DetectorTrainer
    eff = lr.product_net('efficientnetb0', lr.rfcr_case('efficientnetb0')['P'].values)
    for call in (lambda: ag.mobilenetv2_parameters(eff, 'cpu'), lambda: DetectorTrainer(eff, ANCHORS, lr.CLASSES, 3)):
        with pytest.raises(ValueError, match='Conv1/kernel'):
            call()
    bare = yolov3_body(L.Input(shape=[96, 96, 3]), br.MODEL, 3, num_classes=lr.CLASSES)
    for call in (lambda: ag.mobilenetv2_parameters(bare, 'cpu'), lambda: DetectorTrainer(bare, ANCHORS, lr.CLASSES, 3)):
        with pytest.raises(ValueError, match='no weights'):
            call()
    trainer = DetectorTrainer(_net(), ANCHORS, lr.CLASSES, 3)
    for kw in (dict(use_ema=True), dict(use_adv=True)):
        with pytest.raises(NotImplementedError):
            trainer.fit(1, [], **kw)
    with pytest.raises(ValueError, match='0..15'):
        ag.mobilenetv2_block(torch.zeros(1, 2, 2, 3), {}, 16)


def test_committed_seeds_hold_the_rule():
    """per case the committed seed clears ``relu6_margins``' bar at every ReLU6 input and no smaller seed does; on one torch thread, as
    the margins move by a few percent with the number of threads torch sums with"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        host = br.host_parameters(br.values())
        assert len(br.cases()) == 2 * (2 * 5 + 12) and set(br.SEEDS) <= {br.case_id(c) for c in br.cases()}
        for case in br.cases():
            seed = br.case_seed(case)
            ok, m = br.rule_holds(host, case, seed)
            assert ok, (br.case_id(case), m)
            assert len(m) == (1 if case[0] == 'stem' else 1 if case[0] == 0 else 2)
            assert br.first_seed(host, case, seed + 1) == seed, 'the FIRST seed that holds the rule'
    finally:
        torch.set_num_threads(threads)
