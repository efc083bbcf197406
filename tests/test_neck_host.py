"""What tests/test_gpu_neck.py and tests/test_gpu_conv1x1_autograd.py rest on, without a device: the restatements of tests/neck_ref.py
against the oracle's own body, ``autograd.neck_weights`` as the inverse of ``autograd.neck_parameters``, and the margins of the
gradient cases."""
import numpy as np
import pytest
import torch

from oracle import model as om, params
from tests import headtrain_ref as href, layers_ref as lr, neck_ref as nr, selayers_ref as sl


@pytest.mark.parametrize('model_name', nr.MODELS)
def test_restatements_are_the_oracles_body(model_name):
    """on the oracle's float32 taps the NumPy restatement gives oracle.model.yolov3_body's logits bit for bit; the torch restatement on the
    parameters in the operators' layouts agrees with it in float64"""
    case = lr.rfcr_case(model_name)
    P = case['P']
    want = om.yolov3_body(P, params.synthetic_images(lr.BATCH, lr.RFCR_HW[0], lr.RFCR_HW[1]), model_name, nr.ANCHORS, lr.CLASSES)
    got = nr.numpy_neck(P, case['taps'], np.float32)
    assert [g.shape for g in got] == [(lr.BATCH, s, s, 3, 25) for s in (3, 6, 12)]
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    n64 = nr.numpy_neck(P, case['taps'], np.float64)
    t64 = nr.torch_neck(nr.host_parameters(P.values), case['taps'], 'float64')
    for a, b in zip(t64['y'], n64):
        assert a.dtype == np.float64 and href.rel_err(a, b) < 1e-12
    assert len(t64['relu6']) == 2 + 6 + 4 and len(t64['smooth']) == 3 * 6


@pytest.mark.parametrize('model_name', nr.MODELS)
def test_neck_weights_inverts_neck_parameters(model_name):
    from yoloret_amd import autograd as ag
    values = lr.rfcr_case(model_name)['P'].values
    net = lr.product_net(model_name, values)
    par = ag.neck_parameters(net, 'cpu')
    assert sorted(k for k in par) == sorted(('rfcr', 'cin') + nr.HEADS + nr.LINKS)
    host = nr.host_parameters(values)
    for group, d in host.items():      # the layouts are the documented ones
        assert sorted(k for k in par[group] if k != 'name') == sorted(d), group
        for k, v in d.items():
            t = par[group][k]
            assert np.array_equal(t.detach().numpy().view(np.uint32), v.view(np.uint32)), (group, k)
            assert t.requires_grad == (not nr.is_moving(k)), (group, k)
    back = ag.neck_weights(par)
    model = net.get_weights()
    behind = [k for k in model if k.startswith(('rfcr_', 'td', 'bu', 'block_20_', 'block_24_'))]
    assert sorted(back) == sorted(behind) and len(back) == 152
    for k, v in back.items():
        assert v.dtype == np.float32 and v.shape == model[k].shape and np.array_equal(v.view(np.uint32), model[k].view(np.uint32)), k
    w = net.get_weights()
    w.update(back)
    net.set_weights(w)      # what is trained is what is shipped


def _assert_margins(what, host, taps, training):
    # the float32 run's deviation - the margin - moves by a few percent with the number of threads torch sums with; the seeds are chosen,
    # and held here, on one thread, so that the same bits decide on every host
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r64, r32 = nr.torch_neck(host, taps, 'float64', training), nr.torch_neck(host, taps, 'float32', training)
    finally:
        torch.set_num_threads(threads)
    ms, big = nr.margins(r64, r32)
    assert len(ms) == 12
    for where, distance, margin in ms:
        print('%s %s: smallest distance %.3e, margin %.3e' % (what, where, distance, margin))
        assert distance > margin, 'a kink lies too close - choose another seed'
    print('%s: largest |u| before a Swish or sigmoid %.2f' % (what, big))
    assert big < 87.0


@pytest.mark.parametrize('model_name', nr.MODELS)
def test_gradient_cases_rest_on_their_margins(model_name):
    host = nr.host_parameters(lr.rfcr_case(model_name)['P'].values)
    taps, fs = nr.seeded_taps(model_name, nr.GRAD_SEEDS[model_name])
    _assert_margins(model_name + ' inference', host, taps, False)
    g = nr.torch_neck(host, taps, 'float64', False, fs)
    assert all(np.abs(t).max() > 0 for t in g['taps']) and all(np.abs(v).max() > 0 for v in g['grads'].values())
    assert not any(nr.is_bn_affine(k) or nr.is_moving(k) for _, k in g['grads'])


def test_training_case_rests_on_its_margins():
    host = nr.host_parameters(lr.rfcr_case(nr.TRAIN_MODEL)['P'].values)
    taps, fs = nr.seeded_taps(nr.TRAIN_MODEL, nr.TRAIN_SEED)
    _assert_margins(nr.TRAIN_MODEL + ' training', host, taps, True)
    g = nr.torch_neck(host, taps, 'float64', True, fs)
    assert len(g['stats']) == 24 and sum(1 for _, k in g['grads'] if nr.is_bn_affine(k)) == 48
    assert sorted({n for _, _, n in g['stats'].values()}) == [lr.BATCH * s * s for s in (3, 6, 12)]


def test_td1_case_rests_on_its_margins():
    model_name, name, cin, f, _ = nr.TD1_CASE
    P = lr.rfcr_case(model_name)['P']
    assert P.values['td1_conv/kernel'].shape == (1, 1, cin, f)
    x, _ = nr.td1_inputs()
    us64 = sl.preacts(P, name + '_mb', x, 3, 1, 1, f, np.float64, conv=(name + '_conv', f))
    us32 = sl.preacts(P, name + '_mb', x, 3, 1, 1, f, np.float32, conv=(name + '_conv', f))
    assert [w.split(' ')[0] for w, _ in us64] == ['ReLU6', 'Swish', 'Swish', 'sigmoid']
    for where, distance, margin in lr.relu6_margins([(w.split(' of ')[1], u) for w, u in us64[:1]], [(w.split(' of ')[1], u) for w, u in us32[:1]]):
        print('td1 %s: smallest distance %.3e, margin %.3e' % (where, distance, margin))
        assert distance > margin, 'a kink lies too close - choose another seed'
    assert max(float(np.abs(u).max()) for _, u in us64[1:]) < 87.0
