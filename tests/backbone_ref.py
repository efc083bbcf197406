"""The MobileNetV2 backbone of ``autograd.mobilenetv2_backbone`` unit by unit - the stem (Conv1 -> BN -> ReLU6) and the 16 inverted-residual
blocks - restated on torch: what tests/test_backbone_host.py (CPU) and tests/test_gpu_backbone.py (device) share.  Test code; oracle/ is
untouched.

* ``host_parameters``: ``ParamStore.values`` -> the dictionary of ``autograd.mobilenetv2_parameters`` as float32 host arrays, written from
  that function's documentation with ``layers_ref``'s converters;
* ``torch_unit``: one unit on torch in float64 or float32, NHWC, on the primitives tests/convgrad_ref.py and tests/neck_ref.py use
  (torch.nn.functional.conv2d, the same call oracle.torch_ref._Net makes); inference mode (BatchNorms folded in the working dtype) or
  training mode (``bntrain_ref._forward64``: the statistics of the batch), with the gradients of (y * f).sum();
* the cases: MobileNetV2 x0.75 with the weights of ``layers_ref.rfcr_case``, 2 images, the stride-2 units on 8 x 6 and 7 x 5 maps (both
  classes of 'same' padding at stride 2 in rows and columns), the others on 6 x 5; standard-normal inputs of a committed seed;
* THE SEED RULE: per unit, map and mode the first seed of 0, 1, 2, .. whose float64 run keeps every ReLU6 input farther from 0 and from
  6 than ``layers_ref.relu6_margins``' bar, 8 x the float32 run's largest deviation at that tensor.  tests/test_backbone_host.py
  asserts the rule on one torch thread.  Chosen by that rule, never by what the device computes.
* the whole backbone: ``oracle_taps`` are the NumPy oracle's four taps on ``layers_ref.rfcr_case``'s images in float32 and float64."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import model as om, params
from tests import bntrain_ref, convgrad_ref as cref, layers_ref as lr

MODEL = 'mobilenetv2x75'
STRIDES = (1, 2, 1, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1, 2, 1, 1)      # oracle/model.py:53-57, blocks 0..15
UNITS = ('stem',) + tuple(range(16))
BN_MOMENTUM, BN_EPS = 0.9, 1e-3
_shared = {}


def prefix(block):
    return 'expanded_conv_' if block == 0 else 'block_%d_' % block


def unit_stride(unit):
    return 2 if unit == 'stem' else STRIDES[unit]


def unit_maps(unit):
    return ((8, 6), (7, 5)) if unit_stride(unit) == 2 else ((6, 5),)


def cases():
    """[(unit, (h, w), training)]"""
    return [(u, hw, t) for u in UNITS for hw in unit_maps(u) for t in (False, True)]


def case_id(case):
    return '%s-%dx%d-%s' % (case[0], case[1][0], case[1][1], 'training' if case[2] else 'inference')


# the first seed that holds THE SEED RULE, per case (tests/test_backbone_host.py asserts each)
# every case not listed here has seed 0
SEEDS = {'8-6x5-inference': 1, '8-6x5-training': 2, '10-6x5-inference': 1, '12-6x5-training': 3, '13-8x6-inference': 2, '14-6x5-inference': 7,
         '14-6x5-training': 3, '15-6x5-inference': 2, '15-6x5-training': 1}


def case_seed(case):
    return SEEDS.get(case_id(case), 0)


def values():
    return lr.rfcr_case(MODEL)['P'].values


def host_parameters(vals):
    def bn(out, name):
        for p in lr.BN_PARTS:
            out['%s/%s' % (name, p)] = np.asarray(vals['%s/%s' % (name, p)], np.float32).reshape(-1)
    k = np.asarray(vals['Conv1/kernel'], np.float32)
    out = {'Conv1': np.ascontiguousarray(k.reshape(9 * k.shape[2], k.shape[3]))}
    bn(out, 'bn_Conv1')
    for b in range(16):
        p = prefix(b)
        if b > 0:
            out[p + 'expand'] = lr.pack_conv(vals[p + 'expand/kernel'])
            bn(out, p + 'expand_BN')
        out[p + 'depthwise'] = lr.pack_dw(vals[p + 'depthwise/depthwise_kernel'])
        bn(out, p + 'depthwise_BN')
        out[p + 'project'] = lr.pack_conv(vals[p + 'project/kernel'])
        bn(out, p + 'project_BN')
    return out


def unit_keys(host, unit):
    """the keys of ``host`` that unit reads"""
    if unit == 'stem':
        return [k for k in host if k == 'Conv1' or k.startswith('bn_Conv1/')]
    return [k for k in host if k.startswith(prefix(unit))]


def _cin_of(host, unit):
    """input channels of block ``unit`` > 0: the output channels of the unit before it"""
    return host[prefix(unit - 1) + 'project'].shape[0]


def unit_cout(host, unit):
    return host['Conv1'].shape[1] if unit == 'stem' else host[prefix(unit) + 'project'].shape[0]


def is_moving(key):
    return key.endswith(('/moving_mean', '/moving_variance'))


def is_bn_affine(key):
    return key.endswith(('/gamma', '/beta'))


def trained_keys(host, unit, training):
    return [k for k in unit_keys(host, unit) if not is_moving(k) and (training or not is_bn_affine(k))]


def unit_inputs(host, unit, hw, seed):
    """-> (x [2, h, w, cin], f [2, oh, ow, cout]) float32 standard normals"""
    s = unit_stride(unit)
    rng = np.random.default_rng([seed, UNITS.index(unit), hw[0], hw[1]])
    cin = 3 if unit == 'stem' else (host[prefix(0) + 'depthwise'].shape[1] if unit == 0 else _cin_of(host, unit))
    x = rng.standard_normal((lr.BATCH, hw[0], hw[1], cin)).astype(np.float32)
    f = rng.standard_normal((lr.BATCH, -(-hw[0] // s), -(-hw[1] // s), unit_cout(host, unit))).astype(np.float32)
    return x, f


def torch_unit(host, unit, x, dtype, training=False, f=None):
    """-> {'y': NHWC array, 'relu6': [(what, u)], 'stats': {bn: (mean, biased variance, N)} (training)}; with f also 'x': the gradient of
    (y * f).sum() for the input and 'grads': {key: gradient in the parameter's layout} for ``trained_keys``"""
    dt = cref.DT[dtype]
    need = f is not None
    want = set(trained_keys(host, unit, training))
    p = {k: torch.tensor(np.asarray(host[k], np.float64), dtype=dt, requires_grad=need and k in want) for k in unit_keys(host, unit)}
    xt = torch.tensor(np.asarray(x, np.float64), dtype=dt, requires_grad=need)
    relu6, stats = [], {}

    def lin(t, w):
        cin = t.shape[-1]
        return cref._linear(t.reshape(-1, cin), w[:, :cin]).reshape(tuple(t.shape[:-1]) + (w.shape[0],))

    def bn(z, name, act):
        if training:
            u = bntrain_ref._forward64(z.reshape(-1, z.shape[-1]), p[name + '/gamma'], p[name + '/beta'], BN_EPS)
            stats[name] = (u[2].detach().numpy(), u[3].detach().numpy(), u[0].shape[0])
            u = u[0].reshape(z.shape)
        else:
            scale = p[name + '/gamma'] / torch.sqrt(p[name + '/moving_variance'] + BN_EPS)
            u = z * scale + (p[name + '/beta'] - p[name + '/moving_mean'] * scale)
        if act == 'relu6':
            relu6.append(('ReLU6 of ' + name, u.detach().numpy()))
        return cref._act(u, act)

    def same(t, k, stride):
        pads, _ = cref.geometry(t.shape[1], t.shape[2], k, stride, 'same')
        return pads
    if unit == 'stem':
        pt, pl, pb, pr = same(xt, 3, 2)
        w = p['Conv1']
        cin = xt.shape[-1]
        z = F.conv2d(F.pad(xt.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w.reshape(3, 3, cin, w.shape[1]).permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1)
        y = bn(z, 'bn_Conv1', 'relu6')
    else:
        q, s = prefix(unit), STRIDES[unit]
        t = xt
        if unit > 0:
            t = bn(lin(t, p[q + 'expand']), q + 'expand_BN', 'relu6')
        t = bn(cref._depthwise(t, p[q + 'depthwise'], 3, s, same(t, 3, s)), q + 'depthwise_BN', 'relu6')
        y = bn(lin(t, p[q + 'project']), q + 'project_BN', None)
        if s == 1 and y.shape[-1] == xt.shape[-1]:
            y = y + xt
    out = {'y': y.detach().numpy(), 'relu6': relu6, 'stats': stats}
    if need:
        (y * torch.tensor(np.asarray(f, np.float64), dtype=dt)).sum().backward()
        out['x'] = xt.grad.numpy()
        out['grads'] = {k: p[k].grad.numpy() for k in sorted(want)}
    return out


def margins(r64, r32):
    return lr.relu6_margins([(w, u.astype(np.float64)) for w, u in r64['relu6']], [(w, u.astype(np.float32)) for w, u in r32['relu6']])


def rule_holds(host, case, seed):
    unit, hw, training = case
    x, _ = unit_inputs(host, unit, hw, seed)
    m = margins(torch_unit(host, unit, x, 'float64', training), torch_unit(host, unit, x, 'float32', training))
    return all(dist > bar for _, dist, bar in m), m


def first_seed(host, case, limit=4000):
    for seed in range(limit):
        if rule_holds(host, case, seed)[0]:
            return seed
    raise AssertionError('no seed below %d holds the rule for %s' % (limit, case_id(case)))


def oracle_taps():
    """-> (taps32, taps64): the NumPy oracle's b1..b4 on ``layers_ref.rfcr_case``'s images, computed once"""
    if 'taps' not in _shared:
        c = lr.rfcr_case(MODEL)
        x = params.synthetic_images(lr.BATCH, lr.RFCR_HW[0], lr.RFCR_HW[1])
        taps64 = [np.asarray(t, np.float64) for t in om.backbone_taps(c['P'], x.astype(np.float64), MODEL)]
        assert all(t.dtype == np.float64 for t in taps64)
        _shared['taps'] = (c['taps'], taps64)
    return _shared['taps']
