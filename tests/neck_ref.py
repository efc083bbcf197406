"""Everything ``yolov3_body`` runs behind the backbone, with the four taps as inputs: what tests/test_neck_host.py (CPU) and
tests/test_gpu_neck.py (device) share.  Test code over the oracle's own primitives; oracle/ is untouched.

* ``numpy_neck``: oracle/model.py:237-258 restated on ``oracle.model``'s functions (the NumPy oracle), taps in, logits out;
* ``torch_neck``: the same chain on torch from the parameters in the layouts of ``autograd.neck_parameters`` (host arrays), the
  restatement of oracle/torch_ref.py:121-140 in NHWC; inference mode (BatchNorms folded in the working dtype) or training mode
  (``bntrain_ref._forward64``: the statistics of the batch), with the gradients of sum_i (y_i * f_i).sum() for the taps and every
  parameter that is trained in that mode;
* the cases: ``layers_ref.rfcr_case`` (2 images at 96 x 96: maps of 3, 6 and 12) of both RFCR models; the gradient cases draw
  standard-normal taps from a committed seed."""
import numpy as np
import torch

from oracle import model as om, nn
from tests import bntrain_ref, convgrad_ref as cref, layers_ref as lr, segrad_ref as sref

MODELS = lr.RFCR_MODELS
ANCHORS, OUT_F = 3, 3 * (lr.CLASSES + 5)
HEADS = ('td1', 'td2', 'td3', 'bu3', 'bu2', 'bu1')
HEAD_F = dict(td1=512, td2=256, td3=128, bu3=128, bu2=256, bu1=512)
LINKS = ('block_20', 'block_24', 'bu3_down', 'bu2_down')
LINK_F = dict(block_20=256, block_24=128, bu3_down=128, bu2_down=256)
# the first seed per model (of 0, 1, 2, ...) whose standard-normal taps keep every ReLU6 input of the float64 run off the kinks by
# ``layers_ref.relu6_margins`` (twelve ReLU6 inputs with 10^5 elements between them: few seeds do) and |u| < 87 before every Swish and
# sigmoid, in inference mode and, for MobileNetV2 x0.75, in training mode; tests/test_neck_host.py asserts that they hold.  Chosen by
# that rule, never by what the device computes.  The tightest: training mode, bu2_down's ReLU6 input at 9.18e-05 against a margin of
# 8.95e-05 (no seed below 5500 clears the rule by more than 1.3 x there); the margins move by a few percent with the number of threads torch
# sums with, so tests/test_neck_host.py evaluates them on one thread.
GRAD_SEEDS = {'mobilenetv2x75': 57, 'efficientnetb0': 409}
TRAIN_MODEL = 'mobilenetv2x75'
TRAIN_SEED = 1434


# ----------------------------------------------------------------------------- the NumPy oracle, taps in
def numpy_neck(P, taps, dtype):
    """oracle/model.py:237-258 on the taps (b1, b2, b3, b4 already 4x-pooled) in ``dtype`` -> [y1, y2, y3] [B, G, G, 3, 25]"""
    b1, b2, b3, b4 = (np.asarray(t).astype(dtype) for t in taps)
    head = om.make_last_layers_efficientnet_lite
    b1, b2, b3 = om.rfcr_module(P, [b1, b2, b3, b4])
    x, _ = head(P, 'td1', b1, 512, OUT_F)
    c1 = x
    x = om._cbr(P, 'block_20_conv', 'block_20_BN', x, 256)
    x = nn.concat([nn.upsample2(x), b2])
    x, _ = head(P, 'td2', x, 256, OUT_F)
    c2 = x
    x = om._cbr(P, 'block_24_conv', 'block_24_BN', x, 128)
    x = nn.concat([nn.upsample2(x), b3])
    x, _ = head(P, 'td3', x, 128, OUT_F)
    c3 = x
    x, y3 = head(P, 'bu3', c3, 128, OUT_F)
    x = om._cbr(P, 'bu3_down_conv', 'bu3_down_BN', x, 128)
    x = nn.concat([nn.maxpool(x, 2), c2])
    x, y2 = head(P, 'bu2', x, 256, OUT_F)
    x = om._cbr(P, 'bu2_down_conv', 'bu2_down_BN', x, 256)
    x = nn.concat([nn.maxpool(x, 2), c1])
    x, y1 = head(P, 'bu1', x, 512, OUT_F)
    return [y.reshape(y.shape[0], y.shape[1], y.shape[2], ANCHORS, lr.CLASSES + 5) for y in (y1, y2, y3)]


def seeded_taps(model_name, seed):
    """standard-normal taps of the shapes of ``layers_ref.rfcr_case(model_name)``'s, and the functionals f1..f3 of the three logits"""
    rng = np.random.default_rng([seed, MODELS.index(model_name)])
    shapes = [t.shape for t in lr.rfcr_case(model_name)['taps']]
    taps = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    fs = [rng.standard_normal((lr.BATCH, g, g, ANCHORS, lr.CLASSES + 5)).astype(np.float32) for g in (3, 6, 12)]
    return taps, fs


# ----------------------------------------------------------------------------- parameters in the operators' layouts, on the host
def host_parameters(values):
    """``ParamStore.values`` -> the dictionary of ``autograd.neck_parameters`` as float32 host arrays (no 'cin' entry), written from
    that function's documentation with ``layers_ref``'s converters"""
    def bn(name):
        return {p: np.asarray(values['%s/%s' % (name, p)], np.float32).reshape(-1) for p in lr.BN_PARTS}
    rfcr = {c: lr.pack_conv(values[c + '/kernel']) for c in ('rfcr_b1c', 'rfcr_b2c', 'rfcr_b3c', 'rfcr_b4c', 'rfcr_sep_pw')}
    rfcr['rfcr_wsum/alpha'] = np.asarray(values['rfcr_wsum/alpha'], np.float32).reshape(4)
    rfcr['rfcr_sep_dw'] = lr.pack_dw(values['rfcr_sep_dw/depthwise_kernel'])
    for b in ('rfcr_sep_dw_BN', 'rfcr_sep_pw_BN'):
        rfcr.update({'%s/%s' % (b, p): v for p, v in bn(b).items()})
    out = {'rfcr': rfcr}
    for h in HEADS:
        d = {c: lr.pack_conv(values[h + c + '/kernel']) for c in ('_conv', '_mb_project', '_y') if h + c + '/kernel' in values and (c != '_y' or h.startswith('bu'))}
        d['_mb_dw'] = lr.pack_dw(values[h + '_mb_dw/depthwise_kernel'])
        for se in ('_mb_se_reduce', '_mb_se_expand'):
            d[se] = np.asarray(values[h + se + '/kernel'], np.float32)[0, 0]
            d[se + '/bias'] = np.asarray(values[h + se + '/bias'], np.float32).reshape(-1)
        for b in ('_conv_BN', '_mb_dw_BN', '_mb_project_BN'):
            d.update({'%s/%s' % (b, p): v for p, v in bn(h + b).items()})
        out[h] = d
    for name in LINKS:
        d = {'_conv': lr.pack_conv(values[name + '_conv/kernel'])}
        d.update({'_BN/' + p: v for p, v in bn(name + '_BN').items()})
        out[name] = d
    return out


def is_moving(key):
    return key.endswith(('/moving_mean', '/moving_variance'))


def is_bn_affine(key):
    return key.endswith(('/gamma', '/beta'))


def trained_keys(host, training):
    """[(group, key)] of everything that takes a gradient: all but the moving statistics, and in inference mode all but the folded
    gamma and beta as well"""
    return [(g, k) for g, d in host.items() for k in d if not is_moving(k) and (training or not is_bn_affine(k))]


# ----------------------------------------------------------------------------- the chain on torch
def torch_neck(host, taps, dtype, training=False, fs=None):
    """The neck on torch in ``dtype`` ('float64' / 'float32') from ``host_parameters``' dictionary, NHWC throughout ->
    {'y': [y1, y2, y3] arrays [B, G, G, 3, 25], 'relu6': [(what, u)] the inputs of every ReLU6, 'smooth': [(what, u)] those of every
    Swish and sigmoid, 'stats': {(group, bn): (mean, biased variance, N)} (training)}; with fs also 'taps': the gradients of
    sum_i (y_i * f_i).sum() for b1..b4 and 'grads': {(group, key): gradient in the parameter's layout} for ``trained_keys``."""
    dt = cref.DT[dtype]
    need = fs is not None
    want = set(trained_keys(host, training))
    p = {g: {k: torch.tensor(np.asarray(v, np.float64), dtype=dt, requires_grad=need and (g, k) in want) for k, v in d.items()} for g, d in host.items()}
    tt = [torch.tensor(np.asarray(t, np.float64), dtype=dt, requires_grad=need) for t in taps]
    relu6, smooth, stats = [], [], {}

    def lin(t, w):
        cin = t.shape[-1]
        return cref._linear(t.reshape(-1, cin), w[:, :cin]).reshape(tuple(t.shape[:-1]) + (w.shape[0],))

    def bn(z, group, name, act):
        q = p[group]
        if training:
            u = bntrain_ref._forward64(z.reshape(-1, z.shape[-1]), q[name + '/gamma'], q[name + '/beta'], 1e-3)
            stats[(group, name)] = (u[2].detach().numpy(), u[3].detach().numpy(), u[0].shape[0])
            u = u[0].reshape(z.shape)
        else:
            scale = q[name + '/gamma'] / torch.sqrt(q[name + '/moving_variance'] + 1e-3)
            u = z * scale + (q[name + '/beta'] - q[name + '/moving_mean'] * scale)
        what = '%s of %s %s' % (act, group, name)
        if act == 'relu6':
            relu6.append((what, u.detach().numpy()))
        elif act == 'swish':
            smooth.append((what, u.detach().numpy()))
        return cref._act(u, act)

    def dw(t, w, k):
        return cref._depthwise(t, w, k, 1, (k // 2,) * 4)

    def up(t):
        return t.repeat_interleave(2, 1).repeat_interleave(2, 2)

    def pool(t, k):
        return torch.nn.functional.max_pool2d(t.permute(0, 3, 1, 2), k).permute(0, 2, 3, 1)

    def se(t, q, group):
        s = t.mean(dim=(1, 2)) @ q['_mb_se_reduce'] + q['_mb_se_reduce/bias']
        smooth.append(('swish of %s _mb_se_reduce' % group, s.detach().numpy()))
        s = (s * torch.sigmoid(s)) @ q['_mb_se_expand'] + q['_mb_se_expand/bias']
        smooth.append(('sigmoid of %s _mb_se_expand' % group, s.detach().numpy()))
        return t * torch.sigmoid(s)[:, None, None, :]

    def head(t, name):
        q = p[name]
        t = bn(lin(t, q['_conv']), name, '_conv_BN', 'relu6')
        t = bn(dw(t, q['_mb_dw'], 3), name, '_mb_dw_BN', 'swish')
        t = se(t, q, name)
        xo = bn(lin(t, q['_mb_project']), name, '_mb_project_BN', None)
        return xo, (lin(xo, q['_y']) if '_y' in q else None)

    def link(t, name):
        return bn(lin(t, p[name]['_conv']), name, '_BN', 'relu6')
    r = p['rfcr']
    b1, b2, b3, b4 = tt
    c = [lin(t, r[k]) for t, k in zip(tt, ('rfcr_b1c', 'rfcr_b2c', 'rfcr_b3c', 'rfcr_b4c'))]
    a = r['rfcr_wsum/alpha']
    bc = a[0] * up(c[0]) + a[1] * c[1] + a[2] * pool(c[2], 2) + a[3] * c[3]
    bc = bn(dw(bc, r['rfcr_sep_dw'], 5), 'rfcr', 'rfcr_sep_dw_BN', 'relu6')
    bc = bn(lin(bc, r['rfcr_sep_pw']), 'rfcr', 'rfcr_sep_pw_BN', 'relu6')
    b1, b2, b3 = torch.cat([b1, pool(bc, 2)], -1), torch.cat([b2, bc], -1), torch.cat([b3, up(bc)], -1)
    c1, _ = head(b1, 'td1')
    c2, _ = head(torch.cat([up(link(c1, 'block_20')), b2], -1), 'td2')
    c3, _ = head(torch.cat([up(link(c2, 'block_24')), b3], -1), 'td3')
    x, y3 = head(c3, 'bu3')
    x, y2 = head(torch.cat([pool(link(x, 'bu3_down'), 2), c2], -1), 'bu2')
    x, y1 = head(torch.cat([pool(link(x, 'bu2_down'), 2), c1], -1), 'bu1')
    ys = [y.reshape(y.shape[0], y.shape[1], y.shape[2], ANCHORS, lr.CLASSES + 5) for y in (y1, y2, y3)]
    out = {'y': [y.detach().numpy() for y in ys], 'relu6': relu6, 'smooth': smooth, 'stats': stats}
    if need:
        sum((y * torch.tensor(np.asarray(f, np.float64), dtype=dt)).sum() for y, f in zip(ys, fs)).backward()
        out['taps'] = [t.grad.numpy() for t in tt]
        out['grads'] = {(g, k): p[g][k].grad.numpy() for g, k in sorted(want)}
    return out


def margins(r64, r32):
    """``layers_ref.relu6_margins`` over the ReLU6 inputs of two ``torch_neck`` runs, and the largest |u| before a Swish or sigmoid"""
    m = lr.relu6_margins([(w, u.astype(np.float64)) for w, u in r64['relu6']], [(w, u.astype(np.float32)) for w, u in r32['relu6']])
    return m, max(float(np.abs(u).max()) for _, u in r64['smooth'])


# ----------------------------------------------------------------------------- td1 alone (tests/test_gpu_conv1x1_autograd.py)
# (model, block, input channels, F, seed): the widest head block of MobileNetV2 x0.75, 216 -> 512 -> 75, on the 3 x 3 map it has at
# 96 x 96; the seed is the first whose ReLU6 inputs stay off the kinks (tests/test_neck_host.py asserts it)
TD1_CASE = ('mobilenetv2x75', 'td1', 120 + 96, 512, 0)


def td1_inputs():
    """-> (x [2, 3, 3, 216], f1 [2, 3, 3, 75]) float32: the input and the functional of x_out"""
    rng = np.random.default_rng([TD1_CASE[4], TD1_CASE[2]])
    return (rng.standard_normal((lr.BATCH, 3, 3, TD1_CASE[2])).astype(np.float32),
            rng.standard_normal((lr.BATCH, 3, 3, OUT_F)).astype(np.float32))
