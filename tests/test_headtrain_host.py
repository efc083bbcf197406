"""Host side of the output-layer training (no GPU): the Adam restatement of tests/headtrain_ref.py against hand-derived answers,
the cosine schedule, yolov3_features on the host-compiled plan, the gradient's chunk function, and the new entries of the library."""
import ctypes
import math
import types

import numpy as np
import pytest

from tests import headtrain_ref as ref

F = np.float32


# ----------------------------------------------------------------------------- Adam
def test_adam_first_step_from_zero_moments():
    """m = (1 - b1) g, v = (1 - b2) g^2, alpha = lr sqrt(1 - b2) / (1 - b1):
    w' = w - lr g / (|g| + eps / sqrt(1 - b2)).  With w = 1, g = 0.5, lr = 1e-3: eps / sqrt(0.001) = 3.1623e-7,
    0.5 / 0.50000031623 = 0.99999936754, w' = 1 - 0.00099999936754 = 0.99900000063."""
    w, m, v = ref.adam_step(F([1.0, 1.0]), F([0, 0]), F([0, 0]), F([0.5, -0.5]), ref.adam_alpha(1e-3, 1))
    assert abs(float(w[0]) - 0.99900000063) < 1.5e-7 and abs(float(w[1]) - 1.00099999937) < 1.5e-7      # (an ulp of float32 below 1 is 6e-8)
    assert m[0] == F(F(1) - F(.9)) * F(.5) and m[1] == -m[0]
    assert v[0] == F(F(1) - F(.999)) * F(.25) and v[1] == v[0]
    assert float(ref.adam_alpha(1e-3, 1)) == pytest.approx(1e-3 * math.sqrt(1 - .999) / (1 - .9), rel=1e-7)


def test_adam_zero_gradient_changes_nothing():
    w0 = F([1.0, -2.5, 3e-9])
    w, m, v = ref.adam_step(w0, F([0, 0, 0]), F([0, 0, 0]), F([0, 0, 0]), ref.adam_alpha(1e-3, 1))
    assert np.array_equal(w.view(np.uint32), w0.view(np.uint32)) and not m.any() and not v.any()      # 0 / (0 + eps) = 0 exactly


def test_adam_second_step_with_the_same_gradient():
    """With a constant gradient the bias-corrected moments are g and g^2 at every step: m2 = 0.9 * 0.05 + 0.1 * 0.5 = 0.095,
    v2 = 0.999 * 0.00025 + 0.001 * 0.25 = 0.00049975, alpha2 = 1e-3 sqrt(0.001999) / 0.19 = 2.353167e-4, and
    alpha2 m2 / sqrt(v2) = 1e-3 * (0.095 / 0.19) / sqrt(0.00049975 / 0.001999) = 1e-3 * 0.5 / 0.5: the second step subtracts
    1e-3 / (1 + eps / sqrt(v2)) = 1e-3 * (1 - 4.47e-7) as well: w2 = 0.99900000063 - 0.00099999955 = 0.99800000108."""
    g = F([0.5])
    w, m, v = ref.adam_step(F([1.0]), F([0]), F([0]), g, ref.adam_alpha(1e-3, 1))
    w, m, v = ref.adam_step(w, m, v, g, ref.adam_alpha(1e-3, 2))
    # 1 - b formed in float32: float32(0.999) is 0.99899995, so 1 - b2 = 0.0010000467 (relative 4.7e-5; the bound is 2^-24 / 0.001 =
    # 6e-5), and 1 - b1 = 0.100000024 (2^-24 / 0.1 = 6e-7): v carries the first, m the second; through sqrt(v) the step moves by
    # at most 3e-5 of 1e-3 = 3e-8 per step, inside the 2e-7 asked of w below
    assert float(m[0]) == pytest.approx(0.095, rel=1e-6) and float(v[0]) == pytest.approx(0.00049975, rel=1e-4)
    assert float(ref.adam_alpha(1e-3, 2)) == pytest.approx(2.353167e-4, rel=1e-6)
    assert abs(float(w[0]) - 0.99800000108) < 2e-7
    w64, m64, v64 = ref.adam_step64(np.array([1.0]), np.zeros(1), np.zeros(1), np.array([0.5]), 1e-3, 1)
    w64, _, _ = ref.adam_step64(w64, m64, v64, np.array([0.5]), 1e-3, 2)
    assert abs(float(w[0]) - float(w64[0])) < 2e-7


def test_adam_restatement_is_float32_throughout():
    rng = np.random.default_rng(0)
    w, g = rng.standard_normal(1000).astype(F), rng.standard_normal(1000).astype(F)
    wn, mn, vn = ref.adam_step(w, np.zeros_like(w), np.zeros_like(w), g, ref.adam_alpha(1e-3, 1))
    assert wn.dtype == mn.dtype == vn.dtype == np.float32
    w64, _, _ = ref.adam_step64(w.astype(np.float64), 0.0, 0.0, g.astype(np.float64), 1e-3, 1)
    assert np.max(np.abs(wn - w64)) < 1e-6


# ----------------------------------------------------------------------------- the schedule
def test_cosine_schedule_end_points():
    from yoloret_amd.yolo3.train import cosine_decay
    assert ref.cosine_lr(1e-3, 0, 50) == 1e-3
    assert ref.cosine_lr(1e-3, 25, 50) == pytest.approx(5e-4, rel=1e-12)
    assert ref.cosine_lr(1e-3, 50, 50) == pytest.approx(0.0, abs=1e-18)
    assert ref.cosine_lr(1e-3, 49, 50) == pytest.approx(1e-3 * 0.5 * (1 - math.cos(math.pi / 50)), rel=1e-9)
    for e in range(51):
        assert cosine_decay(1e-3, e, 50) == pytest.approx(ref.cosine_lr(1e-3, e, 50), rel=1e-12, abs=1e-18)


# ----------------------------------------------------------------------------- yolov3_features
@pytest.fixture(scope='module')
def body():
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3.model import yolov3_body
    return yolov3_body(L.Input(shape=[96, 96, 3]), 'mobilenetv2x75', 3, num_classes=20)


def test_features_model_shapes_and_parameters(body):
    from yoloret_amd.yolo3.model import output_convs, yolov3_features
    feats = yolov3_features(body)
    assert [tuple(o.shape) for o in feats.outputs] == [(3, 3, 75), (6, 6, 75), (12, 12, 75)]
    assert [(ob.h, ob.w, ob.c) for ob in feats.plan.output_bufs] == [(3, 3, 75), (6, 6, 75), (12, 12, 75)]
    assert feats.inputs[0] is body.inputs[0] and feats.dtype == 0
    kernels = [c.name + '/kernel' for c in output_convs(body)]
    assert kernels == ['bu1_y/kernel', 'bu2_y/kernel', 'bu3_y/kernel']
    want = {k: v for k, v in body.param_shapes.items() if k not in kernels}
    assert len(want) == len(body.param_shapes) - 3 and feats.param_shapes == want
    assert all(body.param_shapes[k] == (1, 1, 75, 75) for k in kernels)
    # set_weights takes the subset of the model's weights that the feature model's param_shapes name
    from yoloret_amd.weights import synthetic_weights
    weights = synthetic_weights(body, 1234, 'conditioned')
    feats.set_weights(weights)
    assert set(feats.get_weights()) == set(want)


def test_features_plans_read_no_dense_output(body):
    """A model output is written densely (a channel stride of 75), which no op can read back: the features that also feed the
    bottom-up path therefore get a producer of their own, in every plan variant."""
    from yoloret_amd.compiler import compile_graph
    from yoloret_amd.yolo3.model import yolov3_features
    feats = yolov3_features(body)
    for variant in (True, 'mid', 'nohead', 'nohead_k', 'latency', False):
        plan = compile_graph(feats.inputs[0], feats.outputs, variant, 0)
        assert [(ob.h, ob.w, ob.c, ob.ld) for ob in plan.output_bufs] == [(3, 3, 75, 75), (6, 6, 75, 75), (12, 12, 75, 75)]
        bad = [(o.name, s.buf.name, s.buf.ld) for o in plan.ops for s in o.srcs if s.buf.external_slot >= 1 or (s.buf.ld % 4 and s.buf.external_slot != 0)]
        assert not bad, (variant, bad)
        assert dict(plan.param_shapes) == feats.param_shapes


def test_features_refuses_other_outputs(body):
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3.model import output_convs, yolov3_features
    feats = yolov3_features(body)
    with pytest.raises(ValueError, match='Reshape5'):
        yolov3_features(feats)                      # its outputs are feature maps, not Reshape5 nodes
    t = L.Input(shape=[4, 4, 8])
    for conv, what in ((L.Conv2D(75, 1, use_bias=True, name='biased_y'), 'bias'), (L.Conv2D(75, 3, use_bias=False, name='k3_y'), '3x3'),
                       (L.Conv2D(75, 1, strides=2, use_bias=False, name='s2_y'), 'stride')):
        fake = types.SimpleNamespace(dtype=0, inputs=[t], outputs=[L.Reshape5(3, name='y_' + what)(conv(t))])
        with pytest.raises(ValueError, match='bias-free 1x1'):
            output_convs(fake)
    bn = L.Reshape5(3, name='y_bn')(L.BatchNormalization(name='y_BN')(L.Conv2D(75, 1, use_bias=False, name='bn_y')(t)))
    with pytest.raises(ValueError, match='bias-free 1x1'):
        yolov3_features(types.SimpleNamespace(dtype=0, inputs=[t], outputs=[bn]))
    act = L.Reshape5(3, name='y_act')(L.ReLU(6., name='y_relu')(L.Conv2D(75, 1, use_bias=False, name='act_y')(t)))
    with pytest.raises(ValueError, match='bias-free 1x1'):
        yolov3_features(types.SimpleNamespace(dtype=0, inputs=[t], outputs=[act]))
    with pytest.raises(ValueError, match='bias-free 1x1'):
        yolov3_features(types.SimpleNamespace(dtype=0, inputs=[t], outputs=[L.Reshape5(3, name='y_in')(t)]))


def test_features_refuses_16_bit_plans():
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3.model import yolov3_body, yolov3_features
    L.set_global_policy('mixed_bfloat16')
    try:
        m16 = yolov3_body(L.Input(shape=[96, 96, 3]), 'mobilenetv2x75', 3, num_classes=20)
    finally:
        L.set_global_policy('float32')
    with pytest.raises(NotImplementedError, match='float32'):
        yolov3_features(m16)


def test_trainer_refuses_ema_adv_and_missing_weights(body):
    from yoloret_amd.yolo3.train import OutputLayerTrainer
    from yoloret_amd.weights import synthetic_weights
    from tests.util import ANCHORS
    if body.get_weights() is None:
        with pytest.raises(ValueError, match='no weights'):
            OutputLayerTrainer(body, ANCHORS, 20, 3)
        body.set_weights(synthetic_weights(body, 1234, 'conditioned'))
    tr = OutputLayerTrainer(body, ANCHORS, 20, 3)
    assert tr.dims == [(75, 75, 76)] * 3 and tr.kernel_names == ['bu1_y/kernel', 'bu2_y/kernel', 'bu3_y/kernel']
    with pytest.raises(NotImplementedError):
        tr.fit(1, [], use_ema=True)
    with pytest.raises(NotImplementedError):
        tr.fit(1, [], use_adv=True)
    with pytest.raises(ValueError, match='classes'):
        OutputLayerTrainer(body, ANCHORS, 80, 3)


# ----------------------------------------------------------------------------- the library
def test_new_entries_are_exported_under_abi_9():
    from yoloret_amd import build, runtime
    L = ctypes.CDLL(build.LIB)
    L.yr_abi_version.restype = ctypes.c_int
    assert L.yr_abi_version() == 9 == runtime.ABI_VERSION
    for sym in ('yr_linear_forward', 'yr_linear_wgrad_chunk', 'yr_linear_wgrad_workspace_bytes', 'yr_linear_wgrad', 'yr_adam_step'):
        getattr(L, sym)
        assert sym in runtime.EXPORTS
    assert 'headtrain.hip' in build.SOURCES


def test_chunk_and_workspace_are_functions_of_the_sizes_only():
    from yoloret_amd import runtime as rt
    for pixels, cin, cout in ((1, 1, 1), (3, 75, 75), (173056, 75, 75), (64 * 52 * 52, 75, 80), (10 ** 7, 75, 75), (4101, 255, 255), (5000, 256, 3)):
        chunk = rt.linear_wgrad_chunk(pixels, cin, cout)
        assert chunk >= 256 and chunk % 16 == 0 and chunk == rt.linear_wgrad_chunk(pixels, cin, cout)
        assert -(-pixels // chunk) <= 2048
        assert rt.linear_wgrad_workspace_bytes(pixels, cin, cout) == -(-pixels // chunk) * cout * ((cin + 3) // 4 * 4) * 4
    for bad in ((0, 75, 75), (-1, 75, 75), (1 << 40, 75, 75), (100, 0, 75), (100, 257, 75), (100, 75, 0), (100, 75, 257)):
        assert rt.linear_wgrad_chunk(*bad) == 0 and rt.linear_wgrad_workspace_bytes(*bad) == 0


# ----------------------------------------------------------------------------- what tests/test_gpu_headtrain_forms.py reaches
def test_form_cases_reach_every_instantiation():
    """The claim of tests/test_gpu_headtrain_forms.py, from its own case lists and its restatement of ht_blocking: the unblocked
    cases run all 25 ht_wgrad_partial_kernel<TCO, TCI> and all 5 ht_forward_kernel<NT>."""
    from tests import test_gpu_headtrain_forms as forms
    assert [forms.blocking(n) for n in forms.WIDTHS] == [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5)]
    assert all(n % 4 and forms.idle_tiles(n) == 0 for n in forms.WIDTHS)
    assert len(forms.FORM_WGRAD) == 25
    assert {forms.wgrad_form(cin, cout) for cin, cout in forms.FORM_WGRAD} == {(tco, tci) for tco in range(1, 6) for tci in range(1, 6)}
    for cin in (29, 77):
        assert {forms.forward_form(cout) for c, cout in forms.FORM_FORWARD if c == cin} == {1, 2, 3, 4, 5}
    # the restatement against the source's own words
    import os
    from yoloret_amd import build
    csrc = os.path.join(os.path.dirname(build.__file__), 'csrc')
    common = open(os.path.join(csrc, 'train_common.h')).read()       # the rule is stated there, once, for headtrain.hip and convgrad.hip
    assert '#define TC_MAX_T %d ' % forms.MAX_T in common
    assert '*blocks = (t + TC_MAX_T - 1) / TC_MAX_T;' in common and '*per = (t + *blocks - 1) / *blocks;' in common
    src = open(os.path.join(csrc, 'headtrain.hip')).read()
    assert '#include "train_common.h"' in src and 'tc_blocking(cout, &bo, &to);' in src and 'tc_blocking(cin, &bi, &ti);' in src
    assert 'HT_MAX_T' not in src and '+ 15) / 16' not in src, 'no second statement of the rule'


def test_ragged_cases_leave_whole_tiles_out_of_range():
    from tests import test_gpu_headtrain_forms as forms
    assert forms.RAGGED_BLOCKINGS == {97: (2, 4), 161: (3, 4), 193: (3, 5), 81: (2, 3), 209: (3, 5)}
    for n, want in forms.RAGGED_BLOCKINGS.items():
        assert forms.blocking(n) == want, n
    assert forms.blocking(3) == (1, 1)
    assert [forms.idle_tiles(n) for n in (97, 161, 193, 81, 209, 3)] == [1, 1, 2, 0, 1, 0]
    used = {n for case in forms.RAGGED_WGRAD + forms.RAGGED_FORWARD for n in case}
    assert used == set(forms.RAGGED_BLOCKINGS) | {3}
    # a block with a whole tile beyond the channel count on the cin side, on the cout side, both at once, and in the forward
    assert any(forms.idle_tiles(cin) and not forms.idle_tiles(cout) for cin, cout in forms.RAGGED_WGRAD)
    assert any(forms.idle_tiles(cout) and not forms.idle_tiles(cin) for cin, cout in forms.RAGGED_WGRAD)
    assert any(forms.idle_tiles(cin) and forms.idle_tiles(cout) for cin, cout in forms.RAGGED_WGRAD)
    assert any(forms.idle_tiles(cout) == 2 for _, cout in forms.RAGGED_FORWARD)
    # blocked shapes take the larger minimum chunk
    from yoloret_amd import runtime as rt
    assert all(rt.linear_wgrad_chunk(p, cin, cout) == 512 for cin, cout in forms.RAGGED_WGRAD for p in (1, 5, 513, 2048 * 512))


def test_chunk_leaves_its_minimum_at_2048_chunks():
    from tests import test_gpu_headtrain_forms as forms
    from yoloret_amd import runtime as rt
    assert (forms.BIG_PIXELS, forms.BIG_CIN, forms.BIG_COUT) == (524289, 5, 3)
    assert rt.linear_wgrad_chunk(524289, 5, 3) == 272 == forms.BIG_CHUNK
    assert rt.linear_wgrad_chunk(524288, 5, 3) == 256
    assert -(-524289 // 272) == 1928 == forms.BIG_SLABS
    assert rt.linear_wgrad_workspace_bytes(524289, 5, 3) == 1928 * 3 * 8 * 4
    assert rt.linear_wgrad_workspace_bytes(524288, 5, 3) == 2048 * 3 * 8 * 4
    for pixels, chunk in forms.BIG_EXACT:
        assert rt.linear_wgrad_chunk(pixels, 5, 3) == chunk and 16 * pixels < 2 ** 24
    # 272 pixels: 68 = 17 quartets per wave, an odd number: eight groups of HT_U = 2 and one single quartet in every wave
    assert 272 % 16 == 0 and (272 // 4) % 4 == 0 and (272 // 4 // 4) % 2 == 1
    # the blocked shapes leave their minimum at 2048 * 512 + 1
    assert rt.linear_wgrad_chunk(2048 * 512, 255, 255) == 512 and rt.linear_wgrad_chunk(2048 * 512 + 1, 255, 255) == 528


def test_kernels_use_no_scratch():
    from yoloret_amd import build
    rows = build.kernel_resources()['headtrain.hip']
    assert len(rows) == 2 + 25 + 5
    assert all(scratch == 0 for _, _, scratch, _, _ in rows)
    full = [r for r in rows if 'ht_wgrad_partial_kernelILi5ELi5E' in r[0]]
    assert len(full) == 1 and full[0][3] >= 2, 'the 5 x 5 tile form keeps at least two waves per SIMD'
