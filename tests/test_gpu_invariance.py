"""Whole-plan invariances the product relies on, beyond what the per-op suite checks:

  A. the logits do not depend on what the workspace held before the step (Model.__call__ reuses one arena per context; a tile a
     kernel never writes, a padding lane it reads, an arrival counter it does not clear would show here): every plan variant is
     run on a workspace poisoned with NaN bytes, large finite bytes and random bytes, into NaN-filled outputs, and must give the
     same bits each time - and image 0 must meet the oracle bar, so a consistently wrong result cannot pass;
  B. the logits do not depend on the tuning table (engine.py: a tuning choice "changes speed only, never results"; every process
     autotunes by timing, parallel.share_tuning installs rank 0's table on every rank): one op at a time, every entry yr_autotune
     itself dispatches for that op (tests/util.py: autotune_candidates, checked against runtime.hip by tests/test_host_logic.py);
  C. the logits do not depend on an image's slot in the batch: EVERY image of each bench configuration's full batch against its own
     batch-1 run and against the oracle;
  D. the hoist-off head-stream plan (compiler.HOIST_UPSAMPLE = False) compiles to launches the library takes.

Entries a launcher refuses with a clean error at forward time (a tile an op's accumulators or LDS cannot hold) count as "not this
op's shape", as they do in yr_autotune; the handle must run the baseline table afterwards."""
import numpy as np
import pytest
import torch

from oracle import params
from tests import fence
from yoloret_amd.weights import synthetic_weights
from tests.util import POISON_PATTERNS, assert_close, autotune_candidates, nan_outputs, poison_workspace

pytestmark = pytest.mark.gpu

POLICY = {'f32': 'float32', 'bf16': 'mixed_bfloat16', 'f16': 'mixed_float16'}


def _ceil16():
    from tests.test_gpu_narrow import CEIL16   # (scaled max, scaled mean) logit error ceilings per (model, 16-bit type)
    return CEIL16


def _model(name, size, dt):
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3.model import yolov3_body
    L.set_global_policy(POLICY[dt])
    try:
        return yolov3_body(L.Input(shape=[size, size, 3]), name, 3, num_classes=20)
    finally:
        L.set_global_policy('float32')


def _oracle(P, name, x, dtype=torch.float32, chunk=16):
    """torch-CPU port of the graph (oracle/torch_ref.py), in chunks of images: [y1, y2, y3] numpy [B,G,G,A,C+5]."""
    from oracle import torch_ref
    ref = torch_ref.TorchReference(P, name, 3, 20, dtype=dtype)
    parts = [ref(x[i:i + chunk]) for i in range(0, len(x), chunk)]
    return [np.concatenate([p[k] for p in parts]) for k in range(3)]


def _errs(a, ref):
    e = np.abs(np.asarray(a, np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    return float(e.max()), float(e.mean())


def _check_image0(ys, ref, name, dt, what):
    """Image 0 against the float32 oracle: the 1e-4 bar (float32 plans), the per-(model, type) ceilings of the 16-bit plans."""
    for k, (y, r) in enumerate(zip(ys, ref)):
        g = y[0:1].reshape(r[0:1].shape)
        if dt == 'f32':
            assert_close(g, r[0:1], 1e-4, '%s y%d' % (what, k + 1))
        else:
            gm, ga = _errs(g, r[0:1])
            cm, ca = _ceil16()[(name, dt)]
            assert gm <= cm and ga <= ca, '%s y%d: scaled error max %.3e / mean %.3e above the ceilings %.1e / %.1e' % (what, k + 1, gm, ga, cm, ca)


def _poisoned_runs(m, xd, ctx=0, seed=0):
    """One forward per poison pattern, each on a freshly poisoned workspace into NaN outputs: [[y1, y2, y3] numpy] per pattern."""
    b, idx = xd.shape[0], xd.device.index
    runs = []
    for n, pat in enumerate(POISON_PATTERNS):
        poison_workspace(m, idx, ctx, pat, seed=seed + n)
        ys = m(xd, out=nan_outputs(m, b), ctx=ctx)
        torch.cuda.synchronize()
        runs.append([y.cpu().numpy() for y in ys])
    return runs


def _assert_same_bits(runs, what):
    for k, y in enumerate(runs[0]):
        assert np.isfinite(y).all(), '%s y%d: non-finite logits (pattern %r)' % (what, k + 1, POISON_PATTERNS[0])
    for n, r in enumerate(runs[1:], 1):
        for k, (a, b) in enumerate(zip(r, runs[0])):
            assert np.isfinite(a).all(), '%s y%d: non-finite logits (pattern %r)' % (what, k + 1, POISON_PATTERNS[n])
            assert np.array_equal(a, b), '%s y%d: logits differ between workspace patterns %r and %r (%d elements)' % (
                what, k + 1, POISON_PATTERNS[0], POISON_PATTERNS[n], int((a != b).sum()))


# ------------------------------------------------------------------ A. workspace contents
# (name, size, type, variant, batch): the variant is reached through the product defaults (small_batch 4 | 2, ksplit_batch 2,
# mbk_batch 24 for float32 plans) and the batch size - tests/conftest.py pins the environment's small_batch / mbk_batch to 0
A_CASES = [('mobilenetv2x75', 160, 'f32', 'throughput', 24), ('mobilenetv2x75', 160, 'f32', 'mid', 6),
           ('mobilenetv2x75', 160, 'f32', 'nohead', 3), ('mobilenetv2x75', 160, 'f32', 'nohead_k', 2),
           ('mobilenetv2x14', 224, 'f32', 'throughput', 24),
           ('efficientnetb0-lite', 224, 'bf16', 'latency', 2), ('efficientnetb0-lite', 224, 'bf16', 'throughput', 3),
           ('efficientnetb3-lite', 224, 'f16', 'throughput', 3),
           ('efficientnetb0', 224, 'bf16', 'throughput', 3), ('efficientnetb3', 224, 'f16', 'throughput', 3),
           ('mobilenetv2x75', 416, 'f32', 'throughput', 64)]     # BASELINE config 2 at its full batch


def _product_defaults(m, dt):
    if dt == 'f32':
        m.small_batch, m.ksplit_batch, m.mbk_batch = 4, 2, 24
    else:
        m.small_batch = 2


def _workspace_case(dev, name, size, dt, variant, b):
    m = _model(name, size, dt)
    _product_defaults(m, dt)
    assert m.variant(b) == variant
    P = params.ParamStore(1234, 'conditioned')
    x = params.synthetic_images(b, size, size)
    ref = _oracle(P, name, x[:1])           # (the oracle's walk creates every parameter)
    m.set_weights(P.values)
    xd = torch.from_numpy(x).to(dev)
    m(xd)                                   # allocates the workspace, autotunes, runs the range guard
    torch.cuda.synchronize()
    runs = _poisoned_runs(m, xd)
    what = '%s@%d %s %s B=%d' % (name, size, dt, variant, b)
    _assert_same_bits(runs, what)
    _check_image0(runs[0], ref, name, dt, what)
    return m, runs


@pytest.mark.parametrize('name,size,dt,variant,b', A_CASES, ids=['%s-%d-%s-%s-b%d' % c for c in A_CASES])
def test_logits_do_not_depend_on_the_workspace(dev, name, size, dt, variant, b):
    _workspace_case(dev, name, size, dt, variant, b)


def _fenced_buffers(m, xd, pattern, seed):
    """A workspace of exactly m.workspace_bytes(b) bytes holding `pattern`, and NaN outputs: what a fenced pass works in."""
    b = xd.shape[0]
    ws = torch.empty(m.workspace_bytes(b), dtype=torch.uint8, device=xd.device)
    if pattern == 'random':
        g = torch.Generator(device=xd.device)
        g.manual_seed(seed)
        ws.random_(0, 256, generator=g)
    else:
        ws.fill_(int(pattern))
    return ws, nan_outputs(m, b)


def _fenced_forward(m, xd, pattern, seed=0):
    """yr_autotune + yr_forward (Model.__call__ on a batch size it has not tuned) with the input batch, the three outputs and the
    workspace each between the guards of tests/fence.py, in both of its variants: -> [y1, y2, y3] numpy."""
    b, idx = xd.shape[0], xd.device.index
    assert m.autotune
    ws, ys = _fenced_buffers(m, xd, pattern, seed)
    saved = m._workspace.get(idx)

    def call(moved):
        m._workspace[idx] = moved(ws)                   # (a view of exactly workspace_bytes(b) bytes: Model.__call__ takes it as it is)
        m._tuned.discard((idx, b))                      # the tuner's trial launches run on the fenced buffers too
        m(moved(xd), out=[moved(y) for y in ys])
        assert m._workspace[idx].data_ptr() == moved(ws).data_ptr()
    try:
        fence.run(call, writes=ys, reads=[xd], scratch=[ws], batch=b)
    finally:
        m._workspace[idx] = saved
    torch.cuda.synchronize()
    return [y.cpu().numpy() for y in ys]


@pytest.mark.parametrize('name,size,dt,variant,b', A_CASES, ids=['%s-%d-%s-%s-b%d' % c for c in A_CASES])
def test_plans_stay_inside_their_buffers(dev, name, size, dt, variant, b):
    """Every plan variant of section A (batches of 2, 3, 6, 24 and config 2's 64: at an odd batch the arena's per-op pointers are
    16-byte aligned and no more) with input, outputs and workspace fenced, once per poison pattern: no byte around any of the five
    buffers changes during yr_autotune + yr_forward, nothing around the input reaches the logits, and the logits are those of the
    unfenced pass bit for bit (which section A holds to the oracle's bar on image 0)."""
    m, runs = _workspace_case(dev, name, size, dt, variant, b)
    xd = torch.from_numpy(params.synthetic_images(b, size, size)).to(dev)
    what = '%s@%d %s %s B=%d, fenced' % (name, size, dt, variant, b)
    for n, pat in enumerate(POISON_PATTERNS):
        got = _fenced_forward(m, xd, pat, seed=n)
        for k, (g, w) in enumerate(zip(got, runs[0])):
            g = g.reshape(w.shape)
            assert np.isfinite(g).all() and np.array_equal(g, w), '%s (pattern %r) y%d differs from the unfenced pass (%d elements)' % (
                what, pat, k + 1, int((g != w).sum()))


def test_ranges_and_profile_passes_stay_inside_their_buffers(dev):
    """yr_forward_ranges and yr_forward_profile, the other two entries that walk a whole plan, through the C ABI with fenced buffers
    (an odd batch): guards intact, logits those of yr_forward."""
    import ctypes
    from yoloret_amd import runtime as rt
    name, size, b = 'mobilenetv2x75', 160, 3
    m = _model(name, size, 'f32')
    m.small_batch = m.mbk_batch = 0
    m.set_weights(synthetic_weights(m, 1234, 'conditioned'))
    xd = torch.from_numpy(params.synthetic_images(b, size, size)).to(dev)
    want = [y.cpu().numpy() for y in m(xd)]
    idx, hd = m._handle(xd.device, b)
    n = len(m.plan_for(b).ops)
    for entry in ('ranges', 'profile'):
        ws, ys = _fenced_buffers(m, xd, 0xFF, 0)
        mx, ms, names = (ctypes.c_float * n)(), (ctypes.c_float * n)(), (ctypes.c_char_p * n)()

        def call(moved):
            p = [rt._ptr(moved(t)) for t in [xd] + ys + [ws]]
            if entry == 'ranges':
                rt.check(rt.lib().yr_forward_ranges(hd, p[0], b, p[1], p[2], p[3], p[4], ws.numel(), rt.stream_ptr(dev), mx))
            else:
                rt.check(rt.lib().yr_forward_profile(hd, p[0], b, p[1], p[2], p[3], p[4], ws.numel(), rt.stream_ptr(dev), 1, ms, names))
        fence.run(call, writes=ys, reads=[xd], scratch=[ws], batch=b)
        torch.cuda.synchronize()
        for k, (y, w) in enumerate(zip(ys, want)):
            assert np.array_equal(y.cpu().numpy().reshape(w.shape), w), 'yr_forward_%s y%d differs from yr_forward' % (entry, k + 1)
        if entry == 'ranges':
            assert all(np.isfinite(v) and v >= 0 for v in mx) and max(mx) > 0


def test_se_tail_plan_clears_its_arrival_counters(dev, monkeypatch):
    """compiler.SE_TAIL (opt-in): the head ops finish their squeeze-excite block themselves and count arrivals in words behind the
    arena; poisoned counters (0xFFFFFFFF, 0x7B7B7B7B, random) must be cleared by the pass itself (runtime.hip: clear_sync)."""
    from yoloret_amd import compiler
    from yoloret_amd import runtime as rt
    monkeypatch.setattr(compiler, 'SE_TAIL', True)
    m, _ = _workspace_case(dev, 'mobilenetv2x75', 160, 'f32', 'throughput', 24)
    assert sum(1 for o in m.plan.ops if o.kind == rt.OP_HEAD and o.gate_out is not None) == 6
    assert m.workspace_bytes(24) > (m.plan.arena_bytes_per_image * 24 + 15) // 16 * 16      # the counters are there, and were poisoned


@pytest.mark.parametrize('name,dt,size,b', [('mobilenetv2x75', 'f32', 416, 64), ('efficientnetb0', 'bf16', 224, 8)])
def test_three_poisoned_contexts_in_flight_equal_the_serial_pass(dev, name, dt, size, b):
    """Three contexts of one Model, each workspace poisoned with a different pattern, in flight on three streams at once: every
    context's logits equal those of the serial pass (ctx 0) on the same input, bit for bit."""
    m = _model(name, size, dt)
    m.set_weights(synthetic_weights(m, 1234, 'survey'))          # (the bench's recipe)
    xd = torch.from_numpy(params.synthetic_images(b, size, size, seed=21)).to(dev)
    idx = xd.device.index
    want = [y.cpu().numpy() for y in m(xd)]
    for c in (1, 2, 3):
        m(xd, ctx=c)                        # allocates the contexts' workspaces
    torch.cuda.synchronize()
    for c, pat in zip((1, 2, 3), POISON_PATTERNS):
        poison_workspace(m, idx, c, pat, seed=c)
    outs = [nan_outputs(m, b) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in range(3)]
    got = []
    for c, st in zip((1, 2, 3), streams):
        with torch.cuda.stream(st):
            got.append(m(xd, out=outs[c - 1], ctx=c))
    torch.cuda.synchronize()
    for c, ys in zip((1, 2, 3), got):
        for k, (y, w) in enumerate(zip(ys, want)):
            a = y.cpu().numpy()
            assert np.isfinite(a).all() and np.array_equal(a, w), 'context %d (pattern %r) y%d differs from the serial pass' % (c, POISON_PATTERNS[c - 1], k + 1)


# ------------------------------------------------------------------ B. tuning table
B_CASES = [('mobilenetv2x75', 160, 'f32', 'throughput', 3), ('mobilenetv2x75', 416, 'f32', 'throughput', 64),
           ('mobilenetv2x75', 160, 'f32', 'nohead_k', 2), ('mobilenetv2x75', 160, 'f32', 'mid', 6),
           ('efficientnetb0-lite', 224, 'bf16', 'latency', 2), ('efficientnetb0', 224, 'bf16', 'throughput', 3),
           ('efficientnetb3-lite', 192, 'f16', 'throughput', 3)]


@pytest.mark.parametrize('name,size,dt,variant,b', B_CASES, ids=['%s-%d-%s-%s-b%d' % c for c in B_CASES])
def test_logits_do_not_depend_on_the_tuning_table(dev, monkeypatch, name, size, dt, variant, b):
    """From the all-zero table, one op at a time set to each entry yr_autotune dispatches for it: the logits must stay bit-identical.
    A YR_OP_MBH / YR_OP_MBX op runs the chained entries if it takes one (yr_mbh_prefers_chained: the register-chained form is built
    for its shape), the tile list otherwise.  Each tunable op must run at least one non-default entry."""
    from yoloret_amd import runtime as rt
    monkeypatch.setenv('YOLORET_AUTOTUNE', '0')
    m = _model(name, size, dt)
    assert not m.autotune
    if variant == 'throughput':
        m.small_batch = m.mbk_batch = 0
    else:
        _product_defaults(m, dt)
    assert m.variant(b) == variant
    m.set_weights(synthetic_weights(m, 1234, 'conditioned'))
    xd = torch.from_numpy(params.synthetic_images(b, size, size)).to(dev)
    m(xd)                                   # range guard (may move ops off the split forms: the plan is final after this call)
    plan = m.plan_for(b)
    n = len(plan.ops)
    zero = [0] * n
    m.set_tuning(b, zero)
    base = [y.clone() for y in m(xd)]
    torch.cuda.synchronize()
    assert all(torch.isfinite(y).all() for y in base)
    what = '%s@%d %s %s B=%d' % (name, size, dt, variant, b)

    def run(table):
        m.set_tuning(b, table)
        try:
            ys = m(xd)
            torch.cuda.synchronize()
        except rt.YoloretHipError as e:
            return str(e)
        return ys

    ran, refused, tried = {}, {}, 0
    for i, op in enumerate(plan.ops):
        cands = autotune_candidates(op)
        if not cands:
            continue
        if isinstance(cands[0], tuple):     # YR_OP_MBH / YR_OP_MBX
            chained, tiles = cands[0][1], cands[1][1]
            t = list(zero)
            t[i] = chained[0]
            cands = chained if not isinstance(run(t), str) else tiles
        ran[op.name] = 0
        for cfg in cands:
            t = list(zero)
            t[i] = cfg
            ys = run(t)
            tried += 1
            if isinstance(ys, str):
                refused.setdefault(op.name, []).append(cfg)
                continue
            ran[op.name] += 1
            for k, (y, y0) in enumerate(zip(ys, base)):
                assert torch.equal(y, y0), '%s: op %d %s (kind %d) entry %#x changes y%d (%d elements)' % (
                    what, i, op.name, op.kind, cfg, k + 1, int((y != y0).sum()))
        if op.name in refused:              # a refused entry leaves the handle as it was
            ys = run(zero)
            assert not isinstance(ys, str) and all(torch.equal(y, y0) for y, y0 in zip(ys, base)), '%s: after a refused entry of %s' % (what, op.name)
    print('%s: %d entries over %d tunable ops; refused at launch: %s' % (
        what, tried, len(ran), ', '.join('%s %s' % (k, [hex(c) for c in v]) for k, v in refused.items()) or 'none'))
    assert ran, '%s: no tunable op' % what
    idle = [k for k, v in ran.items() if v == 0]
    assert not idle, '%s: ops that ran no non-default entry: %s' % (what, idle)


# ------------------------------------------------------------------ C. every image of the bench batch
# BASELINE config 2 and bench.OTHER_CONFIGS, restated: (tag, model, size, batch, type)
C_CONFIGS = [('c2', 'mobilenetv2x75', 416, 64, 'f32'),
             ('c3', 'efficientnetb0-lite', 416, 128, 'bf16'), ('c4', 'mobilenetv2x14', 512, 64, 'f32'), ('c5', 'efficientnetb3-lite', 640, 32, 'f16'),
             ('c3_se', 'efficientnetb0', 416, 128, 'bf16'), ('c5_se', 'efficientnetb3', 640, 32, 'f16')]


@pytest.mark.parametrize('tag,name,size,b,dt', C_CONFIGS, ids=[c[0] for c in C_CONFIGS])
def test_every_image_of_the_bench_batch(dev, tag, name, size, b, dt):
    """The bench's plan at the bench's batch on a poisoned workspace into NaN outputs, then (i) every image run alone (the same plan:
    small_batch = mbk_batch = 0; its own poisoned workspace) equals its slot of the batch bit for bit, (ii) every image against the
    float32 oracle: 1e-4 (float32 plans) or the ceilings of the 16-bit plans - an image beyond them is checked against the NumPy
    emulation of the storage format for THAT image and must be no less accurate than it (a failure tied to a batch slot is a bug)."""
    from oracle import model as om
    from tests.util import entry_on_matrix_pipe
    m = _model(name, size, dt)
    m.small_batch = m.mbk_batch = 0
    P = params.ParamStore(1234, 'conditioned')
    x = params.synthetic_images(b, size, size)
    ref = _oracle(P, name, x)
    m.set_weights(P.values)
    xd = torch.from_numpy(x).to(dev)
    idx = xd.device.index
    m(xd)
    m(xd[:1].contiguous(), ctx=1)           # (autotunes batch 1, allocates its workspace)
    torch.cuda.synchronize()
    poison_workspace(m, idx, 0, 'random', seed=7)
    full = [y.cpu().numpy() for y in m(xd, out=nan_outputs(m, b))]
    torch.cuda.synchronize()
    assert all(np.isfinite(y).all() for y in full), tag
    for i in range(b):                      # (i)
        poison_workspace(m, idx, 1, POISON_PATTERNS[i % 3], seed=100 + i)
        one = m(xd[i:i + 1].contiguous(), out=nan_outputs(m, 1), ctx=1)
        for k, (a, f) in enumerate(zip(one, full)):
            assert np.array_equal(a[0].cpu().numpy(), f[i]), '%s: image %d, y%d differs between the batch-%d and the batch-1 run' % (tag, i, k + 1, b)
    emulated = []                           # (ii)
    for i in range(b):
        if dt == 'f32':
            for k, (y, r) in enumerate(zip(full, ref)):
                assert_close(y[i].reshape(r[i].shape), r[i], 1e-4, '%s image %d y%d' % (tag, i, k + 1))
            continue
        cm, ca = _ceil16()[(name, dt)]
        errs = [_errs(y[i].reshape(r[i].shape), r[i]) for y, r in zip(full, ref)]
        if all(gm <= cm and ga <= ca for gm, ga in errs):
            continue
        emulated.append(i)
        emu = om.yolov3_body(params.QuantStore(1234, 'conditioned', dt, round_entry=entry_on_matrix_pipe(m)), x[i:i + 1], name, 3, 20)
        for k, ((gm, ga), e, r) in enumerate(zip(errs, emu, ref)):
            em, ea = _errs(e, r[i:i + 1])
            print('%s image %d y%d  scaled error vs the fp32 oracle (max / mean): HIP %.2e / %.2e  emulation %.2e / %.2e' % (tag, i, k + 1, gm, ga, em, ea))
            assert gm <= max(cm, em) and ga <= max(ca, ea), '%s image %d y%d beyond the ceilings and the emulation of the format' % (tag, i, k + 1)
            assert ga <= 1.5 * ea + 1e-6 and gm <= 2.0 * em + 1e-5, '%s image %d y%d: less accurate than the emulation of the format' % (tag, i, k + 1)
    print('%s: %d images, batch-1 equal and within the bar; checked against the emulation: %s' % (tag, b, emulated or 'none'))


def test_bench_weights_on_the_bench_plan_vs_fp64(dev):
    """The bench's own weights (the 'survey' recipe, which amplifies rounding noise about 1e3 times: oracle/params.py) on the plan the
    bench times (config 2: the throughput plan at 64 images), every image against the float64 torch oracle: per image and output no
    less accurate than the float32 torch oracle (x1.5, floors 1e-5 max / 1e-6 mean) - the form of
    tests/test_gpu_graph.py::test_logits_survey_recipe_vs_fp64, which runs one image on a batch-1 plan."""
    name, size, b = 'mobilenetv2x75', 416, 64
    m = _model(name, size, 'f32')
    m.small_batch = m.mbk_batch = 0
    assert m.variant(b) == 'throughput'
    P = params.ParamStore(1234, 'survey')
    x = params.synthetic_images(b, size, size)
    ref64 = _oracle(P, name, x.astype(np.float64), dtype=torch.float64)
    ref32 = _oracle(P, name, x)
    m.set_weights(P.values)
    ys = [y.cpu().numpy() for y in m(torch.from_numpy(x).to(dev))]
    torch.cuda.synchronize()
    worst = 0.0
    for i in range(b):
        for k, (y, r32, r64) in enumerate(zip(ys, ref32, ref64)):
            den = np.maximum(1.0, np.abs(r64[i]))
            e_gpu = np.abs(y[i].reshape(r64[i].shape).astype(np.float64) - r64[i]) / den
            e_32 = np.abs(r32[i].astype(np.float64) - r64[i]) / den
            worst = max(worst, float(e_gpu.max()))
            assert e_gpu.max() <= 1.5 * e_32.max() + 1e-5, 'image %d y%d: max %.3e vs torch fp32 %.3e' % (i, k + 1, e_gpu.max(), e_32.max())
            assert e_gpu.mean() <= 1.5 * e_32.mean() + 1e-6, 'image %d y%d: mean %.3e vs torch fp32 %.3e' % (i, k + 1, e_gpu.mean(), e_32.mean())
    print('c2 survey weights, 64 images: worst scaled error vs fp64 %.2e' % worst)


# ------------------------------------------------------------------ D. the head-stream guard
def test_hoist_off_head_stream_plan(dev, monkeypatch):
    """With the up-sampling not hoisted (compiler.HOIST_UPSAMPLE = False) td3's head sees two up-sampled sources, which the
    weight-streaming head form does not gather: the compiler must not choose that form for it (it once did - a comment swallowed
    the guard - and yr_launch_head_stream refused the plan)."""
    from yoloret_amd import compiler
    monkeypatch.setattr(compiler, 'HOIST_UPSAMPLE', False)
    name, size, b = 'mobilenetv2x75', 96, 2
    m = _model(name, size, 'f32')
    P = params.ParamStore(1234, 'conditioned')
    x = params.synthetic_images(b, size, size)
    ref = _oracle(P, name, x)
    m.set_weights(P.values)
    assert m.variant(b) == 'throughput'
    ys = m(torch.from_numpy(x).to(dev))
    torch.cuda.synchronize()
    for k, (y, r) in enumerate(zip(ys, ref)):
        assert_close(y.cpu().numpy().reshape(r.shape), r, 1e-4, 'hoist off y%d' % (k + 1))
