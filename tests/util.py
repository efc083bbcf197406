"""Shared helpers for the parity tests (host<->device staging, tolerances)."""
import numpy as np
import torch

ANCHORS = np.array([10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326],
                   np.float32).reshape(-1, 2)


def round_up(v, m):
    return (v + m - 1) // m * m


def to_dev(a, dev, ld=None, fill=np.nan):
    """[B,H,W,C] numpy -> device tensor [B,H,W,ld]; pad channels are filled with NaN by default so
    that any kernel that lets padding leak into results fails loudly."""
    a = np.asarray(a, np.float32)
    c = a.shape[-1]
    ld = round_up(c, 4) if ld is None else ld
    if ld != c:
        p = np.full(a.shape[:-1] + (ld,), fill, np.float32)
        p[..., :c] = a
        a = p
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def from_dev(t, c=None):
    a = t.detach().cpu().numpy()
    return a if c is None else a[..., :c]


def assert_close(got, ref, tol=1e-4, what=''):
    """|got-ref| <= tol*max(1,|ref|) elementwise (SURVEY.md H3 form of the 1e-4 logits bar)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert np.isfinite(got).all(), '%s: non-finite values in result' % what
    m = float(err.max()) if err.size else 0.0
    assert m <= tol, '%s: max scaled error %.3e > %.1e at %s' % (what, m, tol, np.unravel_index(err.argmax(), err.shape))
    return m


# ---- 16-bit storage (bfloat16 / float16) helpers shared by the reduced-precision tests
REL = {'bf16': 2.0 ** -8, 'f16': 2.0 ** -11}     # half an ulp, relative (normal range)
TINY = {'bf16': 1e-30, 'f16': 2.0 ** -25}        # half an ulp in the subnormal range of float16


def _rt():
    from yoloret_amd import runtime as rt
    return rt


def q16(a, dt):
    """float32 array rounded to the 16-bit type and widened back."""
    rt = _rt()
    a = np.ascontiguousarray(a, np.float32)
    return rt.from_bits16(rt.to_bits16(a, dt), dt).reshape(a.shape)


def to_dev16(a, dev, dt, ld=None, poison=True):
    """[..., C] float32 (values representable in dt) -> device tensor [..., ld] of the 16-bit type; pad channels NaN."""
    rt = _rt()
    a = np.asarray(a, np.float32)
    c = a.shape[-1]
    ld = round_up(c, 8) if ld is None else ld
    if ld != c:
        p = np.full(a.shape[:-1] + (ld,), np.nan if poison else 0.0, np.float32)
        p[..., :c] = a
        a = p
    bits = rt.to_bits16(a, dt).reshape(a.shape)
    t = torch.from_numpy(bits.view(np.int16)).to(dev)
    return t.view(rt.TORCH_DTYPE[rt.dtype_id(dt)])


def from_dev16(t, dt, c=None):
    rt = _rt()
    a = rt.from_bits16(t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16), dt).reshape(tuple(t.shape))
    return a if c is None else a[..., :c]


def assert_rounded_once(got, ref64, dt, what, slack=2e-5):
    """|got - ref| <= half ulp_dt(ref) (x1.02) + slack*max(1,|ref|): one rounding of a float32-accurate value."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref64, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), '%s: non-finite values' % what
    tol = 1.02 * REL[dt] * np.abs(ref) + TINY[dt] + slack * np.maximum(1.0, np.abs(ref))
    bad = np.abs(got - ref) > tol
    assert not bad.any(), '%s: %d of %d beyond half an ulp; worst |d|/tol = %.2f' % (
        what, bad.sum(), bad.size, float((np.abs(got - ref) / tol).max()))


def entry_on_matrix_pipe(model):
    """Whether the plan's network entry takes image and stem kernel as 16-bit MFMA operands (stemblock_h.hip: a STEMBLOCK op in
    the matrix-pipe layout, which carries BN `scale` rows, or the stem + depthwise entry asked for in its matrix-pipe form, rt.STEMBLOCK_ENTRY_MFMA in k) - what QuantStore(round_entry=...) must emulate for this plan."""
    rt = _rt()
    op = model.plan.ops[0]
    return model.plan.dtype != 0 and op.kind == rt.OP_STEMBLOCK and ('scale' in op.params or (op.k & rt.STEMBLOCK_ENTRY_MASK) >> rt.STEMBLOCK_ENTRY_SHIFT == rt.STEMBLOCK_ENTRY_MFMA)


# ---- whole-plan invariance helpers (tests/test_gpu_invariance.py)
# Byte patterns a workspace is poisoned with: 0xFF is a NaN in float32, float16 and bfloat16; 0x7B a large finite value in all three
# (float16 61280, float32 / bfloat16 about 1.3e36); 'random' seeded random bytes (any mixture of the above, subnormals, infinities).
POISON_PATTERNS = (0xFF, 0x7B, 'random')


def poison_workspace(model, device_index, ctx=0, pattern=0xFF, seed=0):
    """Fills the WHOLE workspace tensor of execution context `ctx` (Model.__call__: `_workspace[idx]`, or `[(idx, ctx)]` for ctx > 0)
    with one byte pattern - the arena, its unwritten padding lanes and the squeeze-excite arrival counters behind it (which the runtime
    clears at the start of every pass).  Enqueued on the current stream."""
    ws = model._workspace[device_index if ctx == 0 else (device_index, ctx)]
    if pattern == 'random':
        g = torch.Generator(device=ws.device)
        g.manual_seed(seed)
        ws.random_(0, 256, generator=g)
    else:
        ws.fill_(int(pattern))
    return ws


def nan_outputs(model, b):
    """float32 output tensors for a batch of `b` images filled with NaN, for Model.__call__(x, out=...): an output element a plan
    does not write stays NaN."""
    dev = torch.device('cuda', torch.cuda.current_device())
    return [torch.full((b, ob.h, ob.w, ob.c), float('nan'), dtype=torch.float32, device=dev) for ob in model.plan.output_bufs]


# ---- yr_autotune's candidate lists (yoloret_amd/csrc/runtime.hip), restated: tests/test_host_logic.py checks them against the source.
# Only these entries are dispatched by the tuner, so only these are what a tuning table can hold in practice.
AUTOTUNE_MBH_TILES = [(4, 8), (8, 4), (7, 4), (7, 8), (8, 8), (13, 4), (4, 16), (8, 16), (7, 16), (13, 8),
                      (16, 8), (13, 16), (8, 12), (7, 12), (13, 12), (16, 12), (16, 16), (4, 12), (6, 8)]     # (th, tw)
AUTOTUNE_MBH_CHAINED = [(_rt().MBH_TILE_CHAINED, s) for s in (1, 2, 3, 4, 6)]    # the register-chained form: (forced tile, row segments)
AUTOTUNE_MBR_SEGS = [0, 1, 2, 3, 4, 6, 8, 13, 18, 26]                           # row segments per strip of YR_OP_MBR / YR_OP_MBE
PW_NUM_CFGS = {0: 29, 1: 26, 2: 26}        # == yr_pointwise_num_cfgs(dtype): entries 0 .. n are valid for a pointwise op


def autotune_candidates(op):
    """The non-default tuning entries yr_autotune times for plan op `op` ([] for an op it does not tune).  For YR_OP_MBH / YR_OP_MBX
    both lists are returned as ('chained', [...]) / ('tiles', [...]): which one applies (yr_mbh_prefers_chained) is the library's
    choice by shape, which the caller finds by whether the op takes a chained entry."""
    rt = _rt()
    if op.kind == rt.OP_POINTWISE:
        if op.dtype == 0 and op.se_reduced & rt.PWF_STATIONARY:       # the pixel-stationary form: nothing to tune
            return []
        return list(range(1, PW_NUM_CFGS[op.dtype] + 1))
    if op.kind == rt.OP_MBR and op.k & rt.MBR_STREAM:                # the weight-streaming block form: nothing to tune
        return []
    if op.kind in (rt.OP_MBR, rt.OP_MBE):
        base = op.k & (rt.MBR_FORM_MASK | rt.MBR_NW_MASK)
        return [(base & rt.MBR_NW_MASK) | (s << rt.MBR_SEGS_SHIFT) for s in AUTOTUNE_MBR_SEGS if 0 < s <= op.h]
    if op.kind in (rt.OP_MBH, rt.OP_MBX):
        return [('chained', [th << rt.MBH_TH_SHIFT | tw << rt.MBH_TW_SHIFT for th, tw in AUTOTUNE_MBH_CHAINED]),
                ('tiles', [th << rt.MBH_TH_SHIFT | tw << rt.MBH_TW_SHIFT for th, tw in AUTOTUNE_MBH_TILES])]
    return []
