"""Red zones around the tensors of a launch: shows WHERE a kernel touches memory, which the value checks of the suite cannot.

`run_op(op, batch, writes=[...], reads=[...])` launches one yr_op with every listed tensor moved into a backing allocation of the
form  guard | interior | guard : the interior is a byte copy of the tensor (a NaN pre-fill survives), the op's pointers are switched
to it for the launch and restored afterwards (also when the launch raises).  `run(call, writes, reads)` is the same for any entry
that takes plain pointers: `call(moved)` gets a function that maps a listed tensor to its interior.

* guard size, each side: max(64 KiB, the bytes of one image of the tensor) rounded up to 256 and capped at 32 MiB - one image is
  the granule by which a batch index can be wrong;
* guards of WRITTEN tensors hold seeded random bytes (a stray store of any constant, zero and NaN included, shows); guards of READ
  tensors hold one byte pattern per variant;
* after the launch every guard of every listed tensor is compared byte for byte with its pre-launch copy (a kernel writes to no
  input, so the guards of read tensors must be intact too).  All comparisons run on the tensors' device and are fetched together;
* the launch runs twice:
    variant A  interiors on a 256-byte boundary, read guards 0xFF (NaN in float32 / float16 / bfloat16),
    variant B  interiors 16 bytes past a 256-byte boundary (the weakest alignment include/yoloret_hip.h promises), read guards
               0x7B (a large finite value in all three types);
  both start from the same pre-launch bytes, the written interiors of A and B must be bitwise equal (a result that took a value
  from a read guard differs between the two), and the caller's tensors receive A's bytes, so the assertions of the calling test run
  on them unchanged;
* `cols=n` (for writes[0], or a sequence parallel to `writes` with None for "no check"): elements >= n of every row (last dimension)
  of that written tensor must keep their pre-launch bytes - for outputs whose row stride is wider than what the op may write.

`fence.run(..., scratch=[...])` takes workspaces: written tensors whose contents after the call are unspecified.  They get the
guards of written tensors, but are neither compared between the variants nor handed back.

What the fence cannot see:
* a write that lands beyond the guards (further than one image, or 64 KiB, from the tensor);
* a read outside a tensor whose value is discarded (multiplied away by a select, masked off, never used).

Device-agnostic: tensors are touched only through torch byte views and data_ptr(), and the launch is a parameter
(tests/test_fence_host.py plays the kernel on CPU tensors).
"""
import torch

MIN_GUARD = 64 << 10
MAX_GUARD = 32 << 20
VARIANTS = (('A', 0, 0xFF), ('B', 16, 0x7B))      # name, interior offset past a 256-byte boundary, byte of the read guards
# yr_op fields that hold a device pointer (yr_src pointers are op.src[i].ptr)
POINTER_FIELDS = ('out', 'gate', 'gate_out', 'sync', 'res', 'wgt', 'scale', 'shift', 'wgt2', 'b1', 'b2', 'se_w')


class FenceError(AssertionError):
    pass


def _nbytes(t):
    return t.numel() * t.element_size()


def guard_bytes(t, batch=None):
    img = _nbytes(t)
    if batch and t.dim() >= 1 and t.shape[0] == batch:
        img //= batch
    g = max(MIN_GUARD, img)
    return min((g + 255) // 256 * 256, MAX_GUARD)


def _key(t):
    return t.data_ptr(), _nbytes(t)


def _bytes(t):
    """flat uint8 view of a contiguous tensor"""
    return t.reshape(-1).view(torch.uint8)


class _Slot:
    """One listed tensor in one variant: its backing, the pre-launch copy and where the interior sits."""

    def __init__(self, t, role, written, batch, shift, read_byte, seed):
        if not t.is_contiguous():
            raise ValueError('fence: %s must be contiguous' % role)
        self.t, self.role, self.written = t, role, written
        self.n = _nbytes(t)
        g = guard_bytes(t, batch)
        total = g + self.n + g + 512
        if written:
            gen = torch.Generator(device=t.device)
            gen.manual_seed(seed)
            self.backing = torch.randint(0, 256, (total,), dtype=torch.uint8, device=t.device, generator=gen)
        else:
            self.backing = torch.full((total,), read_byte, dtype=torch.uint8, device=t.device)
        self.lo = g + (shift - self.backing.data_ptr() - g) % 256          # front guard: [0, lo), back guard: [lo + n, total)
        self.backing[self.lo:self.lo + self.n].copy_(_bytes(t))
        self.before = self.backing.clone()
        self.inner = self.backing[self.lo:self.lo + self.n].view(t.dtype).view(t.shape)
        assert self.inner.data_ptr() % 256 == shift

    def checks(self, cols):
        """[(what, changed flag, first, last)] as 0-dim device tensors; offsets are relative to the interior's first byte."""
        out = []
        hi = self.lo + self.n
        for side, a, b in (('before', 0, self.lo), ('after', hi, self.backing.numel())):
            out.append(('guard %s the tensor' % side, a - self.lo) + _span(self.backing[a:b], self.before[a:b]))
        if self.written and cols is not None:
            ld = self.t.shape[-1]
            if not 0 <= cols <= ld:
                raise ValueError('fence: cols=%d outside the row of %d elements of %s' % (cols, ld, self.role))
            es = self.t.element_size()
            now = self.backing[self.lo:hi].view(-1, ld * es)
            was = self.before[self.lo:hi].view(-1, ld * es)
            # offsets inside the interior: row * ld * es + column byte
            d = now[:, cols * es:] != was[:, cols * es:]
            idx = (torch.arange(now.shape[0], device=d.device)[:, None] * (ld * es)
                   + torch.arange(cols * es, ld * es, device=d.device)[None, :])
            out.append(('columns >= %d (the gap of each row)' % cols, 0) + _span_mask(d.reshape(-1), idx.reshape(-1)))
        return out


def _span_mask(d, idx):
    n = d.numel()
    if n == 0:
        z = torch.zeros((), dtype=torch.int64, device=d.device)
        return z, z, z
    big = torch.iinfo(torch.int64).max
    return (d.any().to(torch.int64), torch.where(d, idx, torch.full_like(idx, big)).min(),
            torch.where(d, idx, torch.full_like(idx, -big)).max())


def _span(now, was):
    d = now != was
    return _span_mask(d, torch.arange(d.numel(), device=d.device))


def _listed(writes, reads, cols, scratch=()):
    """[(tensor, written, cols, index in its list)] without duplicates (a tensor listed as written and read is written); scratch
    tensors follow the written ones."""
    writes, reads = list(writes) + list(scratch), list(reads)
    if cols is not None and not isinstance(cols, int):
        cols = list(cols) + [None] * len(list(scratch))
    if cols is None:
        cols = [None] * len(writes)
    elif isinstance(cols, int):
        cols = [cols] + [None] * (len(writes) - 1)
    cols = list(cols)
    if len(cols) != len(writes):
        raise ValueError('fence: cols must be one number (for writes[0]) or parallel to writes')
    seen, out = {}, []
    for written, ts, cs in ((True, writes, cols), (False, reads, [None] * len(reads))):
        for i, (t, c) in enumerate(zip(ts, cs)):
            if t is None:
                continue
            key = _key(t)
            if key in seen:
                continue
            seen[key] = True
            out.append((t, written, c, i))
    spans = sorted((t.data_ptr(), t.data_ptr() + _nbytes(t)) for t, _, _, _ in out if _nbytes(t))
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        if b0 < a1:
            raise ValueError('fence: two listed tensors overlap in memory; list the tensor that owns the bytes once')
    return out


def run(call, writes, reads=(), cols=None, batch=None, roles=None, scratch=()):
    """Runs `call(moved)` once per variant with every listed tensor relocated between guards; `moved(t)` is the interior that stands
    for listed tensor `t`.  Raises FenceError on a touched guard, a touched `cols` gap or a difference between the variants; else the
    written tensors hold variant A's bytes afterwards.  `roles(t)` names a tensor in messages.  `scratch`: workspaces - written
    tensors whose contents after the call are unspecified (a list in arrival order, tiles of a tuned shape): guarded like the
    written ones (random bytes, checked), but neither compared between the variants nor handed back."""
    listed = _listed(writes, reads, cols, scratch)
    unspecified = {_key(t) for t in scratch}
    pending, results = [], {}
    for vi, (vname, shift, read_byte) in enumerate(VARIANTS):
        slots = []
        for j, (t, written, c, i) in enumerate(listed):
            role = '%s[%d]' % ('writes' if written else 'reads', i)
            if roles is not None:
                role += ' (%s)' % roles(t)
            slots.append((_Slot(t, role, written, batch, shift, read_byte, seed=1000 * vi + j + 1), c))
        by_id = {_key(s.t): s for s, _ in slots}

        def moved(t, by_id=by_id):
            return by_id[_key(t)].inner
        call(moved)
        for s, c in slots:
            for what, base, flag, first, last in s.checks(c):
                pending.append(('variant %s: %s tensor %s: %s' % (vname, 'written' if s.written else 'read', s.role, what),
                                base, s.n, torch.stack([flag, first, last])))
        results[vname] = [(s.t, s.role, s.n, s.inner.clone()) for s, _ in slots if s.written and _key(s.t) not in unspecified]
        del slots, by_id
    for (_, role, n, a), (_, _, _, b) in zip(results['A'], results['B']):
        d = _bytes(a) != _bytes(b)
        pending.append(('written tensor %s: variant A (256-byte aligned, NaN around the sources) and variant B (16-byte aligned, large '
                        'finite values around the sources) differ in the interior' % role, 0, n,
                        torch.stack(_span_mask(d, torch.arange(d.numel(), device=d.device)))))
    if pending:
        devs = {p[3].device for p in pending}
        got = {d: torch.stack([p[3] for p in pending if p[3].device == d]).cpu() for d in devs}      # the one synchronise
        at = {d: 0 for d in devs}
        errors = []
        for what, base, n, v in pending:
            flag, first, last = got[v.device][at[v.device]].tolist()
            at[v.device] += 1
            if flag:
                errors.append('%s: bytes %+d .. %+d relative to the interior of %d bytes changed' % (what, first + base, last + base, n))
        if errors:
            raise FenceError('fence: ' + '; '.join(errors))
    for t, _, _, a in results['A']:
        _bytes(t).copy_(_bytes(a))


def _op_pointers(op):
    """[(name, getter, setter)] over the pointer fields of a yr_op"""
    out = []
    for f in POINTER_FIELDS:
        out.append((f, lambda f=f: getattr(op, f), lambda v, f=f: setattr(op, f, v)))
    for i in range(len(op.src)):
        out.append(('src[%d]' % i, lambda i=i: op.src[i].ptr, lambda v, i=i: setattr(op.src[i], 'ptr', v)))
    return out


def run_op(op, batch, writes, reads=(), cols=None, launch=None):
    """`launch(op, batch)` (default: yoloret_amd.runtime.run_op) between guards.  Each listed tensor is matched to the fields of `op`
    that point into it (out, gate, gate_out, sync, res, src[i].ptr and the weight pointers) by data_ptr(): fields that alias (the
    residual of an MBR block is its source) move together, a field that points inside a tensor keeps its offset.  A listed tensor
    that no field points into is an error of the calling test."""
    if launch is None:
        from yoloret_amd import runtime
        launch = runtime.run_op
    fields = _op_pointers(op)
    saved = [(setter, getter()) for _, getter, setter in fields]
    matches = {}
    for t, _, _, _ in _listed(writes, reads, cols):
        p, n = t.data_ptr(), max(_nbytes(t), 1)
        hit = [(name, setter, getter() - p) for name, getter, setter in fields if getter() is not None and p <= getter() < p + n]
        if not hit:
            raise ValueError('fence: a listed tensor of shape %s is not behind any pointer of the op' % (tuple(t.shape),))
        matches[_key(t)] = hit

    def call(moved):
        try:
            for t, _, _, _ in _listed(writes, reads, cols):
                for _, setter, off in matches[_key(t)]:
                    setter(moved(t).data_ptr() + off)
            launch(op, batch)
        finally:
            for setter, v in saved:
                setter(v)

    run(call, writes, reads, cols, batch, roles=lambda t: '+'.join(name for name, _, _ in matches[_key(t)]))
