"""Ingesting a batch of mixed-size images, timed at the size the ragged kernel is for: 64 synthetic images of VOC-like sizes
(500x375, 375x500, 500x333, ...) letterboxed to 416x416.

  (a) the per-image route YoloModel.call_packed took before: 64 pageable host-to-device copies and 64 runtime.letterbox launches;
  (b) the ragged route: pack images + geometry table into one pinned buffer (RaggedStager), one non-blocking copy, one
      runtime.ingest_batch launch - shown in parts (pack on the host, copy, kernel) and end to end;
  (c) for scale, a plain zero_() of the [64,416,416,3] float32 output.

Kernel parts are timed with HIP events around `--iters` calls after a warm-up, with the sources already on the device.  End-to-end
times are host wall clock from the decoded NumPy arrays to a device synchronise, (a) and (b) alternating `--rounds` times in
this process; the median and the smallest are printed.  Both routes must give the same bytes (checked first).  The table goes to
stdout and to --out.

    python tools/ingest_probe.py [--batch 64] [--size 416] [--iters 100] [--rounds 30] [--out profiles/r09_ingest_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import runtime as rt                                            # noqa: E402

VOC_SIZES = [(375, 500), (500, 375), (333, 500), (500, 333), (375, 500), (281, 500), (500, 400), (332, 500), (374, 500), (500, 334)]      # (h, w)


def timed(fn, iters, warmup=10):
    """microseconds per call by HIP events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def wall(fn):
    """microseconds of one call, host clock, ending in a device synchronise"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'ingest_probe.py needs a GPU'
    dev = torch.device('cuda:0')
    rt.lib()
    hw = (a.size, a.size)
    rs = np.random.RandomState(20240416)
    images = [rs.randint(0, 256, size=VOC_SIZES[i % len(VOC_SIZES)] + (3,)).astype(np.uint8) for i in range(a.batch)]
    mbytes_in = sum(im.nbytes for im in images) / 1e6
    mbytes_out = a.batch * a.size * a.size * 3 * 4 / 1e6
    lines = ['ingest_probe: %d images of VOC-like sizes (%.1f MB uint8) -> [%d,%d,%d,3] float32 (%.1f MB); %d timed calls per kernel item, %d '
             'alternating rounds end to end; microseconds' % (a.batch, mbytes_in, a.batch, a.size, a.size, mbytes_out, a.iters, a.rounds)]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    print(lines[0], flush=True)

    xa = torch.empty((a.batch, a.size, a.size, 3), dtype=torch.float32, device=dev)
    xb = torch.empty_like(xa)
    stager = rt.RaggedStager(dev)

    def route_a():
        for i, im in enumerate(images):
            rt.letterbox(torch.from_numpy(im).to(dev), hw, out=xa[i])

    def route_b():
        rt.ingest_batch(*stager.upload(images, hw, rt.INGEST_LETTERBOX), hw, out=xb)

    route_a()
    route_b()
    torch.cuda.synchronize()
    same = bool(torch.equal(xa.view(torch.int32), xb.view(torch.int32)))
    say('bytes of (a) and (b) equal: %s' % ('yes' if same else 'NO'))

    # kernel parts, sources resident
    resident = [torch.from_numpy(im).to(dev) for im in images]
    packed, table = stager.upload(images, hw, rt.INGEST_LETTERBOX)
    torch.cuda.synchronize()
    ka = timed(lambda: [rt.letterbox(r, hw, out=xa[i]) for i, r in enumerate(resident)], a.iters)
    kb = timed(lambda: rt.ingest_batch(packed, table, hw, out=xb), a.iters)
    kc = timed(lambda: xa.zero_(), a.iters)
    # the validation rule with 20 boxes per image in the same launch
    vpacked, vtable = rt.RaggedStager(dev).upload(images, hw, rt.INGEST_VALIDATE)
    boxes = torch.from_numpy(np.tile(np.array([[20, 30, 300, 280, 1]], np.float32), (a.batch, 20, 1))).to(dev)
    counts = torch.full((a.batch,), 20, dtype=torch.int32, device=dev)
    kv = timed(lambda: rt.ingest_batch(vpacked, vtable, hw, boxes=boxes, box_count=counts, out=xb), a.iters)
    # (b) in parts: pack on the host, the one copy
    pack_us = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        tab = rt.ingest_geometry([im.shape[:2] for im in images], hw, rt.INGEST_LETTERBOX)
        hv = stager._host.numpy()
        for im, off in zip(images, tab.host['src_off']):
            hv[off:off + im.size] = im.reshape(-1)
        pack_us.append((time.perf_counter() - t) * 1e6)
    total = table.packed_bytes + table.batch * 64
    dst = torch.empty(total, dtype=torch.uint8, device=dev)
    copy_pinned = timed(lambda: dst.copy_(stager._host[:total], non_blocking=True), a.iters, 3)
    copy_pageable = timed(lambda: [torch.from_numpy(im).to(dev) for im in images], max(a.iters // 5, 1), 2)
    # end to end, alternating
    for _ in range(3):
        wall(route_a)
        wall(route_b)
    ea, eb = [], []
    for _ in range(a.rounds):
        ea.append(wall(route_a))
        eb.append(wall(route_b))
    med = lambda v: float(np.median(v))
    say('(a) per-image route: %d letterbox launches, sources resident       %10.1f' % (a.batch, ka))
    say('    %d pageable copies alone (events)                               %10.1f' % (a.batch, copy_pageable))
    say('    end to end (wall clock, median / min)                           %10.1f / %.1f' % (med(ea), min(ea)))
    say('(b) ragged route: one ingest_batch launch, source resident          %10.1f   %.0f GB/s written' % (kb, mbytes_out * 1e3 / kb))
    say('    the same launch in VALIDATE mode with 20 boxes per image        %10.1f' % kv)
    say('    pack into the pinned buffer (host wall clock, median)           %10.1f' % med(pack_us))
    say('    the one pinned copy (events)                                    %10.1f   %.1f GB/s' % (copy_pinned, total / 1e3 / copy_pinned))
    say('    end to end (wall clock, median / min)                           %10.1f / %.1f' % (med(eb), min(eb)))
    say('(c) zero_() of the output                                           %10.1f   %.0f GB/s' % (kc, mbytes_out * 1e3 / kc))
    say('kernel (b) / (a) = %.3f   end to end (b) / (a) = %.3f   kernel (b) / (c) = %.2f' % (kb / ka, med(eb) / med(ea), kb / kc))
    say('condition: (b) not slower than (a), kernel part: %s; end to end: %s'
        % ('met' if kb <= ka else 'NOT met', 'met' if med(eb) <= med(ea) else 'NOT met'))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
