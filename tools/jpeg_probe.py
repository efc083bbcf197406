"""random_jpeg_quality on the device, timed at the size it is for: 64 synthetic images of VOC-like sizes through
get_random_data(train=True) to 416x416, then the JPEG round trip in place at qualities drawn from [80, 100).

  (1) runtime.jpeg_roundtrip_batch, canvas resident: both launches together (HIP events), and each kernel alone from a rocprofv3
      --kernel-trace --stats run of this tool (--stats-db; "not measured" without one);
  (2) the yardstick for its 27 bytes per pixel: launch 2 of yr_augment_batch (aug_finish_kernel: 24 bytes per pixel in place), from
      the same kernel trace, and a copy_() of the canvas (24 bytes per pixel, events);
  (3) runtime.augment_batch with and without the JPEG stage behind it (events).
The items alternate inside every round of one process; the figures are medians over --rounds.  The result is compared with
tests/jpeg_ref.py on the first two images (bit for bit) before anything is timed.  The table goes to stdout and to --out.

    rocprofv3 --kernel-trace --stats -d /tmp/jpeg_prof -o st -- python tools/jpeg_probe.py --kernels-only
    python tools/jpeg_probe.py --stats-db /tmp/jpeg_prof --out profiles/r12_jpeg_probe.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from yoloret_amd import build, runtime as rt                                     # noqa: E402
from augment_probe import VOC_SIZES                                              # noqa: E402

KERNELS = ('jpeg_code_kernel', 'jpeg_finish_kernel', 'aug_pixels_kernel', 'aug_finish_kernel')


def kernel_stats(path):
    """{kernel: (calls, average microseconds)} from the rocpd database(s) of a rocprofv3 --kernel-trace --stats run."""
    import glob
    import sqlite3
    out = {}
    dbs = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, '**', '*.db'), recursive=True))
    for db in dbs:
        try:
            rows = sqlite3.connect(db).execute('select name, count(*), avg(duration) from kernels group by name').fetchall()
        except sqlite3.Error:
            continue
        for name, calls, avg in rows:
            for key in KERNELS:
                if key in name:
                    out[key] = (int(calls), float(avg) / 1e3)
    return out


def one_round(items, iters):
    """{name: microseconds per call by HIP events}, the items one after the other"""
    out = {}
    for name, fn in items:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out[name] = t0.elapsed_time(t1) * 1e3 / iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--kernels-only', action='store_true', help='only launch the kernels (the run rocprofv3 traces)')
    ap.add_argument('--stats-db', default=None, help='the rocpd database (or its directory) of such a traced run')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'jpeg_probe.py needs a GPU'
    dev = torch.device('cuda:0')
    rt.lib()
    hw = (a.size, a.size)
    rs = np.random.RandomState(20240416)
    images = [rs.randint(0, 256, size=VOC_SIZES[i % len(VOC_SIZES)] + (3,)).astype(np.uint8) for i in range(a.batch)]
    draws = np.random.default_rng(11).random((a.batch, 10), dtype=np.float32)
    dims = [im.shape[:2] for im in images]
    pixels = a.batch * a.size * a.size
    out = torch.empty((a.batch, a.size, a.size, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(rt.augment_workspace_bytes(a.batch, hw), dtype=torch.uint8, device=dev)
    jws = torch.empty(rt.jpeg_workspace_bytes(a.batch, hw), dtype=torch.uint8, device=dev)
    quality = torch.from_numpy(np.random.default_rng((11, 1)).integers(80, 100, a.batch).astype(np.int32)).to(dev)
    packed, table = rt.RaggedStager(dev).upload_table(images, rt.augment_geometry(dims, hw, draws))
    rt.augment_batch(packed, table, hw, out=out, workspace=ws)
    canvas = out.clone()
    torch.cuda.synchronize()

    def jpeg():
        rt.jpeg_roundtrip_batch(out, quality, workspace=jws)

    def augment():
        rt.augment_batch(packed, table, hw, out=out, workspace=ws)

    def both():
        augment()
        jpeg()
    if a.kernels_only:
        for _ in range(a.iters):
            both()
        torch.cuda.synchronize()
        return
    from tests import jpeg_ref as jr
    both()
    got, qs = out[:2].cpu().numpy(), quality[:2].cpu().tolist()
    exact = all(np.array_equal(got[i].view(np.uint32), jr.roundtrip(canvas[i].cpu().numpy(), qs[i]).view(np.uint32)) for i in range(2))
    assert exact, 'the device result differs from tests/jpeg_ref.py'
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    say('jpeg_probe: %d images of VOC-like sizes -> [%d,%d,%d,3] float32 (%.1f MB), all augment stages, qualities uniform in [80, 100); '
        '%d calls per item and round, items alternating, median of %d rounds; microseconds'
        % (a.batch, a.batch, a.size, a.size, pixels * 12 / 1e6, a.iters, a.rounds))
    say('images 0 and 1 equal tests/jpeg_ref.py bit for bit at qualities %s' % qs)
    items = [('jpeg', jpeg), ('copy', lambda: out.copy_(canvas)), ('augment', augment), ('augment+jpeg', both)]
    one_round(items, 10)      # warm-up of every item
    rounds = [one_round(items, a.iters) for _ in range(a.rounds)]
    med = {k: float(np.median([r[k] for r in rounds])) for k, _ in items}
    lo = {k: min(r[k] for r in rounds) for k, _ in items}
    st = kernel_stats(a.stats_db) if a.stats_db else {}

    def trace(key):
        return ('%10.1f   (rocprofv3 kernel trace, average of %d)' % (st[key][1], st[key][0])) if key in st else 'not measured'
    say('(1) jpeg_roundtrip_batch, both launches, canvas resident (events)      %10.1f   min %.1f   %.0f GB/s over the %.0f MB it moves (27 B per pixel)'
        % (med['jpeg'], lo['jpeg'], pixels * 27 / 1e3 / med['jpeg'], pixels * 27 / 1e6))
    say('    launch 1, jpeg_code_kernel: steps a-g, 13.5 B per pixel            %s' % trace('jpeg_code_kernel'))
    say('    launch 2, jpeg_finish_kernel: steps h-j, 13.5 B per pixel          %s' % trace('jpeg_finish_kernel'))
    say('(2) yardstick, launch 2 of augment_batch (aug_finish_kernel, 24 B per pixel in place)   %s' % trace('aug_finish_kernel'))
    say('    copy_() of the canvas, 24 B per pixel (events)                     %10.1f   min %.1f   %.0f GB/s'
        % (med['copy'], lo['copy'], pixels * 24 / 1e3 / med['copy']))
    if 'aug_finish_kernel' in st and 'jpeg_code_kernel' in st and 'jpeg_finish_kernel' in st:
        say('    (1) / (2), kernel trace: (%.1f + %.1f) / %.1f = %.2f' % (st['jpeg_code_kernel'][1], st['jpeg_finish_kernel'][1], st['aug_finish_kernel'][1],
                                                                        (st['jpeg_code_kernel'][1] + st['jpeg_finish_kernel'][1]) / st['aug_finish_kernel'][1]))
    say('    (1) / copy_(), events: %.2f' % (med['jpeg'] / med['copy']))
    say('(3) augment_batch alone (events)                                       %10.1f   min %.1f' % (med['augment'], lo['augment']))
    say('    augment_batch, then jpeg_roundtrip_batch (events)                  %10.1f   min %.1f   + %.1f, x %.2f'
        % (med['augment+jpeg'], lo['augment+jpeg'], med['augment+jpeg'] - med['augment'], med['augment+jpeg'] / med['augment']))
    say('kernel resources (the compiler\'s report):')
    for name, vg, sc, occ, lds in build.kernel_resources()['jpeg.hip']:
        say('    %-40s vgprs %3d scratch %d waves/SIMD %d lds %d' % (name, vg, sc, occ, lds))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
