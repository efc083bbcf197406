"""The training data transform, timed at the size it is for: 64 synthetic images of VOC-like sizes (500x375, 375x500, ...) through
get_random_data(train=True) to 416x416 with all stages on and 20 boxes per image.

  (a) runtime.augment_batch, source and table resident: both launches together (HIP events), and each kernel alone from a
      rocprofv3 --kernel-trace --stats run of this tool (--stats-db; "not measured" without one);
  (b) for comparison, runtime.ingest_batch in VALIDATE mode on the same batch with the same boxes, and a plain zero_() of the
      [64,416,416,3] float32 output;
  (c) end to end from the decoded NumPy arrays: geometry, pack, one pinned copy, both launches, a device synchronise (host wall
      clock, median / min of --rounds);
  (d) what is replaced: the host restatement tests/augment_ref.py per image (NumPy float32: resize, hue, saturation, pow, contrast);
  (e) for context, the host JPEG decode (PIL) of the committed VOC demo images, which none of the above contains.
The deviation of the device result from the float64 evaluation on the unit tests' inputs is repeated from
tests/test_gpu_augment.py::test_all_stages_against_float64.  The table goes to stdout and to --out.

    rocprofv3 --kernel-trace --stats -d /tmp/aug_prof -o st -- python tools/augment_probe.py --kernels-only
    python tools/augment_probe.py --stats-db /tmp/aug_prof --out profiles/r11_augment_probe.txt
"""
import argparse
import glob
import os
import sqlite3
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def kernel_stats(path):
    """{kernel name prefix: (calls, average microseconds)} from the rocpd database(s) of a rocprofv3 --kernel-trace --stats run."""
    out = {}
    dbs = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, '**', '*.db'), recursive=True))
    for db in dbs:
        try:
            rows = sqlite3.connect(db).execute('select name, count(*), avg(duration) from kernels group by name').fetchall()
        except sqlite3.Error:
            continue
        for name, calls, avg in rows:
            for key in ('aug_pixels_kernel', 'aug_finish_kernel', 'ingest_kernel'):
                if key in name:
                    out[key] = (int(calls), float(avg) / 1e3)
    return out


def unit_deviation(dev):
    """(canvas, E_ref, device deviation) on the inputs of tests/test_gpu_augment.py, all stages on."""
    from tests import augment_cases as ac, augment_ref as ar
    rows = []
    for size in ac.CANVASES:
        geo = ac.geometries(size, 15)
        w64 = [ar.image(im, size, g, 15, np.float64) for im, g in zip(ac.images(), geo)]
        w32 = [ar.image(im, size, g, 15) for im, g in zip(ac.images(), geo)]
        packed, table = rt.RaggedStager(dev).upload_table(ac.images(), rt.augment_geometry(ac.SOURCES, size, ac.DRAWS))
        got = rt.augment_batch(packed, table, size).cpu().numpy()
        rows.append((size, max(float(np.abs(a - b).max()) for a, b in zip(w32, w64)),
                     max(float(np.abs(got[i] - w64[i]).max()) for i in range(len(w64)))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--host-images', type=int, default=4, help='images the host restatement is timed on')
    ap.add_argument('--kernels-only', action='store_true', help='only launch the kernels (the run rocprofv3 traces)')
    ap.add_argument('--stats-db', default=None, help='the rocpd database (or its directory) of such a traced run')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'augment_probe.py needs a GPU'
    dev = torch.device('cuda:0')
    rt.lib()
    hw = (a.size, a.size)
    rs = np.random.RandomState(20240416)
    images = [rs.randint(0, 256, size=VOC_SIZES[i % len(VOC_SIZES)] + (3,)).astype(np.uint8) for i in range(a.batch)]
    draws = np.random.default_rng(11).random((a.batch, 10), dtype=np.float32)
    dims = [im.shape[:2] for im in images]
    mbytes_out = a.batch * a.size * a.size * 3 * 4 / 1e6
    boxes = torch.from_numpy(np.tile(np.array([[20, 30, 300, 280, 1]], np.float32), (a.batch, 20, 1))).to(dev)
    counts = torch.full((a.batch,), 20, dtype=torch.int32, device=dev)
    out = torch.empty((a.batch, a.size, a.size, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(rt.augment_workspace_bytes(a.batch, hw), dtype=torch.uint8, device=dev)
    stager = rt.RaggedStager(dev)
    packed, table = stager.upload_table(images, rt.augment_geometry(dims, hw, draws))
    vpacked, vtable = rt.RaggedStager(dev).upload(images, hw, rt.INGEST_VALIDATE)
    npacked, ntable = rt.RaggedStager(dev).upload_table(images, rt.augment_geometry(dims, hw, draws, cont=0))
    torch.cuda.synchronize()

    def full():
        rt.augment_batch(packed, table, hw, boxes=boxes, box_count=counts, out=out, workspace=ws)

    def validate():
        rt.ingest_batch(vpacked, vtable, hw, boxes=boxes, box_count=counts, out=out)
    if a.kernels_only:
        for _ in range(a.iters):
            full()
            validate()
        torch.cuda.synchronize()
        return

    lines = ['augment_probe: %d images of VOC-like sizes (%.1f MB uint8) -> [%d,%d,%d,3] float32 (%.1f MB), all stages, 20 boxes per image; '
             '%d timed calls per kernel item, %d rounds end to end; microseconds'
             % (a.batch, sum(im.nbytes for im in images) / 1e6, a.batch, a.size, a.size, mbytes_out, a.iters, a.rounds)]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    print(lines[0], flush=True)
    ka = timed(full, a.iters)
    kn = timed(lambda: rt.augment_batch(npacked, ntable, hw, boxes=boxes, box_count=counts, out=out, workspace=ws), a.iters)
    kv = timed(validate, a.iters)
    kz = timed(lambda: out.zero_(), a.iters)
    say('(a) augment_batch, both launches, source resident (events)           %10.1f   %.0f GB/s over the %.0f MB the in-place form moves'
        % (ka, 3 * mbytes_out * 1e3 / ka, 3 * mbytes_out))
    st = kernel_stats(a.stats_db) if a.stats_db else {}
    for key, what in (('aug_pixels_kernel', 'launch 1, aug_pixels_kernel: pixels through gamma, channel sums'),
                      ('aug_finish_kernel', 'launch 2, aug_finish_kernel: contrast and clip in place, boxes  ')):
        if key in st:
            say('    %s  %10.1f   (rocprofv3 kernel trace, average of %d)' % (what, st[key][1], st[key][0]))
        else:
            say('    %s  not measured' % what)
    say('    contrast stage off: launch 1 clips, launch 2 only boxes (events)  %10.1f' % kn)
    say('(b) ingest_batch, VALIDATE mode, same batch and boxes (events)        %10.1f%s'
        % (kv, ('   kernel trace %.1f' % st['ingest_kernel'][1]) if 'ingest_kernel' in st else ''))
    say('    zero_() of the output (events)                                    %10.1f   %.0f GB/s' % (kz, mbytes_out * 1e3 / kz))

    def end_to_end():
        p, t = stager.upload_table(images, rt.augment_geometry(dims, hw, draws))
        rt.augment_batch(p, t, hw, boxes=boxes, box_count=counts, out=out, workspace=ws)
    for _ in range(3):
        wall(end_to_end)
    ee = [wall(end_to_end) for _ in range(a.rounds)]
    say('(c) end to end from decoded arrays: geometry, pack, copy, launches    %10.1f / %.1f  (wall clock, median / min; %.1f per image)'
        % (float(np.median(ee)), min(ee), float(np.median(ee)) / a.batch))
    from tests import augment_ref as ar
    host = []
    for i in range(min(a.host_images, a.batch)):
        t = time.perf_counter()
        ar.image(images[i], hw, ar.geometry(dims[i][0], dims[i][1], hw, draws[i]), 15)
        host.append((time.perf_counter() - t) * 1e6)
    say('(d) the host restatement (NumPy float32), per image                   %10.1f  (median of %d images; x %d images = %.0f)'
        % (float(np.median(host)), len(host), a.batch, float(np.median(host)) * a.batch))
    say('augment / validate = %.2f   augment / zero_() = %.2f   host restatement of the batch / (c) = %.0f'
        % (ka / kv, ka / kz, float(np.median(host)) * a.batch / float(np.median(ee))))
    say('launch 1 alone by stage mask (contrast off, no boxes: one launch; events):')
    for mask, what in ((0, 'resize, crop, pad, flip, clip'), (rt.AUG_HUE | rt.AUG_SAT, '+ hue, saturation'), (rt.AUG_GAMMA, '+ gamma (three powf per pixel)'),
                       (rt.AUG_HUE | rt.AUG_SAT | rt.AUG_GAMMA, '+ hue, saturation, gamma')):
        mp, mt = rt.RaggedStager(dev).upload_table(images, rt.augment_geometry(dims, hw, draws, stages=mask))
        torch.cuda.synchronize()
        say('    %-40s %10.1f' % (what, timed(lambda: rt.augment_batch(mp, mt, hw, out=out, workspace=ws), a.iters)))
    say('The recompute form (launch 2 recomputes the pixel instead of reading launch 1\'s back) was not built: it would run launch 1\'s '
        'arithmetic a second time to save launch 2\'s traffic; compare the two launches above.')
    from yoloret_amd.yolo3.data import decode_image
    jpegs = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'demo_*.jpg')))
    dec = []
    for _ in range(5):
        for p in jpegs:
            t = time.perf_counter()
            decode_image(p)
            dec.append((time.perf_counter() - t) * 1e6)
    say('(e) cost context, in no line above: the host JPEG decode (PIL) of the %d committed VOC demo images, per image  %10.1f  (median; x %d = %.0f): '
        'it dominates a real epoch' % (len(jpegs), float(np.median(dec)), a.batch, float(np.median(dec)) * a.batch))
    say('deviation from the float64 evaluation on the unit tests\' inputs (tests/test_gpu_augment.py), all stages on:')
    for size, e_ref, err in unit_deviation(dev):
        say('    canvas %2dx%-2d  E_ref (float32 restatement) %.3e   device %.3e   bound max(4 E_ref, 4 * 2^-24) %.3e'
            % (size[0], size[1], e_ref, err, max(4 * e_ref, 4 * 2.0 ** -24)))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
