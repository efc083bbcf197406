"""Where the loss's labels come from, timed at the size the encoder is for: 64 images at 416, 20 rows per image, C = 20 and C = 80.

  (a) the host path: preprocess_true_boxes per image (wall clock), np.stack, then .to(device) of the three tensors from pageable
      and from pinned memory;
  (b) runtime.encode_labels (zero-fill + scatter: two launches);
  (c) zeroing the same three tensors: hipMemsetAsync, and tensor.zero_();
  (d) an empty two-launch pair: the same entry on the smallest input there is (one image, one row, 32 x 32, C = 0 - 315 floats);
  (e) one batch-64 detection step (DetectionPipeline: network, decode, NMS, records), for scale.

Device items are timed with HIP events around `--iters` calls after a warm-up, all in this process, one after the other; the
table goes to stdout and to --out.  The target of (b) is 1.25 x ((c) + (d)) with (c) the faster of its two forms.

    python tools/labels_probe.py [--batch 64] [--iters 100] [--out profiles/r08_labels_probe.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import runtime as rt                                            # noqa: E402
from yoloret_amd.yolo3.utils import get_anchors, preprocess_true_boxes           # noqa: E402


def random_boxes(rs, batch, rows, size, classes):
    out = np.zeros((batch, rows, 5), np.float32)
    for i in range(batch):
        n = rs.randint(1, rows + 1)
        w = np.clip(np.round(np.exp(rs.uniform(0, np.log(size), n))), 1, size)
        h = np.clip(np.round(np.exp(rs.uniform(0, np.log(size), n))), 1, size)
        x0, y0 = np.floor(rs.rand(n) * (size - w + 1)), np.floor(rs.rand(n) * (size - h + 1))
        out[i, :n] = np.stack([x0, y0, x0 + w, y0 + h, rs.randint(0, classes, n)], -1)
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--rows', type=int, default=20)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--host-iters', type=int, default=5)
    ap.add_argument('--no-detection', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'labels_probe.py needs a GPU'
    dev = torch.device('cuda:0')
    anchors = get_anchors('model_data/yolo_anchors.txt')
    rt.lib()
    # the HIP runtime this process already runs on (torch's and the library's), not a second copy found by name
    mapped = sorted({line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line})
    if not mapped:
        sys.exit('labels_probe.py: no libamdhip64 is mapped into this process - is this a ROCm build of torch?')
    hip = ctypes.CDLL(mapped[0])
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hw = (a.size, a.size)
    lines = ['labels_probe: batch %d, %dx%d, %d rows per image, %d timed calls per item; microseconds per call' % (a.batch, a.size, a.size, a.rows, a.iters)]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    print(lines[0], flush=True)

    tiny = torch.zeros((1, 1, 5), dtype=torch.float32, device=dev)
    tiny_out = rt.encode_labels(tiny, (32, 32), anchors, 0, 3)
    pair = timed(lambda: rt.encode_labels(tiny, (32, 32), anchors, 0, 3, out=tiny_out), a.iters)
    say('(d) empty two-launch pair (1 image, 1 row, 32x32, C=0)        %10.1f' % pair)

    for classes in (20, 80):
        boxes = random_boxes(np.random.RandomState(classes), a.batch, a.rows, a.size, classes)
        # (a) the host path
        t = time.perf_counter()
        for _ in range(a.host_iters):
            per_image = [preprocess_true_boxes(tb, hw, anchors, classes, 3) for tb in boxes]
        encode_us = (time.perf_counter() - t) * 1e6 / a.host_iters
        t = time.perf_counter()
        for _ in range(a.host_iters):
            host = [np.stack([p[s] for p in per_image]) for s in range(3)]
        stack_us = (time.perf_counter() - t) * 1e6 / a.host_iters
        mbytes = sum(h.nbytes for h in host) / 1e6
        pageable = [torch.from_numpy(h) for h in host]
        pinned = [p.pin_memory() for p in pageable]
        out = [torch.empty(p.shape, dtype=torch.float32, device=dev) for p in pageable]
        copy_pageable = timed(lambda: [o.copy_(p) for o, p in zip(out, pageable)], a.iters, 3)
        copy_pinned = timed(lambda: [o.copy_(p, non_blocking=True) for o, p in zip(out, pinned)], a.iters, 3)
        # (b) the device path
        tb = torch.from_numpy(boxes).to(dev)
        skipped = torch.empty((a.batch,), dtype=torch.int32, device=dev)
        enc = timed(lambda: rt.encode_labels(tb, hw, anchors, classes, 3, out=out, skipped=skipped), a.iters)
        same = all(np.array_equal(o.cpu().numpy().view(np.uint32), h.view(np.uint32)) for o, h in zip(out, host)) and not skipped.any().item()
        # (c) zeroing alone
        stream = rt.stream_ptr(dev)

        def memset():
            for o in out:
                assert hip.hipMemsetAsync(o.data_ptr(), 0, o.numel() * 4, stream) == 0
        ms = timed(memset, a.iters)
        zero = timed(lambda: [o.zero_() for o in out], a.iters)
        c = min(ms, zero)
        say('--- C = %d: three tensors of %.1f MB' % (classes, mbytes))
        say('(a) host preprocess_true_boxes x %d (wall clock)               %10.1f' % (a.batch, encode_us))
        say('    np.stack of the three scales (wall clock)                  %10.1f' % stack_us)
        say('    .to(device) from pageable memory                           %10.1f' % copy_pageable)
        say('    .to(device) from pinned memory                             %10.1f' % copy_pinned)
        say('    (a) in all, pageable / pinned                              %10.1f / %.1f' % (encode_us + stack_us + copy_pageable, encode_us + stack_us + copy_pinned))
        say('(b) encode_labels (bytes equal to the host path: %s)          %10.1f   %.0f GB/s of zeros' % ('yes' if same else 'NO', enc, mbytes * 1e3 / enc))
        say('(c) hipMemsetAsync x 3                                         %10.1f' % ms)
        say('    tensor.zero_() x 3                                         %10.1f' % zero)
        say('    (b) / ((c) + (d)) = %.2f  (target: at most 1.25)            (a) / (b) = %.0f pageable, %.0f pinned'
            % (enc / (c + pair), (encode_us + stack_us + copy_pageable) / enc, (encode_us + stack_us + copy_pinned) / enc))
        del pageable, pinned, out, host, per_image

    if not a.no_detection:
        from yoloret_amd import layers as L, weights as W
        from yoloret_amd.pipeline import DetectionPipeline
        from yoloret_amd.yolo3.model import yolov3_body
        model = yolov3_body(L.Input(shape=[a.size, a.size, 3]), 'mobilenetv2x75', 3, num_classes=20)
        model.set_weights(W.synthetic_weights(model, 1234, 'survey'))
        pipe = DetectionPipeline(model, anchors, 20, 3, max_boxes=20, score_threshold=0.2, iou_threshold=0.5)
        x = torch.from_numpy(W.synthetic_images(a.batch, a.size, a.size, seed=20240416)).to(dev)
        image_hw = torch.tensor([[a.size, a.size]] * a.batch, dtype=torch.int32, device=dev)
        step = timed(lambda: pipe(x, image_hw), a.iters, 5)
        say('(e) one detection step, mobilenetv2x75 float32, batch %d      %10.1f' % (a.batch, step))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
