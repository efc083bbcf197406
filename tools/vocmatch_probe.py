"""The device matcher (yr_voc_match, csrc/vocmatch.hip) stand-alone at the sizes it is built for, next to its yardstick: the
batch-64 detection step (forward + decode + NMS + pack) of the flagship model, timed in the same run.

    python tools/vocmatch_probe.py [--batch 64] [--iters 200] [--repeats 7] [--no-step]

One voc_match call (one launch) is timed with device events: warm-up, `iters` calls between two events, median of `repeats`.
Shapes: C=20 rows=400 and C=80 rows=1600 (max_boxes = 20), each with about 10 and about 60 ground-truth boxes per image, and
with every row of an image valid (the worst case of the O(n^2) ranking) and with a quarter of them valid.  A detection is a
jitter of a labelled box of its own class, so boxes are claimed; scores are random.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import runtime as rt                      # noqa: E402


def records(batch, classes, rows, ngt, fill, seed):
    rs = np.random.RandomState(seed)
    det = np.full((batch, rows, 6), -77, np.int32)
    cnt = np.full((batch,), int(rows * fill), np.int32)
    gt = np.zeros((batch, ngt + 8, 5), np.float32)
    gcnt = rs.randint(max(ngt - 8, 1), ngt + 9, batch).astype(np.int32)
    for b in range(batch):
        g = gcnt[b]
        xy = rs.randint(0, 330, (g, 2))
        wh = rs.randint(10, 80, (g, 2))
        gt[b, :g] = np.concatenate([xy, xy + wh, rs.randint(0, classes, (g, 1))], axis=1)
        n = cnt[b]
        src = gt[b, rs.randint(0, g, n)]
        j = rs.randint(-4, 5, (n, 4))
        lo = src[:, :2].astype(np.int64) + j[:, :2]
        hi = np.maximum(src[:, 2:4].astype(np.int64) + j[:, 2:], lo)
        det[b, :n, 0], det[b, :n, 1], det[b, :n, 2], det[b, :n, 3] = lo[:, 1], lo[:, 0], hi[:, 1], hi[:, 0]
        det[b, :n, 4] = rs.rand(n).astype(np.float32).view(np.int32)
        det[b, :n, 5] = src[:, 4].astype(np.int32)
    return det, cnt, gt, gcnt


def median_us(fn, iters, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / iters)
    return float(np.median(times)), float(min(times)), float(max(times))


def detection_step(batch, dev, iters, repeats):
    from yoloret_amd import layers as L
    from yoloret_amd import weights as W
    from yoloret_amd.pipeline import DetectionPipeline
    from yoloret_amd.yolo3.model import yolov3_body
    from yoloret_amd.yolo3.utils import get_anchors
    anchors = get_anchors('model_data/yolo_anchors.txt')
    model = yolov3_body(L.Input(shape=[416, 416, 3]), 'mobilenetv2x75', 3, num_classes=20)
    model.set_weights(W.synthetic_weights(model, 1234, 'survey'))
    pipe = DetectionPipeline(model, anchors, 20, 3, max_boxes=20, score_threshold=0.2, iou_threshold=0.5)
    x = torch.from_numpy(W.synthetic_images(batch, 416, 416, seed=20240416)).to(dev)
    image_hw = torch.tensor([[416, 416]] * batch, dtype=torch.int32, device=dev)
    pipe(x, image_hw)          # allocation and tile autotuning
    torch.cuda.synchronize()
    return median_us(lambda: pipe(x, image_hw), iters, repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--no-step', action='store_true', help='skip the detection step (the yardstick)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'vocmatch_probe.py needs a GPU'
    dev = torch.device('cuda:0')
    step = None
    if not a.no_step:
        step = detection_step(a.batch, dev, max(a.iters // 10, 5), a.repeats)
        print('detection step  mobilenetv2x75 416 f32 B=%d (forward + decode + NMS + pack, one after the other): %9.1f us  (min %.1f, max %.1f)'
              % ((a.batch,) + step))
    for classes, rows in ((20, 400), (80, 1600)):
        for ngt in (10, 60):
            for fill in (1.0, .25):
                det, cnt, gt, gcnt = (torch.from_numpy(t).to(dev) for t in records(a.batch, classes, rows, ngt, fill, classes + ngt))
                flags, npos = rt.voc_match(det, cnt, gt, gcnt, classes)
                med, lo, hi = median_us(lambda: rt.voc_match(det, cnt, gt, gcnt, classes), a.iters, a.repeats)
                valid = flags >= 0
                print('voc_match  B=%d C=%2d rows=%4d valid rows=%4d  gt ~%2d : %8.1f us  (min %.1f, max %.1f)%s   true positives %d of %d, npos %d'
                      % (a.batch, classes, rows, int(cnt[0]), ngt, med, lo, hi, ('  = %.3f of the step' % (med / step[0])) if step else '',
                         int((flags == 1).sum()), int(valid.sum()), int(npos.sum())))


if __name__ == '__main__':
    main()
