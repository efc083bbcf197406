"""The output-layer training kernels stand-alone at the size they are built for: 64 images at 416 (grids 13 / 26 / 52, 75 -> 75
channels, 20 classes).  In ONE process, alternating round by round, the hipEvent time of, per scale,
    (i)   linear_wgrad       x and dy read once, two launches,
    (ii)  copy_() of a tensor of x's plus dy's size: the bytes (i) must read, through the copy engine of the framework
          (it also WRITES that many bytes, so it is an upper estimate of the time of reading them),
    (iii) linear_forward,
and once
    (iv)  adam_step over the three matrices (3 x 75 x 76 floats),
    (v)   OutputLayerTrainer.train_step next to the feature forward alone (mobilenetv2x75, random conditioned weights, four boxes
          per image).
The ratio (i) / (ii) is the yardstick: the gradient is bound by its reads, not by the matrix pipe.

    python tools/headtrain_probe.py [--batch 64] [--rounds 20] [--iters 20] [--out profiles/rNN_headtrain_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import layers as L, runtime as rt           # noqa: E402
from yoloret_amd.weights import synthetic_weights          # noqa: E402
from yoloret_amd.yolo3.model import yolov3_body            # noqa: E402
from yoloret_amd.yolo3.train import OutputLayerTrainer     # noqa: E402
from yoloret_amd.yolo3.utils import get_anchors            # noqa: E402


def timed(variants, rounds, iters):
    """-> (medians, minima) in us per call, the variants alternating round by round"""
    for v in variants:      # warm-up: code objects, allocator, autotune
        v()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(rounds):
        for k, v in enumerate(variants):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                v()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1e3 / iters)
    return [float(np.median(t)) for t in times], [float(np.min(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    anchors = get_anchors('model_data/yolo_anchors.txt')
    c = 3 * (5 + a.classes)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    lines = ['headtrain_probe: batch %d, 416x416, %d -> %d channels; %d rounds x %d calls, alternating; median (min) in us'
             % (a.batch, c, c, a.rounds, a.iters)]
    sums = np.zeros(3)
    for s in range(3):
        g = 416 // (32 >> s)
        x = torch.randn((a.batch, g, g, c), dtype=torch.float32, device=dev, generator=gen)
        dy = torch.randn((a.batch, g, g, c), dtype=torch.float32, device=dev, generator=gen)
        wt = torch.zeros((c, (c + 3) // 4 * 4), dtype=torch.float32, device=dev)
        wt[:, :c] = torch.randn((c, c), dtype=torch.float32, device=dev, generator=gen) / c ** .5
        pixels = a.batch * g * g
        ws = torch.empty(rt.linear_wgrad_workspace_bytes(pixels, c, c), dtype=torch.uint8, device=dev)
        dwt, y = torch.empty_like(wt), torch.empty_like(dy)
        src, dst = torch.empty(x.numel() + dy.numel(), dtype=torch.float32, device=dev), torch.empty(x.numel() + dy.numel(), dtype=torch.float32, device=dev)
        med, low = timed((lambda: rt.linear_wgrad(x, dy, out=dwt, workspace=ws), lambda: dst.copy_(src), lambda: rt.linear_forward(x, wt, out=y)),
                         a.rounds, a.iters)
        sums += med
        nbytes = (x.numel() + dy.numel()) * 4
        lines.append('scale %d (%dx%d, %d pixels, chunk %d, %d slabs): wgrad %.1f (%.1f)  copy_ of %.1f MB %.1f (%.1f)  ratio wgrad / copy_ %.3f, '
                     'reads at %.0f GB/s;  forward %.1f (%.1f)'
                     % (s, g, g, pixels, rt.linear_wgrad_chunk(pixels, c, c), -(-pixels // rt.linear_wgrad_chunk(pixels, c, c)), med[0], low[0],
                        nbytes / 1e6, med[1], low[1], med[0] / med[1], nbytes / med[0] / 1e3, med[2], low[2]))
    lines.append('three scales: wgrad %.1f  copy_ %.1f  ratio %.3f;  forward %.1f' % (sums[0], sums[1], sums[0] / sums[1], sums[2]))
    n = 3 * c * ((c + 3) // 4 * 4)
    w, m, v, gr = (torch.randn(n, dtype=torch.float32, device=dev, generator=gen) for _ in range(4))
    v.abs_()
    med, low = timed((lambda: rt.adam_step(w, m, v, gr, 1e-3),), a.rounds, a.iters)
    lines.append('adam_step over %d floats: %.1f (%.1f)' % (n, med[0], low[0]))
    # the whole step
    net = yolov3_body(L.Input(shape=[416, 416, 3]), 'mobilenetv2x75', 3, num_classes=a.classes)
    net.set_weights(synthetic_weights(net, 1234, 'conditioned'))
    tr = OutputLayerTrainer(net, anchors, a.classes, 3)
    images = torch.rand((a.batch, 416, 416, 3), dtype=torch.float32, device=dev, generator=gen)
    rs = np.random.RandomState(0)
    boxes = np.zeros((a.batch, 4, 5), np.float32)
    for b in range(a.batch):
        for k in range(4):
            bw, bh = rs.uniform(16, 300, 2)
            x0, y0 = rs.uniform(0, 416 - bw), rs.uniform(0, 416 - bh)
            boxes[b, k] = (x0, y0, x0 + bw, y0 + bh, rs.randint(a.classes))
    tb = torch.from_numpy(boxes).to(dev)
    med, low = timed((lambda: tr.features(images), lambda: tr.train_step_from_boxes(images, tb), lambda: net(images)), a.rounds, max(a.iters // 4, 1))
    lines.append('batch %d: feature forward %.1f (%.1f)  train_step_from_boxes %.1f (%.1f)  the model\'s own forward %.1f (%.1f);  step - features = %.1f'
                 % (a.batch, med[0], low[0], med[1], low[1], med[2], low[2], med[1] - med[0]))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
