"""The loss gradient stand-alone at the size it is built for: 64 images at 416 (grids 13 / 26 / 52, 20 classes), four labelled
boxes per image and scale, random logits (the recipe of tools/loss_probe.py).  Per scale, in ONE process and alternating round
by round, the hipEvent time of
    (i)   yr_yolo_loss                      the forward alone (memset + three launches),
    (ii)  zero_() of a tensor of dfeats' size  the cheapest way to write that many bytes,
    (iii) yr_yolo_loss_grad                 forward and gradient (memset + three launches),
the ratio (iii) / ((i) + (ii)) and the bytes the gradient call moves at least (logits and labels read once by the forward part,
dfeats written once; the class channels of object rows are read a second time, which is negligible).

    python tools/lossgrad_probe.py [--batch 64] [--rounds 20] [--iters 20] [--boxes 4] [--out profiles/rNN_lossgrad_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import runtime as rt                      # noqa: E402
from yoloret_amd.yolo3.utils import get_anchors            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--boxes', type=int, default=4)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    anchors = get_anchors('model_data/yolo_anchors.txt')
    rs = np.random.RandomState(0)
    lines = ['lossgrad_probe: batch %d, 416x416, %d classes, %d boxes per image and scale; %d rounds x %d calls, alternating; median (min) in us'
             % (a.batch, a.classes, a.boxes, a.rounds, a.iters)]
    sums = np.zeros(3)
    for s, mask in enumerate(([6, 7, 8], [3, 4, 5], [0, 1, 2])):
        g = 416 // (32 >> s)
        logits = rs.randn(a.batch, g, g, 3, 5 + a.classes).astype(np.float32)
        y_true = np.zeros_like(logits)
        for b in range(a.batch):
            for _ in range(a.boxes):
                j, i, k = rs.randint(g), rs.randint(g), rs.randint(3)
                w, h = anchors[mask][k] * rs.uniform(0.6, 1.6, 2)
                y_true[b, j, i, k, :5] = ((i + rs.uniform()) / g, (j + rs.uniform()) / g, w / 416, h / 416, 1)
                y_true[b, j, i, k, 5 + rs.randint(a.classes)] = 1
        ws = torch.empty(rt.yolo_loss_workspace_bytes(a.batch, g, g, 3), dtype=torch.uint8, device=dev)
        f, y, an = torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev), anchors[mask]
        d = torch.empty_like(f)
        variants = (lambda: rt.yolo_loss(f, y, an, (416, 416), .5, workspace=ws),
                    lambda: d.zero_(),
                    lambda: rt.yolo_loss_grad(f, y, an, (416, 416), .5, workspace=ws, out=d))
        for v in variants:      # warm-up: code objects, allocator
            v()
        torch.cuda.synchronize()
        times = [[], [], []]
        for _ in range(a.rounds):
            for k, v in enumerate(variants):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    v()
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1) * 1e3 / a.iters)
        med = [float(np.median(t)) for t in times]
        low = [float(np.min(t)) for t in times]
        sums += med
        nbytes = 3 * f.numel() * 4
        lines.append('scale %d (%dx%d): forward %.1f (%.1f)  zero_ %.1f (%.1f)  forward+gradient %.1f (%.1f)  ratio grad / (forward + zero_) %.3f;  '
                     'dfeats %.1f MB, moved >= %.1f MB -> %.0f GB/s'
                     % (s, g, g, med[0], low[0], med[1], low[1], med[2], low[2], med[2] / (med[0] + med[1]), f.numel() * 4 / 1e6, nbytes / 1e6,
                        nbytes / med[2] / 1e3))
    lines.append('three scales: forward %.1f  zero_ %.1f  forward+gradient %.1f  ratio %.3f' % (sums[0], sums[1], sums[2], sums[2] / (sums[0] + sums[1])))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
