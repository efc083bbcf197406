"""The loss forward stand-alone at the size it is built for: 64 images at 416 (grids 13 / 26 / 52, 20 classes), four
labelled boxes per image and scale, random logits.  Prints the hipEvent time of one scale's call (memset + three launches)
and of the three scales together; run it under `rocprofv3 --kernel-trace --stats` for the per-launch figures of DESIGN.md.

    python tools/loss_probe.py [--batch 64] [--iters 50] [--boxes 4]
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
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--boxes', type=int, default=4)
    ap.add_argument('--classes', type=int, default=20)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    anchors = get_anchors('model_data/yolo_anchors.txt')
    rs = np.random.RandomState(0)
    cases = []
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
        cases.append((torch.from_numpy(logits).to(dev), torch.from_numpy(y_true).to(dev), anchors[mask], ws))

    def run(which):
        return [rt.yolo_loss(f, y, an, (416, 416), .5, workspace=ws) for f, y, an, ws in (cases[i] for i in which)]

    for which, name in (((0,), 'scale 0 (13x13)'), ((1,), 'scale 1 (26x26)'), ((2,), 'scale 2 (52x52)'), ((0, 1, 2), 'three scales')):
        out = run(which)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            out = run(which)
        t1.record()
        torch.cuda.synchronize()
        print('%-16s %8.1f us per call   terms %s' % (name, t0.elapsed_time(t1) * 1e3 / a.iters, ' | '.join(str(o.tolist()) for o in out)))


if __name__ == '__main__':
    main()
