"""The backward operators stand-alone at the size they are built for: 64 images at 416 (grids 13 / 26 / 52).  In ONE process,
alternating round by round, the hipEvent time of each entry next to copy_() of a tensor as large as the bytes that entry must read
AND write (copy_ reads and writes its size, so its tensor holds half of them): the yardstick of the loss and headtrain probes.
    linear_dgrad       75 <- 75 channels at the three scales' pixel counts: reads dy, writes dx
    depthwise forward / dgrad / wgrad, 3x3, stride 1, 'same' at 13x13x512, 26x26x256, 52x52x128 (wgrad reads two maps, writes 9 C floats)
    bn_act_backward    Swish at 26x26x256: reads da and u, writes dz
Reads nothing outside the package.

    python tools/convgrad_probe.py [--batch 64] [--rounds 20] [--iters 10] [--out profiles/rNN_convgrad_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import runtime as rt           # noqa: E402


def timed(variants, rounds, iters):
    """-> (medians, minima) in us per call, the variants alternating round by round"""
    for v in variants:
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


def yardstick(nbytes, dev):
    """copy_ between two tensors of nbytes / 2: it moves nbytes"""
    n = max(nbytes // 8, 1)
    src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    return lambda: dst.copy_(src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    def randn(*shape):
        return torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    lines = ['convgrad_probe: batch %d, 416x416; %d rounds x %d calls, alternating; median (min) in us; ratio = entry / copy_ of the bytes it reads and writes'
             % (a.batch, a.rounds, a.iters)]

    def row(name, fn, nbytes):
        med, low = timed((fn, yardstick(nbytes, dev)), a.rounds, a.iters)
        lines.append('%-44s %9.1f (%9.1f)   copy_ of %7.1f MB moved %9.1f (%9.1f)   ratio %.2f   %.0f GB/s' % (
            name, med[0], low[0], nbytes / 1e6, med[1], low[1], med[0] / med[1], nbytes / med[0] / 1e3))

    c = 75
    wt = torch.zeros((c, 76), dtype=torch.float32, device=dev)
    wt[:, :c] = randn(c, c) / c ** .5
    for g in (13, 26, 52):
        dy = randn(a.batch, g, g, c)
        dx = torch.empty_like(dy)
        row('linear_dgrad 75<-75 %dx%d (%d pixels)' % (g, g, a.batch * g * g), lambda: rt.linear_dgrad(dy, wt, c, out=dx), 2 * dy.numel() * 4)
    for g, ch in ((13, 512), (26, 256), (52, 128)):
        x, dy, w = randn(a.batch, g, g, ch), randn(a.batch, g, g, ch), randn(9, ch)
        y, dw = torch.empty_like(x), torch.empty_like(w)
        ws = torch.empty(rt.depthwise_wgrad_workspace_bytes(a.batch, g, g, ch, 3), dtype=torch.uint8, device=dev)
        nb = x.numel() * 4
        row('depthwise_forward 3x3 %dx%dx%d' % (g, g, ch), lambda: rt.depthwise_forward(x, w, out=y), 2 * nb)
        row('depthwise_dgrad   3x3 %dx%dx%d' % (g, g, ch), lambda: rt.depthwise_dgrad(dy, w, (g, g), out=y), 2 * nb)
        row('depthwise_wgrad   3x3 %dx%dx%d (chunk %d rows, %d slabs)' % (g, g, ch, rt.depthwise_wgrad_chunk(a.batch, g, g, ch, 3), ws.numel() // (36 * ch)),
            lambda: rt.depthwise_wgrad(x, dy, 3, out=dw, workspace=ws), 2 * nb)
    da, u, sc = randn(a.batch, 26, 26, 256), randn(a.batch, 26, 26, 256), randn(256)
    dz = torch.empty_like(da)
    row('bn_act_backward swish 26x26x256', lambda: rt.bn_act_backward(da, u, sc, 'swish', out=dz), 3 * da.numel() * 4)
    row('bn_act_backward relu6 26x26x256', lambda: rt.bn_act_backward(da, u, sc, 'relu6', out=dz), 3 * da.numel() * 4)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
