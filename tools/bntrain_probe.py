"""BatchNorm in training mode stand-alone at the size it is built for: 64 images at 416, the neck's maps 13x13x512, 26x26x256 and
52x52x128.  In ONE process, alternating round by round, the hipEvent time of each entry next to copy_() of a tensor as large as the
bytes the CONTRACT must move at least (copy_ reads and writes its size, so its tensor holds half of them):
    bn_train_forward    z read once, a written: 2 maps (the kernels read z three times: sums, squared deviations, apply)
    bn_train_backward   da and z read, dz written: 3 maps (the kernels read da and z twice: sums, apply); with need_dz=False 2 maps
Reads nothing outside the package.

    python tools/bntrain_probe.py [--batch 64] [--rounds 20] [--iters 10] [--out profiles/rNN_bntrain_probe.txt]
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
    lines = ['bntrain_probe: batch %d, 416x416; %d rounds x %d calls, alternating; median (min) in us; ratio = entry / copy_ of the bytes the contract must move'
             % (a.batch, a.rounds, a.iters)]

    def row(name, fn, nbytes):
        med, low = timed((fn, yardstick(nbytes, dev)), a.rounds, a.iters)
        lines.append('%-52s %9.1f (%9.1f)   copy_ of %7.1f MB moved %9.1f (%9.1f)   ratio %.2f   %.0f GB/s' % (
            name, med[0], low[0], nbytes / 1e6, med[1], low[1], med[0] / med[1], nbytes / med[0] / 1e3))

    for g, ch in ((13, 512), (26, 256), (52, 128)):
        pixels = a.batch * g * g
        z, da = 3 + 2 * randn(a.batch, g, g, ch), randn(a.batch, g, g, ch)
        gamma, beta = 1 + .1 * randn(ch), .1 * randn(ch)
        mm, mv = torch.zeros(ch, device=dev), torch.ones(ch, device=dev)
        out, dz = torch.empty_like(z), torch.empty_like(z)
        ws = torch.empty(rt.bn_train_workspace_bytes(pixels, ch), dtype=torch.uint8, device=dev)
        chunk = rt.bn_train_chunk(pixels, ch)
        what = '%dx%dx%d (chunk %d pixels, %d slabs)' % (g, g, ch, chunk, -(-pixels // chunk))
        nb = z.numel() * 4
        _, mean, invstd = rt.bn_train_forward(z, gamma, beta, act='relu6', out=out, workspace=ws)
        row('bn_train_forward relu6 ' + what, lambda: rt.bn_train_forward(z, gamma, beta, 1e-3, .9, 'relu6', mm, mv, out=out, workspace=ws), 2 * nb)
        row('bn_train_backward relu6 ' + what, lambda: rt.bn_train_backward(da, z, gamma, beta, mean, invstd, 'relu6', out=dz, workspace=ws), 3 * nb)
        row('bn_train_backward relu6, no dz ' + what, lambda: rt.bn_train_backward(da, z, gamma, beta, mean, invstd, 'relu6', need_dz=False, workspace=ws),
            2 * nb)
        if g == 26:
            row('bn_train_forward swish ' + what, lambda: rt.bn_train_forward(z, gamma, beta, 1e-3, .9, 'swish', mm, mv, out=out, workspace=ws), 2 * nb)
            row('bn_train_backward swish ' + what, lambda: rt.bn_train_backward(da, z, gamma, beta, mean, invstd, 'swish', out=dz, workspace=ws), 3 * nb)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
