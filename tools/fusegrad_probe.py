"""The fusing operators (csrc/fusegrad.hip) stand-alone at the sizes they are built for: 64 images at 416.  In ONE process, alternating
round by round, the hipEvent time of each entry next to copy_() of a tensor as large as the bytes the CONTRACT must move at least
(copy_ reads and writes its size, so its tensor holds half of them), in maps of the LARGE side (L) and the small side (S = L / k^2):
    maxpool_forward     x read, y written: L + S          maxpool_backward    dy and x read, dx written: 2 L + S
    upsample2_forward   x read, y written: S + L          upsample2_backward  dy read, dx written: L + S
    wsum_forward        four maps read, y written: 5      wsum_backward       dy read, four dx written: 5; with d alpha the four maps
                                                                              are read too: 9; d alpha alone: 5
Reads nothing outside the package.

    python tools/fusegrad_probe.py [--batch 64] [--rounds 20] [--iters 10] [--out profiles/rNN_fusegrad_probe.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bntrain_probe import timed, yardstick      # noqa: E402
from yoloret_amd import runtime as rt           # noqa: E402


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
    b = a.batch

    def randn(*shape):
        return torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    lines = ['fusegrad_probe: batch %d, 416x416; %d rounds x %d calls, alternating; median (min) in us; ratio = entry / copy_ of the bytes the contract must move'
             % (b, a.rounds, a.iters)]

    def row(name, fn, nbytes):
        med, low = timed((fn, yardstick(nbytes, dev)), a.rounds, a.iters)
        lines.append('%-44s %9.1f (%9.1f)   copy_ of %7.1f MB moved %9.1f (%9.1f)   ratio %.2f   %.0f GB/s' % (
            name, med[0], low[0], nbytes / 1e6, med[1], low[1], med[0] / med[1], nbytes / med[0] / 1e3))

    for k, g, ch in ((2, 52, 48), (2, 52, 128), (4, 104, 24)):
        x = torch.clamp(3 + 4 * randn(b, g, g, ch), 0, 6)          # behind a ReLU6: ties over large areas
        y, dy, dx = torch.empty(b, g // k, g // k, ch, device=dev), randn(b, g // k, g // k, ch), torch.empty_like(x)
        big, small = x.numel() * 4, y.numel() * 4
        what = ' k=%d %dx%dx%d' % (k, g, g, ch)
        row('maxpool_forward' + what, lambda: rt.maxpool_forward(x, k, out=y), big + small)
        row('maxpool_backward' + what, lambda: rt.maxpool_backward(dy, x, k, out=dx), 2 * big + small)
    for g, ch in ((13, 256), (26, 96)):
        x, dy = randn(b, g, g, ch), randn(b, 2 * g, 2 * g, ch)
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        what = ' %dx%dx%d' % (g, g, ch)
        row('upsample2_forward' + what, lambda: rt.upsample2_forward(x, out=y), 5 * x.numel() * 4)
        row('upsample2_backward' + what, lambda: rt.upsample2_backward(dy, out=dx), 5 * x.numel() * 4)
    g, ch = 26, 48
    xs, dy, alpha = [randn(b, g, g, ch) for _ in range(4)], randn(b, g, g, ch), torch.tensor([1.25, -0.7, 0.5, 0.33], device=dev)
    y, dxs = torch.empty_like(dy), [torch.empty_like(dy) for _ in range(4)]
    pixels = b * g * g
    chunk = rt.wsum_chunk(pixels, ch)
    ws = torch.empty(rt.wsum_workspace_bytes(pixels, ch), dtype=torch.uint8, device=dev)
    nb = dy.numel() * 4
    what = ' %dx%dx%d' % (g, g, ch)
    lines.append('wsum_backward: chunk %d pixels, %d slabs' % (chunk, -(-pixels // chunk)))
    row('wsum_forward' + what, lambda: rt.wsum_forward(xs, alpha, out=y), 5 * nb)
    row('wsum_backward, maps and alpha' + what, lambda: rt.wsum_backward(dy, xs, alpha, out=dxs, workspace=ws), 9 * nb)
    row('wsum_backward, maps only' + what, lambda: rt.wsum_backward(dy, None, alpha, need_alpha=False, out=dxs), 5 * nb)
    row('wsum_backward, alpha only' + what, lambda: rt.wsum_backward(dy, xs, alpha, need=(False,) * 4, workspace=ws), 5 * nb)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
