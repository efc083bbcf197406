"""The squeeze-excite block (csrc/segrad.hip) stand-alone at the sizes it is built for: 64 images at 416, the head blocks' maps and
EfficientNet's stage 2.  In ONE process, alternating round by round, the hipEvent time of each entry next to copy_() of a tensor as
large as the bytes the CONTRACT must move at least (copy_ reads and writes its size, so its tensor holds half of them), in maps:
    se_forward                    x read twice (the mean, then the product), y written: 3
    se_backward, dx and params    dy read twice (dg, then dx), x read, dx written: 4
    se_backward, dx only          the same four: 4
    se_backward, params only      dy and x read: 2
(the [B, C] and [B, R] vectors, the kernels and the slabs are small next to a map and are not counted).  Reads nothing outside the
package.

    python tools/segrad_probe.py [--batch 64] [--rounds 20] [--iters 10] [--out profiles/rNN_segrad_probe.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bntrain_probe import timed, yardstick      # noqa: E402
from yoloret_amd import runtime as rt           # noqa: E402

SHAPES = ((13, 512, 128), (26, 256, 64), (52, 128, 32), (104, 96, 4))      # (map side, C, R)


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
    lines = ['segrad_probe: batch %d; %d rounds x %d calls, alternating; median (min) in us; ratio = entry / copy_ of the bytes the contract must move'
             % (b, a.rounds, a.iters)]

    def row(name, fn, nbytes):
        med, low = timed((fn, yardstick(nbytes, dev)), a.rounds, a.iters)
        lines.append('%-44s %9.1f (%9.1f)   copy_ of %7.1f MB moved %9.1f (%9.1f)   ratio %.2f   %.0f GB/s' % (
            name, med[0], low[0], nbytes / 1e6, med[1], low[1], med[0] / med[1], nbytes / med[0] / 1e3))

    for g, c, r in SHAPES:
        x, dy = randn(b, g, g, c), randn(b, g, g, c)
        w1, b1, w2, b2 = randn(c, r) / c ** .5, randn(r), randn(r, c) / r ** .5, randn(c)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        ws = torch.empty(rt.se_workspace_bytes(b, g * g, c, r), dtype=torch.uint8, device=dev)
        _, m, z1, gate = rt.se_forward(x, w1, b1, w2, b2, out=y, workspace=ws)
        chunk = rt.se_chunk(b, g * g, c)
        nb = x.numel() * 4
        what = ' %dx%dx%d R%d' % (g, g, c, r)
        lines.append('%dx%dx%d R%d: chunk %d pixels, %d slabs an image' % (g, g, c, r, chunk, -(-g * g // chunk)))
        row('se_forward' + what, lambda: rt.se_forward(x, w1, b1, w2, b2, out=y, workspace=ws), 3 * nb)
        row('se_backward, dx and params' + what, lambda: rt.se_backward(dy, x, w1, w2, m, z1, gate, out=dx, workspace=ws), 4 * nb)
        row('se_backward, dx only' + what, lambda: rt.se_backward(dy, x, w1, w2, m, z1, gate, need_params=False, out=dx, workspace=ws), 4 * nb)
        row('se_backward, params only' + what, lambda: rt.se_backward(dy, x, w1, w2, m, z1, gate, need_dx=False, workspace=ws), 2 * nb)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
