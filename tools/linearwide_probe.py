"""The wide 1x1 entries (csrc/linearwide.hip) at the size they are built for: eleven 1x1 layers of MobileNetV2 x0.75's neck at 64 images
of 416 x 416 (grids 13 / 26 / 52, O = 75): the first convolution of the six head blocks, the four link convolutions and the 512 -> O
projection of td1 and bu1.  In ONE process, alternating round by round, the hipEvent time of
    wide       the wide entry (linear_wide_forward / _dgrad / _wgrad),
    copy_      copy_() of a tensor as large as the bytes the contract must move (both operands and the result, each once; copy_ reads
               and writes its size, so its tensor holds half of them): the yardstick of the other probes,
    blocks     the only way to the same result without the wide entries: the narrow entries (linear_forward / _dgrad / _wgrad, at most
               256 channels on either side) on column blocks of at most 256 channels with torch glue - contiguous() slices of the
               activations, add of the partial products, cat of the column blocks.  The weight's blocks are cut once, outside the timed
               window.  A layer that is narrow on both sides is one narrow call, into preallocated outputs like the wide call.
Reads nothing outside the package.

    python tools/linearwide_probe.py [--batch 64] [--rounds 20] [--iters 10] [--out profiles/rNN_linearwide_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import runtime as rt           # noqa: E402

O = 75
LAYERS = [      # (name, grid, cin, cout)
    ('td1_conv', 13, 120 + 96, 512), ('td1/bu1_mb_project', 13, 512, O), ('block_20_conv', 13, O, 256),
    ('td2_conv', 26, 256 + 72 + 96, 256), ('block_24_conv', 26, O, 128),
    ('td3_conv', 52, 128 + 24 + 96, 128), ('bu3_conv', 52, O, 128), ('bu3_down_conv', 52, O, 128),
    ('bu2_conv', 26, 128 + O, 256), ('bu2_down_conv', 26, O, 256), ('bu1_conv', 13, 256 + O, 512),
]


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


def cuts(n):
    """n channels -> [(first, last + 1)] of the fewest equal blocks of at most 256, each but the last a multiple of 4"""
    k = -(-n // 256)
    size = (-(-n // k) + 3) // 4 * 4
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def pack(w):
    """[cout, cin] -> wt [cout, round_up(cin, 4)], pad columns 0"""
    out = torch.zeros((w.shape[0], (w.shape[1] + 3) // 4 * 4), dtype=torch.float32, device=w.device)
    out[:, :w.shape[1]] = w
    return out


def blockwise(x, dy, w):
    """-> (forward, dgrad, wgrad) closures of the narrow entries on blocks of at most 256 channels"""
    cin, cout = w.shape[1], w.shape[0]
    ci, co = cuts(cin), cuts(cout)
    wts = {(i, j): pack(w[c0:c1, a0:a1]) for j, (c0, c1) in enumerate(co) for i, (a0, a1) in enumerate(ci)}
    ws = torch.empty(max(rt.linear_wgrad_workspace_bytes(x.numel() // cin, a1 - a0, c1 - c0) for a0, a1 in ci for c0, c1 in co), dtype=torch.uint8,
                     device=x.device)

    one = len(ci) == 1 and len(co) == 1      # one narrow call: it writes into buffers of its own, as the wide call does
    if one:
        oy, odx, odw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(wts[(0, 0)])

    def cols(t, cut):
        return [t] if len(cut) == 1 else [t[..., a:b].contiguous() for a, b in cut]

    def forward():
        if one:
            return rt.linear_forward(x, wts[(0, 0)], out=oy)
        xs, ys = cols(x, ci), []
        for j in range(len(co)):
            y = rt.linear_forward(xs[0], wts[(0, j)])
            for i in range(1, len(ci)):
                y = y.add_(rt.linear_forward(xs[i], wts[(i, j)]))
            ys.append(y)
        return ys[0] if len(ys) == 1 else torch.cat(ys, -1)

    def dgrad():
        if one:
            return rt.linear_dgrad(dy, wts[(0, 0)], cin, out=odx)
        ds, dxs = cols(dy, co), []
        for i, (a0, a1) in enumerate(ci):
            dx = rt.linear_dgrad(ds[0], wts[(i, 0)], a1 - a0)
            for j in range(1, len(co)):
                dx = dx.add_(rt.linear_dgrad(ds[j], wts[(i, j)], a1 - a0))
            dxs.append(dx)
        return dxs[0] if len(dxs) == 1 else torch.cat(dxs, -1)

    def wgrad():
        if one:
            return rt.linear_wgrad(x, dy, out=odw, workspace=ws)
        xs, ds = cols(x, ci), cols(dy, co)
        rows = []
        for j in range(len(co)):
            parts = [rt.linear_wgrad(xs[i], ds[j], workspace=ws) for i in range(len(ci))]
            # the blocks' pad columns lie inside the row: only the last block's stay
            parts = [p[:, :a1 - a0] for p, (a0, a1) in zip(parts[:-1], ci[:-1])] + [parts[-1]]
            rows.append(parts[0] if len(parts) == 1 else torch.cat(parts, -1))
        return rows[0] if len(rows) == 1 else torch.cat(rows, 0)
    return forward, dgrad, wgrad


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
    lines = ['linearwide_probe: batch %d, 416x416; %d rounds x %d calls, alternating; median (min) in us; wide = the wide entry, copy_ = copy_ of the bytes the '
             'contract moves, blocks = the narrow entries on <= 256-wide column blocks with torch glue' % (a.batch, a.rounds, a.iters)]
    worst = {}
    for name, g, cin, cout in LAYERS:
        x, dy = randn(a.batch, g, g, cin), randn(a.batch, g, g, cout)
        w = randn(cout, cin) / cin ** .5
        wt = pack(w)
        pixels = a.batch * g * g
        y, dx, dwt = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(wt)
        ws = torch.empty(rt.linear_wide_wgrad_workspace_bytes(pixels, cin, cout), dtype=torch.uint8, device=dev)
        bf, bd, bw = blockwise(x, dy, w)
        # the two ways agree (another order of the sums: last bits)
        for got, want in ((rt.linear_wide_forward(x, wt), bf()), (rt.linear_wide_dgrad(dy, wt, cin), bd()), (rt.linear_wide_wgrad(x, dy), bw())):
            err = float((got - want).abs().max() / want.abs().max())
            assert got.shape == want.shape and err < 1e-5, (name, err)
        nb = 4 * (x.numel() + dy.numel() + wt.numel())
        chunk = rt.linear_wide_wgrad_chunk(pixels, cin, cout)
        lines.append('%s %dx%d, %d -> %d (%d pixels; %d x %d column blocks; gradient chunk %d, %d slabs)' % (
            name, g, g, cin, cout, pixels, len(cuts(cin)), len(cuts(cout)), chunk, -(-pixels // chunk)))
        for what, wide, blocks in (('forward', lambda: rt.linear_wide_forward(x, wt, out=y), bf), ('dgrad', lambda: rt.linear_wide_dgrad(dy, wt, cin, out=dx), bd),
                                   ('wgrad', lambda: rt.linear_wide_wgrad(x, dy, out=dwt, workspace=ws), bw)):
            med, low = timed((wide, yardstick(nb, dev), blocks), a.rounds, a.iters)
            lines.append('    %-8s wide %8.1f (%8.1f)   copy_ of %6.1f MB %8.1f (%8.1f)   blocks %8.1f (%8.1f)   wide / copy_ %5.2f   wide / blocks %5.2f' % (
                what, med[0], low[0], nb / 1e6, med[1], low[1], med[2], low[2], med[0] / med[1], med[0] / med[2]))
            worst[what] = max(worst.get(what, 0.0), med[0] / med[2])
    lines.append('largest wide / blocks: ' + ', '.join('%s %.2f' % kv for kv in worst.items()))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
