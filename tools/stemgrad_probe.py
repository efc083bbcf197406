"""The 3 x 3 entry-convolution operators (csrc/stemgrad.hip) and the whole training step at the size they are built for: 64 images of
416 x 416 x 3 -> 208 x 208 x 24 (MobileNetV2 x0.75) and -> 48 (x1.4 and the wider EfficientNets), stride 2, 'same'.  In ONE process,
alternating round by round, the hipEvent time of
    entry      conv3x3_forward / conv3x3_dgrad / conv3x3_wgrad into preallocated outputs,
    copy_      copy_() of a tensor as large as the bytes the entry must move (each operand and the result once; copy_ reads and writes
               its size, so its tensor holds half of them): the yardstick of the other training probes,
    torch      the only other way to the same result: torch.nn.functional.conv2d on the same memory (the NHWC maps as channels_last
               views, the asymmetric 'same' pad as F.pad inside the timed call) and its autograd for either gradient alone,
and then one DetectorTrainer.train_step_from_boxes of MobileNetV2 x0.75 next to the forward-only plan of the same model and an
OutputLayerTrainer.train_step_from_boxes on the same batch.  Reads nothing outside the package.

    python tools/stemgrad_probe.py [--batch 64] [--rounds 10] [--iters 5] [--out profiles/rNN_stemgrad_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import layers as L, runtime as rt                            # noqa: E402
from yoloret_amd.weights import synthetic_weights                           # noqa: E402
from yoloret_amd.yolo3.model import yolov3_body                             # noqa: E402
from yoloret_amd.yolo3.train import DetectorTrainer, OutputLayerTrainer     # noqa: E402
from yoloret_amd.yolo3.utils import get_anchors                             # noqa: E402


def timed(variants, rounds, iters):
    """-> (medians, minima, maxima) in us per call, the variants alternating round by round"""
    for v in variants:      # warm-up: code objects, allocator, the library's algorithm search
        v()
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
    return [float(np.median(t)) for t in times], [float(np.min(t)) for t in times], [float(np.max(t)) for t in times]


def yardstick(nbytes, dev):
    """copy_ between two tensors of nbytes / 2: it moves nbytes"""
    n = max(nbytes // 8, 1)
    src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    return lambda: dst.copy_(src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    b, h, w, cin = a.batch, 416, 416, 3
    lines = ['stemgrad_probe: %d x %d x %d x %d, stride 2, \'same\'; %d rounds x %d calls, alternating; median (min .. max) in us'
             % (b, h, w, cin, a.rounds, a.iters)]
    x = torch.randn((b, h, w, cin), dtype=torch.float32, device=dev, generator=gen)
    for cout in (24, 48):
        pt, pl, oh, ow = rt.depthwise_geometry(h, w, 3, 2, 'same')
        wt = torch.randn((9 * cin, cout), dtype=torch.float32, device=dev, generator=gen) / 27 ** .5
        dy = torch.randn((b, oh, ow, cout), dtype=torch.float32, device=dev, generator=gen)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(wt)
        ws = torch.empty(rt.conv3x3_wgrad_workspace_bytes(b, oh, ow, cin, cout), dtype=torch.uint8, device=dev)
        moved = (x.numel() + dy.numel()) * 4
        # torch on the same memory: NCHW views of the NHWC maps (channels_last), the Keras kernel as [cout, cin, 3, 3]
        xt = x.permute(0, 3, 1, 2)
        dyt = dy.permute(0, 3, 1, 2)
        wtt = wt.reshape(3, 3, cin, cout).permute(3, 2, 0, 1).contiguous()
        pads = (pl, (ow - 1) * 2 + 3 - w - pl, pt, (oh - 1) * 2 + 3 - h - pt)

        def conv(xin, win):
            return F.conv2d(F.pad(xin, pads), win, stride=2)
        xg, wg = xt.detach().requires_grad_(True), wtt.detach().requires_grad_(True)
        yx, yw = conv(xg, wtt), conv(xt, wg)
        chunk = rt.conv3x3_wgrad_chunk(b, oh, ow, cin, cout)
        lines.append('%d -> %d channels: %.1f MB in, %.1f MB out; wgrad chunk %d rows, %d slabs'
                     % (cin, cout, x.numel() * 4 / 1e6, dy.numel() * 4 / 1e6, chunk, -(-b * oh // chunk)))
        for name, entry, other in (
                ('forward', lambda: rt.conv3x3_forward(x, wt, 2, 'same', out=y), lambda: conv(xt, wtt)),
                ('dgrad', lambda: rt.conv3x3_dgrad(dy, wt, (h, w), 2, 'same', out=dx), lambda: torch.autograd.grad(yx, xg, dyt, retain_graph=True)),
                ('wgrad', lambda: rt.conv3x3_wgrad(x, dy, 2, 'same', out=dw, workspace=ws), lambda: torch.autograd.grad(yw, wg, dyt, retain_graph=True))):
            with torch.no_grad() if name == 'forward' else torch.enable_grad():
                med, low, high = timed((entry, yardstick(moved, dev), other), a.rounds, a.iters)
            lines.append('  %-7s entry %.1f (%.1f .. %.1f)  copy_ of %.1f MB %.1f (%.1f .. %.1f)  ratio entry / copy_ %.3f, %.0f GB/s;  torch conv2d %.1f (%.1f .. %.1f), %.2f x the entry'
                         % (name, med[0], low[0], high[0], moved / 1e6, med[1], low[1], high[1], med[0] / med[1], moved / med[0] / 1e3, med[2], low[2], high[2],
                            med[2] / med[0]))
        del y, dx, dw, dy, ws, yx, yw, xg, wg
    del x
    torch.cuda.empty_cache()
    if not a.skip_step:
        anchors = get_anchors('model_data/yolo_anchors.txt')
        net = yolov3_body(L.Input(shape=[416, 416, 3]), 'mobilenetv2x75', 3, num_classes=a.classes)
        net.set_weights(synthetic_weights(net, 1234, 'conditioned'))
        images = torch.rand((b, 416, 416, 3), dtype=torch.float32, device=dev, generator=gen)
        rs = np.random.RandomState(0)
        boxes = np.zeros((b, 4, 5), np.float32)
        for i in range(b):
            for k in range(4):
                bw, bh = rs.uniform(16, 300, 2)
                x0, y0 = rs.uniform(0, 416 - bw), rs.uniform(0, 416 - bh)
                boxes[i, k] = (x0, y0, x0 + bw, y0 + bh, rs.randint(a.classes))
        tb = torch.from_numpy(boxes).to(dev)
        full, head = DetectorTrainer(net, anchors, a.classes, 3), OutputLayerTrainer(net, anchors, a.classes, 3)
        torch.cuda.reset_peak_memory_stats(dev)
        med, low, high = timed((lambda: full.train_step_from_boxes(images, tb), lambda: net(images), lambda: head.train_step_from_boxes(images, tb)),
                               max(a.rounds // 2, 3), max(a.iters // 2, 1))
        lines.append('MobileNetV2 x0.75, batch %d at 416 x 416: DetectorTrainer.train_step_from_boxes %.0f (%.0f .. %.0f)  the forward-only plan %.0f (%.0f .. %.0f)  '
                     'OutputLayerTrainer.train_step_from_boxes %.0f (%.0f .. %.0f);  full step / plan %.2f, full step / output-layer step %.2f;  peak device memory %.1f GB'
                     % (b, med[0], low[0], high[0], med[1], low[1], high[1], med[2], low[2], high[2], med[0] / med[1], med[0] / med[2],
                        torch.cuda.max_memory_allocated(dev) / 1e9))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
