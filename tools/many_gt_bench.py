"""Times the box-side entry points that take up to 1 024 ground-truth rows per image, at the BASELINE shapes of tools/heads_bench.py and
tools/retina_bench.py (SSD300: 8 828 priors, batch 32), with `boxes` random boxes in `pad` rows per image.  HIP events, median of `runs` runs of 20 calls.
usage: python tools/many_gt_bench.py [pad [boxes [runs]]]      (defaults 1024 1023 5; `60 6` is the shape of the default path)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import odtk  # noqa: F401
from odtk import ops
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _synth as S

pad = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
boxes = int(sys.argv[2]) if len(sys.argv) > 2 else pad - 1
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device('cuda')


def gt_of(N, size, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.full((N, pad, 5), -1.0)
    h = torch.rand(N, boxes, generator=g) * 0.45 * size + 0.05 * size
    w = torch.rand(N, boxes, generator=g) * 0.45 * size + 0.05 * size
    gt[:, :boxes] = torch.stack([h / 2 + torch.rand(N, boxes, generator=g) * (size - h), w / 2 + torch.rand(N, boxes, generator=g) * (size - w), h, w,
                                 torch.randint(0, 20, (N, boxes), generator=g).float()], -1)
    return gt.to(dev)


def timeit(f, reps=20):
    ts = []
    for _ in range(3):
        f()
    for _ in range(runs):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            f()
        e.record(); torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / reps * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def report(name, t):
    print(f'P={pad} boxes={boxes} {name:16s} median {t[0]:9.1f} us  (min {t[1]:.1f}, max {t[2]:.1f} of {runs} runs)', flush=True)


g = torch.Generator().manual_seed(0)
i32 = dict(dtype=torch.int32, device=dev)
# SSD300, config 2: 8 828 priors, 32 images
from odtk.ssd300 import prior_spec
fs, nas, hwp = prior_spec()
pri = ops.ssd_priors(300, fs, nas, hwp, dev)
N, A = 32, pri[0].shape[0]
gt = gt_of(N, 300, 1)
out = (torch.zeros(N, **i32), torch.zeros(N, pad, **i32), torch.zeros(N, A, dtype=torch.uint8, device=dev), torch.zeros(N, A, **i32), torch.zeros(N, 4, **i32))
report('ssd_match', timeit(lambda: ops.ssd_match(pri[0], pri[1], pri[3], gt, *out)))
# RetinaNet, config 3: 800 x 800, 16 images, 120 087 anchors
N = 16
anc = ops.retina_anchors(800, S.pyramid_shapes(800, 800), [9] * 5, S.retina_priors_flat(), dev)
A = anc[0].shape[0]
gt = gt_of(N, 800, 2)
ngt, best, status, rg, counts = (torch.zeros(N, **i32), torch.zeros(N, pad, **i32), torch.zeros(N, A, dtype=torch.uint8, device=dev), torch.zeros(N, A, **i32),
                                 torch.zeros(N, 4, **i32))
ws = ops.retina_match_workspace(A, N, pad, dev)
pconf = torch.randn(N, A, 21, device=dev); pbox = torch.randn(N, A, 4, device=dev) * 0.5
parts = torch.empty(N, 2, device=dev); dconf = torch.empty_like(pconf); dbox = torch.empty_like(pbox)
report('retina_match', timeit(lambda: ops.retina_match(anc[0], anc[1], anc[3], gt, ngt, best, status, rg, counts, ws)))
report('retina_loss', timeit(lambda: ops.retina_loss(pconf, pbox, anc[2], anc[3], gt, ngt, best, status, rg, counts, 0.25, 2.0, 1.0 / N, parts, dconf, dbox)))
del pconf, pbox, dconf, dbox, ws
# CenterNet, config 5: 512 x 512, 16 images -> 128 x 128 x 20
N, H, W, C = 16, 128, 128, 20
kp = (torch.randn(N, H, W, C, generator=g) - 2).to(dev); off = torch.rand(N, H, W, 2, generator=g).to(dev); size = (torch.rand(N, H, W, 2, generator=g) * 40).to(dev)
gt = gt_of(N, 512, 3)
parts = torch.zeros(N, 4, device=dev); dk, do, dz = torch.empty_like(kp), torch.empty_like(off), torch.empty_like(size)
ws = ops.centernet_workspace(N, H, W, C, dev)
report('centernet_loss', timeit(lambda: ops.centernet_loss(kp, off, size, gt, 4.0, 1.0 / N, parts, dk, do, dz, ws)))
# FCOS, config 5: 512 x 512, 16 images, 21 classes
shapes = S.pyramid_shapes(512, 512)
conf = [(torch.randn(N, h, w, 21, generator=g) - 2).to(dev) for h, w in shapes]
reg = [torch.exp(torch.randn(N, h, w, 4, generator=g)).to(dev) for h, w in shapes]
cen = [torch.randn(N, h, w, 1, generator=g).to(dev) for h, w in shapes]
gt = gt_of(N, 512, 4)
loss = torch.zeros(N, device=dev)
dc, dr, dz = [torch.empty_like(t_) for t_ in conf], [torch.empty_like(t_) for t_ in reg], [torch.empty_like(t_) for t_ in cen]
ws = ops.fcos_workspace(conf, N, dev)
report('fcos_loss', timeit(lambda: ops.fcos_loss(conf, reg, cen, gt, 1.0 / N, loss, dc, dr, dz, ws)))
# YOLOv3, config 4: 416 x 416, 8 images
N = 8
preds = [torch.randn(N, h, h, 3, 25, generator=g).to(dev) for h in (13, 26, 52)]
gt = gt_of(N, 416, 5)
parts = torch.zeros(N, 5, device=dev); dp = [torch.empty_like(p) for p in preds]
ws = ops.yolov3_workspace(preds, N, dev)
report('yolov3_loss', timeit(lambda: ops.yolov3_loss(preds, S.yolo_priors_flat(), [32., 16., 8.], gt, (1., 1., 5., 1.), 1.0 / N, parts, dp, ws)))
