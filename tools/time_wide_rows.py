"""HIP-event timing of the box-side entry points behind DESIGN.md section 3, "Box side beyond 31 classes" (raw lines: profiles/wide_rows_c81_vs_c21.json).
Needs an MI355X:   python tools/time_wide_rows.py C TAG      (C: logits per row, background included; TAG: a label copied into the line)
odtk_ssd_loss at N = 32, A = 8 828; odtk_retina_loss at N = 2, A = 120 087; the two batched decodes at N = 8.  Random logits, four boxes and 24 positive
rows per image, 84 mined negatives; 10 warm-up launches, then 50 timed one by one between two events.  Prints one JSON line (median, minimum, 90th
percentile in microseconds).  Run it from a checkout of another commit to time that commit's library."""
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import odtk
from odtk import ops
C, tag = int(sys.argv[1]), sys.argv[2]
dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(1)
i32, u8 = torch.int32, torch.uint8

def timed(fn, iters=50, warm=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return {'median_us': round(ts[len(ts) // 2], 2), 'min_us': round(ts[0], 2), 'p90_us': round(ts[int(len(ts) * .9)], 2)}

def match(N, A, P, kind):
    G = 4
    gt = torch.full((N, P, 5), -1.0); gt[:, :G, :2] = 100. + 100. * torch.rand(N, G, 2, generator=g); gt[:, :G, 2:4] = 50.; gt[:, :G, 4] = torch.randint(0, C - 1, (N, G), generator=g).float()
    status = torch.full((N, A), 2, dtype=u8)
    pos = torch.randint(0, A, (N, 24), generator=g)
    status.scatter_(1, pos, 1)
    best = torch.full((N, P), -1, dtype=i32); best[:, :G] = torch.randint(0, A, (N, G), generator=g).to(i32)
    status.scatter_(1, best[:, :G].long(), 0 if kind == 'ssd' else 3)
    rg = torch.randint(0, G, (N, A), generator=g).to(i32)
    counts = torch.zeros(N, 4, dtype=i32); counts[:, 0] = G + (status == 1).sum(1).to(i32); counts[:, 1] = (status == 2).sum(1).to(i32)
    counts[:, 2] = torch.minimum(3 * counts[:, 0], counts[:, 1])
    ngt = torch.full((N,), G, dtype=i32)
    return [t.to(dev) for t in (gt, ngt, best, status, rg, counts)]

out = {'tag': tag, 'C': C, 'version': int(odtk._lib.load().odtk_version())}
# odtk_ssd_loss N = 32, A = 8828
N, A, P, ld = 32, 8828, 60, C + 4
pred = torch.randn(N, A, ld, generator=g).to(dev)
yx = (20. + 260. * torch.rand(A, 2, generator=g)).to(dev); hw = (16. + 100. * torch.rand(A, 2, generator=g)).to(dev)
gt, ngt, best, status, rg, counts = match(N, A, P, 'ssd')
negloss = torch.zeros(N, A, device=dev)
ops.softmax_ce_const(pred, N * A, C, ld, C - 1, negloss)
nsel = int(counts[0, 2])
sel = torch.stack([torch.nonzero(status[n] == 2).flatten()[: 3 * 28].to(i32) for n in range(N)])
sel_idx = torch.full((N, A), -1, dtype=i32, device=dev); sel_idx[:, : sel.shape[1]] = sel
sel_cnt = torch.full((N,), sel.shape[1], dtype=i32, device=dev)
parts = torch.zeros(N, 4, device=dev); dpred = torch.zeros(N, A, ld, device=dev)
out['ssd_loss_N32_A8828'] = timed(lambda: ops.ssd_loss(pred, C, yx, hw, gt, ngt, best, status, rg, counts, negloss, sel_idx, sel_cnt, 1.0 / N, parts, dpred))
# batched decodes, N = 8
N8 = 8
conf = torch.zeros(N8, A, C - 1, device=dev); boxes = torch.zeros(N8, A, 4, device=dev); keep = torch.zeros(N8, A, dtype=u8, device=dev); cand = torch.zeros(N8, A, C - 1, dtype=u8, device=dev)
p8 = pred[:N8].contiguous()
out['ssd_decode_batched_N8_A8828'] = timed(lambda: ops.ssd_decode_batched(p8, C, yx, hw, 0.5, conf, boxes, keep, cand))
del pred, dpred, p8, conf, cand
# RetinaNet at 800 x 800: A = 120087
N, A = 2, 120087
pconf = torch.randn(N, A, C, generator=g).to(dev); pbox = (0.5 * torch.randn(N, A, 4, generator=g)).to(dev)
yx = (20. + 760. * torch.rand(A, 2, generator=g)).to(dev); hw = (16. + 300. * torch.rand(A, 2, generator=g)).to(dev)
gt, ngt, best, status, rg, counts = match(N, A, P, 'retina')
parts = torch.zeros(N, 2, device=dev); dconf = torch.zeros(N, A, C, device=dev); dbox = torch.zeros(N, A, 4, device=dev)
out['retina_loss_N2_A120087'] = timed(lambda: ops.retina_loss(pconf, pbox, yx, hw, gt, ngt, best, status, rg, counts, 0.25, 2.0, 1.0 / N, parts, dconf, dbox))
del dconf
pc8 = torch.randn(N8, A, C, generator=g).to(dev); pb8 = (0.5 * torch.randn(N8, A, 4, generator=g)).to(dev)
conf = torch.zeros(N8, A, C - 1, device=dev); boxes = torch.zeros(N8, A, 4, device=dev); keep = torch.zeros(N8, A, dtype=u8, device=dev); cand = torch.zeros(N8, A, C - 1, dtype=u8, device=dev)
out['retina_decode_batched_N8_A120087'] = timed(lambda: ops.retina_decode_batched(pc8, pb8, yx, hw, 0.5, conf, boxes, keep, cand))
print(json.dumps(out))
