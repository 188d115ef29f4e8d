"""HIP-event timing of RefineDet's box-side entry points behind DESIGN.md section 3, "RefineDet320 / PFPNetR beyond 95 classes" (raw line:
profiles/refinedet_rows.json).  Needs an MI355X:   python tools/time_refinedet_rows.py TAG      (TAG: a label copied into the line)
odtk_refinedet_loss, odtk_refinedet_decode_batched and odtk_refinedet_decode at RefineDet320's shape: A = 6 375 anchors (heads.refinedet_anchors(320)),
N = 32 images (bench_configs.SHAPES['refinedet']), at C = 21 and C = 96 logits (the one-thread kernels) and C = 97 and C = 121 (the 16-lane kernels).
Random logits, four boxes and 24 positive rows per image, 84 mined negatives.  ONE process: all operands are made first, then 10 warm-up rounds and 50
timed rounds, each round running every (entry point, C) once between two events, so that the four class counts share whatever the box does meanwhile.
Prints one JSON line (median, minimum, 90th percentile in microseconds)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import odtk
import bench_configs
from odtk import heads, ops

tag = sys.argv[1] if len(sys.argv) > 1 else ''
dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(1)
i32, u8 = torch.int32, torch.uint8
anc = heads.refinedet_anchors(320, dev)
A, N, P, G = anc[0].shape[0], bench_configs.SHAPES['refinedet'][1], 60, 4
CLASSES = [21, 96, 97, 121]


def operands(C):
    gt = torch.full((N, P, 5), -1.0)
    gt[:, :G, :2] = 100. + 100. * torch.rand(N, G, 2, generator=g)
    gt[:, :G, 2:4] = 50.
    gt[:, :G, 4] = torch.randint(0, C - 1, (N, G), generator=g).float()
    status = torch.full((N, A), 2, dtype=u8)
    status.scatter_(1, torch.randint(0, A, (N, 24), generator=g), 1)
    best = torch.full((N, P), -1, dtype=i32)
    best[:, :G] = torch.randint(0, A, (N, G), generator=g).to(i32)
    status.scatter_(1, best[:, :G].long(), 3)
    rg = torch.randint(0, G, (N, A), generator=g).to(i32)
    counts = torch.zeros(N, 4, dtype=i32)
    counts[:, 0] = G + (status == 1).sum(1).to(i32)
    counts[:, 1] = (status == 2).sum(1).to(i32)
    counts[:, 2] = torch.minimum(3 * counts[:, 0], counts[:, 1])
    sel = torch.stack([torch.nonzero(status[n] == 2).flatten()[: 3 * 28].to(i32) for n in range(N)])
    sel_idx = torch.full((N, A), -1, dtype=i32)
    sel_idx[:, : sel.shape[1]] = sel
    x = dict(arm_loc=0.5 * torch.randn(N, A, 4, generator=g), arm_conf=torch.randn(N, A, 2, generator=g), odm_loc=0.5 * torch.randn(N, A, 4, generator=g),
             odm_conf=torch.randn(N, A, C, generator=g), gt=gt, ngt=torch.full((N,), G, dtype=i32), best=best, status=status, rg=rg, counts=counts,
             sel_idx=sel_idx, sel_cnt=torch.full((N,), sel.shape[1], dtype=i32))
    x = {k: v.to(dev) for k, v in x.items()}
    x['negloss'] = torch.zeros(N, A, device=dev)
    ops.softmax_ce_const(x['arm_conf'], N * A, 2, 2, 1, x['negloss'])
    x.update(parts=torch.zeros(N, 8, device=dev), d_arm_loc=torch.zeros(N, A, 4, device=dev), d_arm_conf=torch.zeros(N, A, 2, device=dev),
             d_odm_loc=torch.zeros(N, A, 4, device=dev), d_odm_conf=torch.zeros(N, A, C, device=dev), conf=torch.zeros(N, A, C - 1, device=dev),
             boxes=torch.zeros(N, A, 4, device=dev), keep=torch.zeros(N, A, dtype=u8, device=dev), cand=torch.zeros(N, A, C - 1, dtype=u8, device=dev))
    return x


def calls(x):
    return {'refinedet_loss': lambda: ops.refinedet_loss(x['arm_loc'], x['arm_conf'], x['odm_loc'], x['odm_conf'], anc[2], anc[3], x['gt'], x['ngt'], x['best'],
                                                         x['status'], x['rg'], x['counts'], x['negloss'], x['sel_idx'], x['sel_cnt'], 1.0 / N, x['parts'],
                                                         x['d_arm_loc'], x['d_arm_conf'], x['d_odm_loc'], x['d_odm_conf']),
            'refinedet_decode_batched': lambda: ops.refinedet_decode_batched(x['arm_loc'], x['arm_conf'], x['odm_loc'], x['odm_conf'], anc[2], anc[3], 0.5,
                                                                             x['conf'], x['boxes'], x['keep'], x['cand']),
            'refinedet_decode': lambda: ops.refinedet_decode(x['arm_loc'][0], x['arm_conf'][0], x['odm_loc'][0], x['odm_conf'][0], anc[2], anc[3], 0.5)}


fns = {(name, C): fn for C in CLASSES for name, fn in calls(operands(C)).items()}
times = {k: [] for k in fns}
for it in range(60):
    for k, fn in fns.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        if it >= 10:
            times[k].append(a.elapsed_time(b) * 1e3)
out = {'tag': tag, 'version': int(odtk._lib.load().odtk_version()), 'device': torch.cuda.get_device_name(0), 'N': N, 'A': A}
for (name, C), ts in times.items():
    ts.sort()
    out[f'{name}_C{C}'] = {'median_us': round(ts[len(ts) // 2], 2), 'min_us': round(ts[0], 2), 'p90_us': round(ts[int(len(ts) * .9)], 2)}
print(json.dumps(out))
