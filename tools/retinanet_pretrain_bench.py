"""RetinaNet classification pre-training (`is_pretraining: True`) throughput on one GPU: the ImageNet geometry 224 x 224, batch 64, random-init
weights, synthetic pictures and labels already in device memory; one step = forward, global-average-pool softmax cross-entropy head, backward,
Momentum.  Prints ONE JSON line: images/s per engine (host clock around `steps` steps that end in a device synchronise, after `warmup` steps)
and the two head kernels' time per launch (HIP events around 200 back-to-back launches on the step's own [64 * 49][224] rows).
usage: python tools/retinanet_pretrain_bench.py [steps=20] [warmup=5] [batch=64] [size=224]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import odtk  # noqa: E402
from odtk import ops  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
batch = int(sys.argv[3]) if len(sys.argv) > 3 else 64
size = int(sys.argv[4]) if len(sys.argv) > 4 else 224
assert torch.cuda.is_available(), 'needs an MI355X'
cfg = {'is_bottleneck': True, 'residual_block_list': [3, 4, 6, 3], 'init_conv_filters': 16, 'mode': 'train', 'is_pretraining': True,
       'data_shape': [size, size, 3], 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'data_format': 'channels_last', 'batch_size': batch,
       'gamma': 2.0, 'alpha': 0.25, 'nms_score_threshold': 0.8, 'nms_max_boxes': 10, 'nms_iou_threshold': 0.45, 'verbose': False}
g = torch.Generator().manual_seed(0)
imgs = (torch.rand(batch, size, size, 3, generator=g) * 255).round()
labels = torch.randint(0, 224, (batch,), generator=g).numpy()
out = {'metric': 'retinanet_pretrain_images_per_s', 'size': size, 'batch': batch, 'steps': steps, 'warmup': warmup,
       'device': torch.cuda.get_device_name(0)}
for engine in ('f32x3', 'bf16'):
    m = odtk.RetinaNet(dict(cfg, compute_dtype=engine), {'num_train': batch, 'num_val': 0, 'train_generator': [(imgs, labels)], 'val_generator': None})
    m.set_batch(imgs, labels)
    for _ in range(warmup):
        loss = m.train_step(1e-4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = m.train_step(1e-4)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out[engine] = {'images_per_s': round(batch / dt, 1), 'ms_per_step': round(dt * 1e3, 3), 'loss': float(loss.item())}
    assert np.isfinite(out[engine]['loss'])
    if engine == 'f32x3':                        # the head on the f32 rows of the last unit (the f32 engines' operand)
        f = m.feat
        HW = f.H * f.W
        fwd = lambda: ops.gap_softmax_ce_fwd(f.t, f.ld, f.N, HW, f.C, m.labels, 1.0 / batch, m.logits, m.ce, m.pred, m.correct, m.dlogits)  # noqa: E731
        bwd = lambda: ops.gap_softmax_ce_bwd(m.dlogits, f.N, HW, f.C, m.grad_of(f), f.ld, False)  # noqa: E731
        for name, fn in (('head_fwd_us', fwd), ('head_bwd_us', bwd)):
            for _ in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name] = round(e0.elapsed_time(e1) * 1e3 / 200, 2)
    del m
print(json.dumps(out))
