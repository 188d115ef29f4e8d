#!/usr/bin/env python
"""Classification-input benchmark (needs an MI355X and PIL).  Prints ONE JSON line:
  * imagenet_data.get_generator images/s at the 224 x 224 / batch 64 pre-training config (random crop, flip, colour jitter), next to voc_data.get_generator
    over the SAME pictures and augmentor config (plus pad_truth_to) in the same run: 128 pictures of 500 x 375, 4:2:0, quality 90 (tools/jpeg_bench.py's);
  * odtk_classify_eval at N = 64, C = 224 by HIP events, next to odtk_gap_softmax_ce_fwd at the same shape (HW = 49: the 7 x 7 map of a 224 x 224 input).
Every figure: warm-up first, then `--reps` repetitions, median with min and max."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from make_jpeg_fixtures import picture          # noqa: E402


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v)}


def loader_rate(it, batch, reps, batches=4):
    for _ in range(3):
        next(it)
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(batches):
            next(it)
        torch.cuda.synchronize(); t.append(batches * batch / (time.perf_counter() - t0))
    it.close()
    return spread(t)


def event_ms(fn, reps, inner=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--pictures', type=int, default=128)
    a = ap.parse_args()
    from PIL import Image
    import odtk  # noqa: F401
    from odtk import imagenet_data, ops, voc_data
    assert torch.cuda.is_available(), 'imagenet_bench needs an MI355X'
    dev = torch.device('cuda:0')
    datas = []
    for k in range(a.pictures):
        buf = io.BytesIO()
        Image.fromarray(picture(500, 375, 1000 + k), 'RGB').save(buf, 'JPEG', quality=90, subsampling=2)
        datas.append(buf.getvalue())
    B = 64
    res = {'pictures': len(datas), 'batch': B, 'output_shape': [224, 224], 'reps': a.reps}
    cfg = {'data_format': 'channels_last', 'output_shape': [224, 224], 'crop_method': 'random', 'flip_prob': [0., 0.5], 'fill_mode': 'BILINEAR',
           'keep_aspect_ratios': False, 'constant_values': 0., 'color_jitter_prob': 0.5}
    with tempfile.TemporaryDirectory() as d:
        inet, voc = os.path.join(d, 'imagenet.tfrecord'), os.path.join(d, 'voc.tfrecord')
        with voc_data.TFRecordWriter(inet) as w:
            for k, data in enumerate(datas):
                w.write(imagenet_data.encode_example(data, [375, 500, 3], k % 224))
        with voc_data.TFRecordWriter(voc) as w:
            for k, data in enumerate(datas):
                w.write(voc_data.encode_example(data, [375, 500, 3], [[50, 300, 60, 400, k % 20]]))
        res['imagenet_generator_images_per_s'] = loader_rate(iter(imagenet_data.get_generator([inet], B, len(datas), cfg, device=dev, seed=0)), B, a.reps)
        res['voc_generator_images_per_s'] = loader_rate(iter(voc_data.get_generator([voc], B, len(datas), dict(cfg, pad_truth_to=60), device=dev, seed=0)),
                                                        B, a.reps)
    N, C, HW = 64, 224, 49
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N * HW, C, generator=g).to(dev)
    labels = torch.randint(0, C, (N,), generator=g).to(torch.int32).to(dev)
    logits, loss, correct, dlogits = torch.zeros(N, C, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, C, device=dev)
    pred = torch.zeros(N, dtype=torch.int32, device=dev)
    ev = odtk.ClassificationEvaluator(C, 5, device=dev)
    ops.gap_softmax_ce_fwd(x, C, N, HW, C, labels, 1.0 / N, logits, loss, pred, correct, dlogits)
    res['gap_softmax_ce_fwd_ms'] = event_ms(lambda: ops.gap_softmax_ce_fwd(x, C, N, HW, C, labels, 1.0 / N, logits, loss, pred, correct, dlogits), a.reps)
    res['classify_eval_ms'] = event_ms(lambda: ev.update(logits, labels), a.reps)
    res['classify_eval_shape'] = {'N': N, 'C': C, 'HW_of_the_head': HW}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
