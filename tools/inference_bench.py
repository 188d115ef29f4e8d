"""Inference and evaluation rates, per-image path against batched path, in ONE process on ONE set of weights; prints one JSON line.

Per class and engine (--classes ssd300,ssd512,yolov3,retinanet,centernet,refinedet,pfpnet; engines of the class or --engines):
  * the loop of test_one_image on a model built without test_batch_size.  Since the seven classes share one inference path (heads.BatchedInference) this row
    and the B = 1 row below time the SAME code; the row stays so that runs of this tool on older commits, where it was the separate per-image tail, compare;
  * test_images at B = 1, 8, 32 (16 for RetinaNet 800 x 800) on models built with test_batch_size = B from the same weights;
  * evaluate() at batch_size 1 and at the largest B over the same validation generator, with the share of the wall time spent in Python staging
    (VOCEvaluator.add) and in result();
  * the kernel times of the batched tail at the largest B by HIP events: the decode launch, and compaction + NMS + pack (BatchedTail.launch), plus the
    read-back (wall clock); CenterNet's tail is the decode alone (score / arg-max + one top-k workgroup per image, heads.CenterNetBatched).
Only pairs measured in the same process count: two boxes of a pool differ by more than most changes.  Synthetic weights and pixels; the score threshold is
lowered for the SSD family (--score-threshold, default 0.01) so that the tail has detections to carry; the other classes keep their configuration's
threshold (at 0.01 a random-weight RetinaNet has more candidate rows than the NMS takes).
--nms-methods hard,linear,gaussian: only the tail, once per method, on ONE decode output: a model at the largest B runs one batch, then a BatchedTail per
method is timed by HIP events on that model's conf / boxes / cand (NMS + pack; 'hard' is the launch chain of odtk_nms_image_class + odtk_detection_pack, the
soft methods odtk_soft_nms_image_class + odtk_detection_pack_scored), with the detections each returns."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402

import odtk             # noqa: E402
from odtk import ops    # noqa: E402
import bench_configs as BCFG    # noqa: E402

CLASSES = {'ssd300': 'SSD300', 'ssd512': 'SSD512', 'yolov3': 'YOLOv3', 'retinanet': 'RetinaNet', 'centernet': 'CenterNet', 'refinedet': 'RefineDet320',
           'pfpnet': 'PFPNetR'}
ENGINES = {'ssd300': ['f32', 'f32x3', 'bf16'], 'ssd512': ['f32'], 'yolov3': ['f32'], 'retinanet': ['f32'], 'centernet': ['f32'], 'refinedet': ['f32'],
           'pfpnet': ['f32']}              # (the last three: the engine test mode defaults to)
BATCHES = {'ssd300': [1, 8, 32], 'ssd512': [1, 8, 32], 'yolov3': [1, 8, 32], 'retinanet': [1, 8, 16], 'centernet': [1, 8, 32], 'refinedet': [1, 8, 32],
           'pfpnet': [1, 8, 32]}
THRESHOLD_KEY = {'centernet': 'score_threshold'}                  # (CenterNet has no NMS: its threshold has a key of its own)


def build(name, engine, B, thr, weights=None):
    cfg, size, _, _ = BCFG.config_of(name, dtype=engine, mode='test', **({} if thr is None else {THRESHOLD_KEY.get(name, 'nms_score_threshold'): thr}))
    if B is not None:
        cfg['test_batch_size'] = B
    m = getattr(odtk, CLASSES[name])(cfg, None)
    if weights is not None:
        m.load_oracle_params(weights)
    return m, size


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed_evaluate(m, gen, n_images, B):
    spent = {'add': 0.0, 'result': 0.0}
    add0, res0 = odtk.VOCEvaluator.add, odtk.VOCEvaluator.result

    def add(self, *a):
        t = time.perf_counter()
        r = add0(self, *a)
        spent['add'] += time.perf_counter() - t
        return r

    def result(self):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = res0(self)
        torch.cuda.synchronize()
        spent['result'] += time.perf_counter() - t
        return r
    m.evaluate(generator=gen[:1], batch_size=B)                       # warm-up
    odtk.VOCEvaluator.add, odtk.VOCEvaluator.result = add, result
    try:
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = m.evaluate(generator=gen, num_images=n_images, batch_size=B)
        torch.cuda.synchronize()
        total = time.perf_counter() - t
    finally:
        odtk.VOCEvaluator.add, odtk.VOCEvaluator.result = add0, res0
    return {'batch_size': B, 'images_per_s': n_images / total, 'ms': 1e3 * total, 'python_staging_share': spent['add'] / total,
            'result_share': spent['result'] / total, 'detections': int(r['num_detections'].sum())}


def tail_times(m, name, reps):
    t = m._tail_batched
    if name == 'centernet':
        from odtk.centernet import STRIDE as CN_STRIDE
        out = {'N': t.N, 'pixels_per_image': t.H * t.W, 'top_k': t.K}
        out['decode_ms'] = events_ms(lambda: t.launch(m.keypoints, m.offset, m.size, m.score_threshold, CN_STRIDE), reps)     # score / arg-max + peak test + top-k
        out['read_back_ms'] = 1e3 * wall(lambda: t.read(), reps)
        out['read_back_bytes'] = int(t.words.numel() * 4)
        return out
    iou = m.nms_iou_threshold
    cand = t.cand.view(torch.uint8)
    out = {'N': t.N, 'rows_per_image': t.A, 'compaction': bool(t.compact)}
    if name in ('refinedet', 'pfpnet'):
        out['decode_ms'] = events_ms(lambda: ops.refinedet_decode_batched(m.arm_loc, m.arm_conf, m.odm_loc, m.odm_conf, m.anc[2], m.anc[3], m.nms_score_threshold,
                                                                           t.conf, t.boxes, t.keep, t.cand), reps)
    elif name in ('ssd300', 'ssd512'):
        out['decode_ms'] = events_ms(lambda: ops.ssd_decode_batched(m.pred, m.num_classes, m.pri[2], m.pri[3], m.nms_score_threshold, t.conf, t.boxes, t.keep,
                                                                      t.cand), reps)
    elif name == 'retinanet':
        out['decode_ms'] = events_ms(lambda: ops.retina_decode_batched(m.pconf, m.pbox, m.anc[2], m.anc[3], m.nms_score_threshold, t.conf, t.boxes, t.keep,
                                                                        t.cand), reps)
    elif name == 'yolov3':
        from odtk.yolov3 import STRIDE

        def decode_loop():
            for b in range(t.N):
                ops.yolov3_decode_candidates([p[b] for p in m.preds], m.priors_flat, (STRIDE[2], STRIDE[2], STRIDE[1]), out=(t.conf[b], t.boxes[b]))
            torch.ge(t.conf, m.nms_score_threshold, out=t.cand)
        out['decode_ms'] = events_ms(decode_loop, reps)                      # N launches of the single-image decode + one threshold launch
        out['decode_host_ms'] = 1e3 * wall(decode_loop, reps)                # the same by the wall clock, device idle before and after: the host's enqueue time shows
    out['nms_pack_ms' if not t.compact else 'compact_nms_pack_ms'] = events_ms(lambda: t.launch(t.conf, t.boxes, cand, iou), reps)
    out['read_back_ms'] = 1e3 * wall(lambda: t.read(), reps)
    out['read_back_bytes'] = int(t.words.numel() * 4)
    return out


def tail_by_method(name, engine, a):
    """the NMS + pack time of the batched tail per nms_method at the largest B, on the decode output of one batch of synthetic pictures"""
    from odtk import heads
    B = [b for b in BATCHES[name] if b <= a.max_batch][-1]
    thr = a.score_threshold if a.score_threshold is not None else (0.01 if name in ('ssd300', 'ssd512') else None)
    m, size = build(name, engine, B, thr)
    g = torch.Generator().manual_seed(11)
    m.test_images((torch.rand(B, size, size, 3, generator=g) * 255).round().numpy())
    t = m._tail_batched
    cand = t.cand.view(torch.uint8)
    row = {'class': name, 'engine': engine, 'input': size, 'N': t.N, 'rows_per_image': t.A, 'classes': t.nc, 'max_boxes': t.max_boxes,
           'score_threshold': m.nms_score_threshold, 'candidates_per_problem_mean': float(cand.sum()) / (t.N * t.nc),
           'candidates_per_problem_max': int(cand.sum(dim=1).max()), 'nms_pack_ms': {}, 'detections': {}}
    for method in a.nms_methods.split(','):
        t2 = heads.BatchedTail(t.N, t.A, t.nc, t.max_boxes, t.dev, method=method, sigma=m.soft_nms_sigma, min_score=m.soft_nms_min_score)
        row['nms_pack_ms'][method] = events_ms(lambda: t2.launch(t.conf, t.boxes, cand, m.nms_iou_threshold), max(a.reps, 20))
        row['detections'][method] = sum(len(d[0]) for d in t2.read())
    return row


def run(name, engine, a):
    Bs = [b for b in BATCHES[name] if b <= a.max_batch]
    thr = a.score_threshold if a.score_threshold is not None else (0.01 if name in ('ssd300', 'ssd512') else None)
    one, size = build(name, engine, None, thr)
    weights = one.export_params()
    n_img = a.images
    g = torch.Generator().manual_seed(11)
    images = (torch.rand(n_img, size, size, 3, generator=g) * 255).round().numpy()
    gt = BCFG.synthetic_gt(n_img, size, 12).numpy()
    gen = [(images[s: s + 8], gt[s: s + 8]) for s in range(0, n_img, 8)]
    row = {'class': name, 'engine': engine, 'input': size, 'images': n_img, 'score_threshold': getattr(one, THRESHOLD_KEY.get(name, 'nms_score_threshold'))}

    def loop():
        for k in range(n_img):
            one.test_one_image(images[k: k + 1])
    sec = wall(loop, a.reps)
    row['test_one_image_loop'] = {'images_per_s': n_img / sec, 'ms_per_image': 1e3 * sec / n_img}
    row['test_images'] = {}
    big = None
    for B in Bs:
        m, _ = build(name, engine, B, thr, weights)

        def batched(m=m, B=B):
            for s in range(0, n_img, B):
                m.test_images(images[s: s + B])
        sec = wall(batched, a.reps)
        row['test_images'][str(B)] = {'images_per_s': n_img / sec, 'ms_per_image': 1e3 * sec / n_img,
                                      'speedup_vs_loop': row['test_one_image_loop']['ms_per_image'] / (1e3 * sec / n_img)}
        if B == Bs[-1]:
            big = m
        else:
            del m
            torch.cuda.empty_cache()
    row['evaluate'] = [timed_evaluate(one, gen, n_img, 1), timed_evaluate(big, gen, n_img, Bs[-1])]
    row['evaluate_speedup'] = row['evaluate'][0]['ms'] / row['evaluate'][1]['ms']
    row['tail'] = tail_times(big, name, max(a.reps, 5))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', default='ssd300')
    ap.add_argument('--engines', default=None, help='comma list; default: the engines of each class')
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max-batch', type=int, default=32)
    ap.add_argument('--score-threshold', type=float, default=None, help='default: 0.01 for the SSD family, the class configuration otherwise')
    ap.add_argument('--nms-methods', default=None, help="comma list of 'hard', 'linear', 'gaussian': time only the tail (NMS + pack), once per method")
    a = ap.parse_args()
    torch.set_num_threads(16)
    rows = []
    for name in a.classes.split(','):
        for engine in (a.engines.split(',') if a.engines else ENGINES[name]):
            rows.append(tail_by_method(name, engine, a) if a.nms_methods else run(name, engine, a))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({'tool': 'inference_bench', 'device': torch.cuda.get_device_name(0), 'rows': rows}))


if __name__ == '__main__':
    main()
