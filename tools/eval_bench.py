"""Times the VOC evaluator (odtk.VOCEvaluator.result / csrc/voc_eval.hip) and end-to-end SSD300.evaluate; prints one JSON line.

  * VOC07-test sized input: 4 952 images, 20 classes, ~100 detections and ~2.4 GT rows per image (seeded);
  * stress: 100 000 images x 20 detections = 2 M detections of one class;
  * per input: result() with device synchronisation (host packing, the one upload, the kernels, the read-back), the kernels alone (odtk_voc_eval
    on uploaded tensors, HIP events) and the NumPy restatement (tests/voc_eval_ref.evaluate_fast) on 16 threads;
  * SSD300.evaluate on the exact f32 engine (test mode, score threshold 0.01) in images/s, and the evaluator's share of it.
  * --coco: only the COCO-style leg on the VOC07-test sized input (odtk.COCOEvaluator, default 10 thresholds x 4 area ranges, max_dets 100): result()
    wall time, the kernels alone (odtk_coco_eval, HIP events), ten VOCEvaluator.result() calls at the ten thresholds on the same data (what the
    ten-threshold number cost before odtk_coco_eval existed) and the NumPy restatement (tests/coco_eval_ref.evaluate_fast).
  * --flags: only the ground-truth-flag leg on the VOC07-test sized input with VOC07-test's share of `difficult` rows (2 944 of 14 976):
    odtk_voc_eval_flags / odtk_coco_eval_flags next to odtk_voc_eval / odtk_coco_eval on the same uploaded tensors in the same process, the calls
    interleaved, every repetition timed by its own pair of HIP events (median, min, max).  The flagged calls end with the read-back of the flag check
    (a 4-byte copy and a stream synchronisation inside the entry point), which the events include.
Per-kernel times: run `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/eval_bench.py --kernels-only` separately."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np      # noqa: E402
import torch            # noqa: E402

import odtk             # noqa: E402
from odtk import ops    # noqa: E402
import voc_eval_ref as R                # noqa: E402
import coco_eval_ref as CR              # noqa: E402


def synthetic(seed, n_img, C, det_per_img, gt_mean, one_class=None):
    rng = np.random.default_rng(seed)
    ng = np.clip(rng.poisson(gt_mean - 1, n_img) + 1, 1, 12) if gt_mean != int(gt_mean) else np.full(n_img, int(gt_mean))
    dets, gts = [], []
    for k in range(n_img):
        n = int(ng[k])
        yc, xc, h, w = rng.uniform(20, 280, n), rng.uniform(20, 280, n), rng.uniform(8, 120, n), rng.uniform(8, 120, n)
        cls = rng.integers(0, C, n) if one_class is None else np.full(n, one_class)
        g = np.stack([yc, xc, h, w, cls], 1).astype(np.float32)
        j = rng.integers(0, n, det_per_img)
        hit = rng.random(det_per_img) < 0.3
        c = np.stack([yc - h / 2, xc - w / 2, yc + h / 2, xc + w / 2], 1)[j]
        rnd = rng.uniform(0, 260, (det_per_img, 2))
        box = np.where(hit[:, None], c + rng.normal(0, 4, (det_per_img, 4)), np.concatenate([rnd, rnd + rng.uniform(5, 80, (det_per_img, 2))], 1))
        dc = np.where(hit, cls[j], rng.integers(0, C, det_per_img)) if one_class is None else np.full(det_per_img, one_class)
        dets.append((rng.random(det_per_img).astype(np.float32), box.astype(np.float32), dc.astype(np.int32)))
        gts.append(g)
    return dets, gts


def time_result(dets, gts, C, dev, reps):
    ev = odtk.VOCEvaluator(C, device=dev)
    for d, g in zip(dets, gts):
        ev.add(list(d), g)
    ev.result()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ev.result()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return ev, 1e3 * float(np.median(ts))


def time_kernels(ev, C, dev, reps):
    scores, boxes, cls, img, gt, gi = ev._pack()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    args = [t(scores), t(boxes), t(cls), t(img), t(gt), t(gi)]
    D, G, I = scores.shape[0], gt.shape[0], ev.num_images
    ws = ops.voc_eval_workspace(D, G, I, C, dev)
    tp = torch.empty(D, dtype=torch.uint8, device=dev)
    npos = torch.empty(C, dtype=torch.int32, device=dev)
    ap = torch.empty(C, dtype=torch.float64, device=dev)
    run = lambda: ops.voc_eval(*args, I, C, 0.5, 'voc07', ws, tp, npos, ap)   # noqa: E731
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def coco_leg(dev, reps):
    C = 20
    dets, gts = synthetic(0, 4952, C, 100, 2.4, None)
    ev = odtk.COCOEvaluator(C, device=dev)
    voc = [odtk.VOCEvaluator(C, float(t), 'area', device=dev) for t in ev.iou_thresholds]
    for d, g in zip(dets, gts):
        ev.add(list(d), g)
        for v in voc:
            v.add(list(d), g)

    def wall(f):
        f()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return 1e3 * float(np.median(ts))
    r = ev.result()
    row = {'images': len(gts), 'detections': int(r['num_detections'].sum()), 'gt_rows': sum(len(g) for g in gts), 'pairs': int(r['ap'].shape[0] * r['ap'].shape[1]),
           'AP': r['AP'], 'AP50': r['AP50'], 'AP75': r['AP75'], 'result_ms': wall(ev.result), 'ten_voc_results_ms': wall(lambda: [v.result() for v in voc])}
    args, _ = ev._upload()
    D, G, I = args[0].shape[0], args[4].shape[0], ev.num_images
    T, Rn = ev.iou_thresholds.shape[0], ev.area_ranges.shape[0]
    ws = ops.coco_eval_workspace(D, G, I, C, T, Rn, dev)
    match = torch.empty(Rn, T, D, dtype=torch.uint8, device=dev)
    npos = torch.empty(Rn, C, dtype=torch.int32, device=dev)
    ap, rec = (torch.empty(Rn, T, C, dtype=torch.float64, device=dev) for _ in range(2))
    run = lambda: ops.coco_eval(*args, I, C, ev.iou_thresholds, ev.area_ranges, ev.max_dets, ws, match, npos, ap, rec)   # noqa: E731
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    row['kernels_ms'] = e0.elapsed_time(e1) / reps
    row['voc_kernels_ms'] = time_kernels(voc[0], C, dev, reps)
    t = time.perf_counter()
    ref = CR.evaluate_fast(dets, gts, C)
    row['numpy_ref_ms'] = 1e3 * (time.perf_counter() - t)
    row['match_equal_ref'] = bool(np.array_equal(ref['match'], r['match']))
    row['ap_max_abs_diff_ref'] = float(np.nanmax(np.abs(ref['ap'] - r['ap'])))
    return row


def flags_leg(dev, reps):
    C = 20
    dets, gts = synthetic(0, 4952, C, 100, 2.4, None)
    G = sum(len(g) for g in gts)
    rng = np.random.default_rng(5)
    difficult = np.zeros(G, np.uint8)
    difficult[rng.permutation(G)[: round(G * 2944 / 14976)]] = 1
    ev = odtk.COCOEvaluator(C, device=dev)
    at = 0
    for d, g in zip(dets, gts):
        ev.add(list(d), g, flags=difficult[at: at + len(g)])
        at += len(g)
    args, _, gfl, nign_host = ev._upload(True)
    D, I = args[0].shape[0], ev.num_images
    T, Rn = ev.iou_thresholds.shape[0], ev.area_ranges.shape[0]
    ws_v, ws_c = ops.voc_eval_workspace(D, G, I, C, dev), ops.coco_eval_workspace(D, G, I, C, T, Rn, dev)
    tp = torch.empty(D, dtype=torch.uint8, device=dev)
    npos, nign = (torch.empty(C, dtype=torch.int32, device=dev) for _ in range(2))
    ap = torch.empty(C, dtype=torch.float64, device=dev)
    match = torch.empty(Rn, T, D, dtype=torch.uint8, device=dev)
    npos_c = torch.empty(Rn, C, dtype=torch.int32, device=dev)
    ap_c, rec_c = (torch.empty(Rn, T, C, dtype=torch.float64, device=dev) for _ in range(2))
    runs = {
        'voc_eval': lambda: ops.voc_eval(*args, I, C, 0.5, 'voc07', ws_v, tp, npos, ap),
        'voc_eval_flags': lambda: ops.voc_eval_flags(*args, gfl, I, C, 0.5, 'voc07', ws_v, tp, npos, nign, ap),
        'coco_eval': lambda: ops.coco_eval(*args, I, C, ev.iou_thresholds, ev.area_ranges, ev.max_dets, ws_c, match, npos_c, ap_c, rec_c),
        'coco_eval_flags': lambda: ops.coco_eval_flags(*args, gfl, I, C, ev.iou_thresholds, ev.area_ranges, ev.max_dets, ws_c, match, npos_c, ap_c,
                                                       rec_c),
    }
    times = {k: [] for k in runs}
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    for _ in range(reps):                                              # interleaved: a drift of the clock hits all four alike
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    row = {'images': I, 'detections': D, 'gt_rows': G, 'flagged_rows': int(difficult.sum()), 'reps': reps, 'ignored_per_class_sum': int(nign_host.sum())}
    for k, v in times.items():
        row[k + '_ms'] = {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}
    return row


def time_numpy(dets, gts, C):
    t = time.perf_counter()
    R.evaluate_fast(dets, gts, C)
    return 1e3 * (time.perf_counter() - t)


def ssd300_e2e(dev, n_images):
    from oracle import ssd300_ref as SR
    cfg = {'mode': 'test', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 1,
           'nms_score_threshold': 0.01, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': '', 'verbose': False,
           'compute_dtype': 'f32'}
    p = SR.init_params(3)
    imgs, _ = SR.synthetic_batch(2, 7)
    SR.calibrate_bn(p, imgs, subtract_mean=False)
    val = [tuple(t.numpy() for t in SR.synthetic_batch(4, 300 + i)) for i in range(n_images // 4)]
    m = odtk.SSD300(cfg, None)
    m.load_oracle_params(p)
    m.evaluate(generator=val[:1])                                     # warm-up
    spent = []
    orig = odtk.VOCEvaluator.result

    def timed(self):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = orig(self)
        torch.cuda.synchronize()
        spent.append(time.perf_counter() - t)
        return r
    odtk.VOCEvaluator.result = timed
    try:
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = m.evaluate(generator=val)
        torch.cuda.synchronize()
        total = time.perf_counter() - t
    finally:
        odtk.VOCEvaluator.result = orig
    return {'images': n_images, 'images_per_s': n_images / total, 'evaluate_ms': 1e3 * total, 'result_ms': 1e3 * spent[0],
            'evaluator_share': spent[0] / total, 'detections': int(r['num_detections'].sum()), 'mAP': r['mAP']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--e2e-images', type=int, default=256)
    ap.add_argument('--kernels-only', action='store_true', help='a few kernel runs of both inputs (for rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--coco', action='store_true', help='only the COCO-style leg (odtk.COCOEvaluator against ten VOC passes and the NumPy restatement)')
    ap.add_argument('--flags', action='store_true', help='only the flag leg: the _flags entry points next to the unflagged ones, VOC07-test sized')
    a = ap.parse_args()
    torch.set_num_threads(16)
    os.environ.setdefault('OMP_NUM_THREADS', '16')
    dev = torch.device('cuda:0')
    if a.flags:
        print(json.dumps({'flags_voc07': flags_leg(dev, a.reps)}))
        return
    if a.coco:
        print(json.dumps({'coco_voc07': coco_leg(dev, a.reps)}))
        return
    out = {}
    for name, spec in [('voc07', (0, 4952, 20, 100, 2.4, None)), ('stress_2m', (1, 100000, 20, 20, 2, 0))]:
        t0 = time.perf_counter()
        dets, gts = synthetic(*spec)
        ev, ms_result = time_result(dets, gts, spec[2], dev, 1 if a.kernels_only else a.reps)
        ms_kern = time_kernels(ev, spec[2], dev, 3 if a.kernels_only else a.reps)
        row = {'images': spec[1], 'detections': sum(len(d[0]) for d in dets), 'gt_rows': sum(len(g) for g in gts),
               'result_ms': ms_result, 'kernels_ms': ms_kern}
        if not a.kernels_only:
            row['numpy_ref_ms'] = time_numpy(dets, gts, spec[2])
            row['speedup_kernels_vs_numpy'] = row['numpy_ref_ms'] / ms_kern
            row['speedup_result_vs_numpy'] = row['numpy_ref_ms'] / ms_result
        row['setup_s'] = time.perf_counter() - t0
        out[name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    if not a.kernels_only:
        out['ssd300_evaluate_f32'] = ssd300_e2e(dev, a.e2e_images)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
