"""NumPy restatement of the PASCAL VOC metric that csrc/voc_eval.hip computes (include/odtk.h, odtk_voc_eval): the yardstick of
tests/test_cpu_voc_eval.py and tests/test_gpu_voc_eval.py.

Ground truth rows [yc, xc, h, w, cls] px (cls < 0 = padding), corners in f32 as y1 = yc - h/2, y2 = yc + h/2.  Within a class detections are ranked by
score, descending, ties to the earlier sequence number (argsort(kind='stable') of -score over sequence order).  Each detection, in that order, takes the
first GT row of its (image, class) with the largest IoU (f32, no +1 term; min / max ignore a NaN operand as C's fminf / fmaxf do, and a union that
is not > 0 -- NaN included -- gives IoU 0, so a detection box with non-finite coordinates is simply a miss) when IoU > iou_threshold and the row is not taken yet (TP), else it is an FP.
AP in f64 from the cumulative sums along the class's rank: 'voc07' = 11-point (t = np.arange(0., 1.1, 0.1)), 'area' = area under the precision
envelope (VOC2010+).  A class without GT has AP NaN and is left out of the mAP."""
import numpy as np


def iou_f32(box, gts):
    """box f32[4] (y1, x1, y2, x2) against gts f32[n, 4] -> f32[n]"""
    box = np.asarray(box, np.float32)
    gts = np.asarray(gts, np.float32).reshape(-1, 4)
    ih = np.fmax(np.fmin(box[2], gts[:, 2]) - np.fmax(box[0], gts[:, 0]), np.float32(0))
    iw = np.fmax(np.fmin(box[3], gts[:, 3]) - np.fmax(box[1], gts[:, 1]), np.float32(0))
    inter = ih * iw
    union = (box[2] - box[0]) * (box[3] - box[1]) + (gts[:, 2] - gts[:, 0]) * (gts[:, 3] - gts[:, 1]) - inter
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(union > 0, inter / np.where(union > 0, union, np.float32(1)), np.float32(0)).astype(np.float32)


def gt_corners(rows):
    rows = np.asarray(rows, np.float32).reshape(-1, 5)
    yc, xc, h, w = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    two = np.float32(2)
    return np.stack([yc - h / two, xc - w / two, yc + h / two, xc + w / two], 1).astype(np.float32)


def average_precision(tp_sorted, npos, metric='voc07'):
    """tp flags along the class's global rank -> AP (f64); NaN when npos == 0"""
    if npos == 0:
        return float('nan')
    tp_sorted = np.asarray(tp_sorted, np.float64)
    tp = np.cumsum(tp_sorted)
    fp = np.cumsum(1.0 - tp_sorted)
    rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    if metric == 'voc07':
        ap = 0.0
        for t in np.arange(0., 1.1, 0.1):
            p = 0.0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.
        return float(ap)
    if metric != 'area':
        raise ValueError(metric)
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]                     # mpre[i] = max(mpre[i], mpre[i + 1]) from the back
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def _flatten(dets, gts):
    scores = np.concatenate([np.asarray(d[0], np.float32).reshape(-1) for d in dets]) if dets else np.zeros(0, np.float32)
    boxes = np.concatenate([np.asarray(d[1], np.float32).reshape(-1, 4) for d in dets]) if dets else np.zeros((0, 4), np.float32)
    cls = np.concatenate([np.asarray(d[2]).reshape(-1).astype(np.int64) for d in dets]) if dets else np.zeros(0, np.int64)
    img = np.concatenate([np.full(len(np.asarray(d[0]).reshape(-1)), k, np.int64) for k, d in enumerate(dets)]) if dets else np.zeros(0, np.int64)
    return scores, boxes, cls, img


def evaluate_fast(dets, gts, num_classes, iou_threshold=0.5, metric='voc07'):
    """evaluate() with the greedy match vectorised, for millions of detections.  A detection takes GT row j iff its best IoU > threshold and no
    detection ranked before it in the same (image, class) has j as its best row with IoU > threshold (such an earlier one either took j or found it
    taken): TP = first occurrence of (image, class, j) among the above-threshold detections in rank order.  tests/test_cpu_voc_eval.py checks it
    against evaluate() on random cases."""
    scores, boxes, cls, img = _flatten(dets, gts)
    C, D = int(num_classes), scores.shape[0]
    rows = [np.asarray(g, np.float32).reshape(-1, 5) for g in gts]
    g = np.concatenate(rows) if rows else np.zeros((0, 5), np.float32)
    gimg = np.concatenate([np.full(len(r), k, np.int64) for k, r in enumerate(rows)]) if rows else np.zeros(0, np.int64)
    keep = g[:, 4] >= 0
    g, gimg = g[keep], gimg[keep]
    gcls = g[:, 4].astype(np.int64)
    npos = np.bincount(gcls, minlength=C)[:C].astype(np.int64)
    gkey = gimg * (C + 1) + gcls
    gord = np.argsort(gkey, kind='stable')                                # row order inside each (image, class)
    gk = gkey[gord]
    gcorn = gt_corners(g[gord])
    dkey = img * (C + 1) + cls
    lo = np.searchsorted(gk, dkey, 'left')
    cnt = np.searchsorted(gk, dkey, 'right') - lo
    M = int(cnt.max()) if D and gk.size else 0
    best = np.full(D, -1.0, np.float32)
    bj = np.full(D, -1, np.int64)
    for m in range(M):                                                    # ascending row: strict > keeps the first maximum
        has = cnt > m
        j = lo[has] + m
        gb, db = gcorn[j], boxes[has]
        ih = np.fmax(np.fmin(db[:, 2], gb[:, 2]) - np.fmax(db[:, 0], gb[:, 0]), np.float32(0))
        iw = np.fmax(np.fmin(db[:, 3], gb[:, 3]) - np.fmax(db[:, 1], gb[:, 1]), np.float32(0))
        inter = ih * iw
        union = (db[:, 2] - db[:, 0]) * (db[:, 3] - db[:, 1]) + (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]) - inter
        with np.errstate(divide='ignore', invalid='ignore'):
            iou = np.where(union > 0, inter / np.where(union > 0, union, np.float32(1)), np.float32(0)).astype(np.float32)
        idx = np.nonzero(has)[0]
        up = iou > best[idx]
        best[idx[up]] = iou[up]
        bj[idx[up]] = j[up]
    order = np.lexsort((np.arange(D), -scores, cls))                      # class, score descending, sequence
    tp = np.zeros(D, np.uint8)
    cand = order[(bj[order] >= 0) & (best[order] > np.float32(iou_threshold))]
    _, first = np.unique(bj[cand], return_index=True)                     # (a GT row belongs to one (image, class): its index is the key)
    tp[cand[first]] = 1
    ap = np.full(C, np.nan)
    cs = cls[order]
    starts = np.searchsorted(cs, np.arange(C + 1), 'left')
    for c in range(C):
        ap[c] = average_precision(tp[order[starts[c]: starts[c + 1]]], npos[c], metric)
    valid = ~np.isnan(ap)
    return {'mAP': float(np.mean(ap[valid])) if valid.any() else float('nan'), 'AP': ap, 'npos': npos,
            'num_detections': np.bincount(cls, minlength=C)[:C].astype(np.int64), 'tp': tp}


def evaluate(dets, gts, num_classes, iou_threshold=0.5, metric='voc07'):
    """dets: per image (scores f32[K], boxes f32[K, 4], cls i32[K]); gts: per image f32[pad, 5].
    -> dict(mAP, AP f64[C], npos i64[C], num_detections i64[C], tp u8[sum K] in sequence order)"""
    scores, boxes, cls, img = _flatten(dets, gts)
    C = int(num_classes)
    rows = [np.asarray(g, np.float32).reshape(-1, 5) for g in gts]
    npos = np.zeros(C, np.int64)
    for r in rows:
        for c in r[:, 4]:
            if c >= 0:
                npos[int(c)] += 1
    tp = np.zeros(scores.shape[0], np.uint8)
    ap = np.full(C, np.nan)
    for c in range(C):
        sel = np.nonzero(cls == c)[0]                                   # sequence order
        order = sel[np.argsort(-scores[sel], kind='stable')]             # global rank of the class
        taken = {}
        for i in order:
            m = int(img[i])
            r = rows[m] if m < len(rows) else np.zeros((0, 5), np.float32)
            mine = np.nonzero(r[:, 4] == c)[0]
            if mine.size:
                ious = iou_f32(boxes[i], gt_corners(r[mine]))
                j = int(np.argmax(ious))
                if ious[j] > np.float32(iou_threshold) and (m, j) not in taken:
                    taken[(m, j)] = True
                    tp[i] = 1
        ap[c] = average_precision(tp[order], npos[c], metric)
    valid = ~np.isnan(ap)
    return {'mAP': float(np.mean(ap[valid])) if valid.any() else float('nan'), 'AP': ap, 'npos': npos,
            'num_detections': np.bincount(cls, minlength=C)[:C] if cls.size else np.zeros(C, np.int64), 'tp': tp}
