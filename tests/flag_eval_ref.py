"""NumPy restatement of the two evaluation protocols WITH ground-truth flags (include/odtk.h, odtk_voc_eval_flags / odtk_coco_eval_flags): the
yardstick of tests/test_cpu_flag_eval.py and tests/test_gpu_flag_eval.py.  It never calls the library, and it is written from the protocols -- the
PASCAL VOC devkit's VOCevaldet and pycocotools' evaluateImg -- with plain loops; the IoU and the AP sums are those of voc_eval_ref.py / coco_eval_ref.py.

A flag per ground-truth row: 0 an ordinary object, 1 ignore (VOC `difficult`; pycocotools' `ignore` with iscrowd = 0), 2 crowd (iscrowd = 1).

VOC (voc_evaluate): ranking and IoU as voc_eval_ref.  Each detection, in rank order, looks at the first row of its (image, class) with the largest IoU
over ALL rows.  IoU > threshold and the row flagged: code 2, the row is not taken.  IoU > threshold, flag 0, row free: code 1, the row is taken.
Otherwise code 0.  npos = flag-0 rows, num_ignored_gt = flagged rows.  AP over the code-0 / code-1 detections only; NaN when npos == 0.

COCO (coco_evaluate): as coco_eval_ref, except: a row is ignored for range r iff its flag is non-zero or its area is outside the range; a matched row
is skipped only if its flag is not 2 (a crowd row absorbs any number of detections); the overlap with a flag-2 row is intersection / detection area
(f32, 0 unless the detection's area is > 0).  The result also has 'max_crowd_hits': the largest number of detections that one crowd row took at one
(r, t) -- what a test reads to see that its data exercises the rule.

Without flags both functions do exactly what voc_eval_ref.evaluate / coco_eval_ref.evaluate do (tests/test_cpu_flag_eval.py checks it)."""
import numpy as np

import coco_eval_ref as C
import voc_eval_ref as V


def _flag_rows(gts, flags):
    rows = [np.asarray(g, np.float32).reshape(-1, 5) for g in gts]
    if flags is None:
        flags = [None] * len(rows)
    out = []
    for r, f in zip(rows, flags):
        f = np.zeros(len(r), np.int64) if f is None else np.asarray(f).astype(np.int64).reshape(-1)
        assert f.shape[0] == r.shape[0]
        out.append(f)
    return rows, out


def overlap_f32(box, corners, crowd):
    """box f32[4] against corners f32[n, 4]: IoU (voc_eval_ref.iou_f32), or intersection / area of `box` where crowd[n] is set"""
    box = np.asarray(box, np.float32)
    corners = np.asarray(corners, np.float32).reshape(-1, 4)
    iou = V.iou_f32(box, corners)
    ih = np.fmax(np.fmin(box[2], corners[:, 2]) - np.fmax(box[0], corners[:, 0]), np.float32(0))
    iw = np.fmax(np.fmin(box[3], corners[:, 3]) - np.fmax(box[1], corners[:, 1]), np.float32(0))
    inter = ih * iw
    area = (box[2] - box[0]) * (box[3] - box[1])
    with np.errstate(divide='ignore', invalid='ignore'):
        ioa = (inter / area).astype(np.float32) if area > 0 else np.zeros(len(corners), np.float32)
    return np.where(np.asarray(crowd, bool), ioa, iou).astype(np.float32)


def voc_evaluate(dets, gts, num_classes, flags=None, iou_threshold=0.5, metric='voc07'):
    """dets / gts as voc_eval_ref.evaluate; flags: per image an int array [pad] (or None = zeros), or None for no flags at all
    -> dict(mAP, AP, npos, num_ignored_gt, num_detections, match u8[D] (0 FP, 1 TP, 2 on a flagged row), tp = (match == 1))"""
    scores, boxes, cls, img = V._flatten(dets, gts)
    Cn = int(num_classes)
    rows, fl = _flag_rows(gts, flags)
    npos, nign = np.zeros(Cn, np.int64), np.zeros(Cn, np.int64)
    for r, f in zip(rows, fl):
        for c, x in zip(r[:, 4], f):
            if c >= 0:
                (nign if x else npos)[int(c)] += 1
    match = np.zeros(scores.shape[0], np.uint8)
    ap = np.full(Cn, np.nan)
    for c in range(Cn):
        sel = np.nonzero(cls == c)[0]
        order = sel[np.argsort(-scores[sel], kind='stable')]
        taken = set()
        for i in order:
            m = int(img[i])
            r = rows[m] if m < len(rows) else np.zeros((0, 5), np.float32)
            mine = np.nonzero(r[:, 4] == c)[0]
            if mine.size == 0:
                continue
            ious = V.iou_f32(boxes[i], V.gt_corners(r[mine]))
            j = int(np.argmax(ious))                                       # the first of the largest, over all rows
            if not ious[j] > np.float32(iou_threshold):
                continue
            if fl[m][mine[j]]:
                match[i] = 2                                                # difficult: not counted, and the row is not taken
            elif (m, j) not in taken:
                taken.add((m, j))
                match[i] = 1
        codes = match[order]
        ap[c] = V.average_precision(codes[codes != 2], npos[c], metric)
    valid = ~np.isnan(ap)
    return {'mAP': float(np.mean(ap[valid])) if valid.any() else float('nan'), 'AP': ap, 'npos': npos, 'num_ignored_gt': nign,
            'num_detections': np.bincount(cls, minlength=Cn)[:Cn] if cls.size else np.zeros(Cn, np.int64), 'match': match,
            'tp': (match == 1).astype(np.uint8)}


def coco_evaluate(dets, gts, num_classes, flags=None, iou_thresholds=None, area_ranges=None, max_dets=100):
    """coco_eval_ref.evaluate with flags (see the module text) -> its dict + 'num_ignored_gt' i64[C] + 'max_crowd_hits'"""
    thr, rng = C._args(iou_thresholds, area_ranges)
    scores, boxes, cls, img = V._flatten(dets, gts)
    Cn, T, R, D = int(num_classes), thr.shape[0], rng.shape[0], scores.shape[0]
    rows, fl = _flag_rows(gts, flags)
    match = np.full((R * T, D), 2, np.uint8)
    npos = np.zeros((R, Cn), np.int64)
    nign = np.zeros(Cn, np.int64)
    for g, f in zip(rows, fl):
        for row, x in zip(g, f):
            if row[4] >= 0:
                if x:
                    nign[int(row[4])] += 1
                    continue
                area = row[2] * row[3]
                for r in range(R):
                    if not (area < rng[r, 0] or area > rng[r, 1]):
                        npos[r, int(row[4])] += 1
    crowd_hits = 0
    for m in range(len(dets)):
        for c in np.unique(cls[img == m]):
            sel = np.nonzero((img == m) & (cls == c))[0]
            kept = sel[np.argsort(-scores[sel], kind='stable')][:max_dets]
            mine = np.nonzero(rows[m][:, 4] == c)[0] if m < len(rows) else np.zeros(0, np.int64)
            g = rows[m][mine] if mine.size else np.zeros((0, 5), np.float32)
            gf = fl[m][mine] if mine.size else np.zeros(0, np.int64)
            corners = V.gt_corners(g)
            garea = g[:, 2] * g[:, 3]
            ious = [overlap_f32(boxes[i], corners, gf == 2) for i in kept]
            for r in range(R):
                lo, hi = rng[r]
                ign = (gf != 0) | (garea < lo) | (garea > hi)
                visit = [j for j in range(len(g)) if not ign[j]] + [j for j in range(len(g)) if ign[j]]
                for t in range(T):
                    hits = {}
                    for k, i in enumerate(kept):
                        best, mrow = thr[t], None
                        for j in visit:
                            if j in hits and gf[j] != 2:                    # matched already, and no crowd
                                continue
                            if mrow is not None and not ign[mrow] and ign[j]:
                                break
                            if ious[k][j] < best:
                                continue
                            best, mrow = ious[k][j], j
                        if mrow is not None:
                            hits[mrow] = hits.get(mrow, 0) + 1
                            code = 2 if ign[mrow] else 1
                        else:
                            b = boxes[i]
                            area = (b[2] - b[0]) * (b[3] - b[1])
                            code = 2 if (area < lo or area > hi) else 0
                        match[r * T + t, i] = code
                    crowd_hits = max([crowd_hits] + [n for j, n in hits.items() if gf[j] == 2])
    ap = np.full((R, T, Cn), np.nan)
    rec = np.full((R, T, Cn), np.nan)
    for c in range(Cn):
        sel = np.nonzero(cls == c)[0]
        order = sel[np.argsort(-scores[sel], kind='stable')]
        for r in range(R):
            for t in range(T):
                ap[r, t, c], rec[r, t, c] = C.average_precision(match[r * T + t, order], npos[r, c])
    out = C._result(match, npos, ap, rec, cls, Cn, thr, rng)
    out['num_ignored_gt'] = nign
    out['max_crowd_hits'] = int(crowd_hits)
    return out
