"""NumPy restatement of the COCO-style metric that csrc/voc_eval.hip computes (include/odtk.h, odtk_coco_eval): the yardstick of
tests/test_cpu_coco_eval.py and tests/test_gpu_coco_eval.py.  It never calls the library.

pycocotools' evaluateImg / accumulate without crowd regions, on the project's f32 IoU (voc_eval_ref.iou_f32: the kernel's operation order):
  * per (image, class) the detections are ranked by descending score, ties to the lower sequence index; the first max_dets take part, the rest get code 2;
  * for area range r a GT row is ignored iff h * w < lo or h * w > hi (f32); the rows are visited non-ignored first, then ignored, each in row order;
  * for threshold t each detection, in rank order, starts with best = thr[t], m = none and walks the rows: skip a matched row; stop when m is a non-ignored
    row and this one is ignored; skip when iou < best; else best = iou, m = row.  m becomes matched; the detection is TP (1) if m is not ignored, else
    ignored (2); without m it is ignored (2) if its own area (y2 - y1) * (x2 - x1) is outside [lo, hi], else FP (0);
  * npos[r][c] = non-ignored rows of class c; per (r, t, c) the code-0 / code-1 detections in global rank order give cumulative tp, fp,
    recall = tp / npos, precision = tp / (tp + fp + eps), the envelope (suffix max), q_k = envelope at the first position with recall >= x_k
    (x = np.linspace(0, 1, 101)), 0 without one; AP = mean(q); recall = the last recall (0 without counted detections); NaN where npos == 0.
evaluate() follows this text with plain loops; evaluate_fast() takes the k-th detection of every segment at once."""
import numpy as np

import voc_eval_ref as V

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10).astype(np.float32)
AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float32)
RECALL_POINTS = np.linspace(0, 1, 101)
EPS = np.finfo(np.float64).eps


def _args(iou_thresholds, area_ranges):
    thr = IOU_THRESHOLDS if iou_thresholds is None else np.asarray(iou_thresholds, np.float32).reshape(-1)
    rng = AREA_RANGES if area_ranges is None else np.asarray(area_ranges, np.float32).reshape(-1, 2)
    return thr, rng


def _nanmean(x):
    x = np.asarray(x, np.float64).reshape(-1)
    ok = ~np.isnan(x)
    return float(x[ok].mean()) if ok.any() else float('nan')


def summarize(ap, recall, thr):
    """the summary numbers of COCOEvaluator.result() from ap / recall [R, T, C]"""
    R, _, C = ap.shape

    def at(v):
        k = np.nonzero(np.abs(thr - np.float32(v)) < 1e-6)[0]
        return _nanmean(ap[0, k[0]]) if k.size else float('nan')
    nan = float('nan')
    return {'AP': _nanmean(ap[0]), 'AP50': at(0.5), 'AP75': at(0.75), 'APs': _nanmean(ap[1]) if R >= 4 else nan,
            'APm': _nanmean(ap[2]) if R >= 4 else nan, 'APl': _nanmean(ap[3]) if R >= 4 else nan, 'AR': _nanmean(recall[0]),
            'AP_per_class': np.array([_nanmean(ap[0, :, c]) for c in range(C)])}


def average_precision(codes, npos):
    """codes along the class's global rank order (0 FP, 1 TP, 2 not counted) -> (AP, last recall) in f64, plain loops"""
    if npos == 0:
        return float('nan'), float('nan')
    tp = fp = 0
    rec, prec = [], []
    for c in codes:
        if c == 2:
            continue
        tp += int(c == 1)
        fp += int(c == 0)
        rec.append(tp / float(npos))
        prec.append(tp / (tp + fp + EPS))
    for k in range(len(prec) - 2, -1, -1):                                  # the envelope: suffix max
        prec[k] = max(prec[k], prec[k + 1])
    q = np.zeros(101)
    pos = 0
    for k, x in enumerate(RECALL_POINTS):                                  # x ascends and so does recall: the first position only moves forward
        while pos < len(rec) and not rec[pos] >= x:
            pos += 1
        q[k] = prec[pos] if pos < len(rec) else 0.0
    return float(np.mean(q)), (rec[-1] if rec else 0.0)


def _accumulate_fast(match, scores, cls, npos, C):
    P = match.shape[0]
    R = npos.shape[0]
    T = P // R
    D = scores.shape[0]
    order = np.lexsort((np.arange(D), -scores, cls))
    starts = np.searchsorted(cls[order], np.arange(C + 1), 'left')
    ap = np.full((R, T, C), np.nan)
    rec = np.full((R, T, C), np.nan)
    for c in range(C):
        o = order[starts[c]: starts[c + 1]]
        for r in range(R):
            if npos[r, c] == 0:
                continue
            for t in range(T):
                codes = match[r * T + t, o]
                codes = codes[codes != 2]
                tp = np.cumsum(codes == 1).astype(np.float64)
                fp = np.cumsum(codes == 0).astype(np.float64)
                rc = tp / float(npos[r, c])
                pr = tp / (tp + fp + EPS)
                pr = np.maximum.accumulate(pr[::-1])[::-1]
                inds = np.searchsorted(rc, RECALL_POINTS, 'left')
                q = np.where(inds < len(pr), pr[np.minimum(inds, len(pr) - 1)], 0.0) if len(pr) else np.zeros(101)
                ap[r, t, c] = float(np.mean(q))
                rec[r, t, c] = rc[-1] if len(rc) else 0.0
    return ap, rec


def _result(match, npos, ap, rec, cls, C, thr, rng):
    R, T = rng.shape[0], thr.shape[0]
    out = {'match': match.reshape(R, T, -1), 'npos': npos, 'ap': ap, 'recall': rec, 'num_detections': np.bincount(cls, minlength=C)[:C].astype(np.int64),
           'iou_thresholds': thr, 'area_ranges': rng}
    out.update(summarize(ap, rec, thr))
    return out


def evaluate(dets, gts, num_classes, iou_thresholds=None, area_ranges=None, max_dets=100):
    """dets: per image (scores f32[K], boxes f32[K, 4], cls i32[K]); gts: per image f32[pad, 5] -> dict(match u8[R, T, D] in sequence order, npos i64[R, C],
    ap / recall f64[R, T, C], the summary numbers)"""
    thr, rng = _args(iou_thresholds, area_ranges)
    scores, boxes, cls, img = V._flatten(dets, gts)
    C, T, R, D = int(num_classes), thr.shape[0], rng.shape[0], scores.shape[0]
    rows = [np.asarray(g, np.float32).reshape(-1, 5) for g in gts]
    match = np.full((R * T, D), 2, np.uint8)
    npos = np.zeros((R, C), np.int64)
    for g in rows:
        for row in g:
            if row[4] >= 0:
                area = row[2] * row[3]
                for r in range(R):
                    if not (area < rng[r, 0] or area > rng[r, 1]):
                        npos[r, int(row[4])] += 1
    for m in range(len(dets)):
        for c in np.unique(cls[img == m]):
            sel = np.nonzero((img == m) & (cls == c))[0]
            kept = sel[np.argsort(-scores[sel], kind='stable')][:max_dets]
            g = rows[m][rows[m][:, 4] == c] if m < len(rows) else np.zeros((0, 5), np.float32)
            corners = V.gt_corners(g)
            garea = g[:, 2] * g[:, 3]
            ious = [V.iou_f32(boxes[i], corners) for i in kept]
            for r in range(R):
                lo, hi = rng[r]
                ign = (garea < lo) | (garea > hi)
                visit = [j for j in range(len(g)) if not ign[j]] + [j for j in range(len(g)) if ign[j]]
                for t in range(T):
                    matched = set()
                    for k, i in enumerate(kept):
                        best, mrow = thr[t], None
                        for j in visit:
                            if j in matched:
                                continue
                            if mrow is not None and not ign[mrow] and ign[j]:
                                break
                            if ious[k][j] < best:
                                continue
                            best, mrow = ious[k][j], j
                        if mrow is not None:
                            matched.add(mrow)
                            code = 2 if ign[mrow] else 1
                        else:
                            b = boxes[i]
                            area = (b[2] - b[0]) * (b[3] - b[1])
                            code = 2 if (area < lo or area > hi) else 0
                        match[r * T + t, i] = code
    ap = np.full((R, T, C), np.nan)
    rec = np.full((R, T, C), np.nan)
    for c in range(C):
        sel = np.nonzero(cls == c)[0]
        order = sel[np.argsort(-scores[sel], kind='stable')]
        for r in range(R):
            for t in range(T):
                ap[r, t, c], rec[r, t, c] = average_precision(match[r * T + t, order], npos[r, c])
    return _result(match, npos, ap, rec, cls, C, thr, rng)


def evaluate_fast(dets, gts, num_classes, iou_thresholds=None, area_ranges=None, max_dets=100):
    """evaluate() with the k-th ranked detection of every (image, class) segment handled at once, all (r, t) pairs side by side: a segment's state is its
    own GT rows' matched flags, so segments do not interact.  The walk over the rows collapses to: among the untaken non-ignored rows with
    iou >= thr the largest IoU, the later row among equals; without one, the same among the ignored rows."""
    thr, rng = _args(iou_thresholds, area_ranges)
    scores, boxes, cls, img = V._flatten(dets, gts)
    C, T, R, D = int(num_classes), thr.shape[0], rng.shape[0], scores.shape[0]
    P = R * T
    pr, pt = np.repeat(np.arange(R), T), np.tile(np.arange(T), R)           # pair -> (r, t)
    rows = [np.asarray(g, np.float32).reshape(-1, 5) for g in gts]
    g = np.concatenate(rows) if rows else np.zeros((0, 5), np.float32)
    gimg = np.concatenate([np.full(len(x), k, np.int64) for k, x in enumerate(rows)]) if rows else np.zeros(0, np.int64)
    keep = g[:, 4] >= 0
    g, gimg = g[keep], gimg[keep]
    gcls = g[:, 4].astype(np.int64)
    garea = g[:, 2] * g[:, 3]
    ign_r = (garea[:, None] < rng[None, :, 0]) | (garea[:, None] > rng[None, :, 1])            # [G, R]
    npos = np.zeros((R, C), np.int64)
    for r in range(R):
        npos[r] = np.bincount(gcls[~ign_r[:, r]], minlength=C)[:C]
    gkey = gimg * (C + 1) + gcls
    gord = np.argsort(gkey, kind='stable')
    gk, gcorn, ign = gkey[gord], V.gt_corners(g[gord]), ign_r[gord][:, pr]                    # ign [G, P]
    dkey = img * (C + 1) + cls
    lo = np.searchsorted(gk, dkey, 'left')
    cnt = np.searchsorted(gk, dkey, 'right') - lo
    order = np.lexsort((np.arange(D), -scores, dkey))                      # segments, rank order inside
    ks = dkey[order]
    first = np.searchsorted(ks, ks, 'left')
    rank = np.empty(D, np.int64)
    rank[order] = np.arange(D) - first
    darea = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    outside = (darea[:, None] < rng[None, :, 0]) | (darea[:, None] > rng[None, :, 1])          # [D, R]
    match = np.full((P, D), 2, np.uint8)
    taking = rank < max_dets
    lone = taking & (cnt == 0)                                              # no GT row of its (image, class): FP unless its area is outside
    match[:, lone] = np.where(outside[lone][:, pr], 2, 0).astype(np.uint8).T
    matched = np.zeros((gk.shape[0], P), bool)
    pcol = np.arange(P)[None, :]
    for k in range(int(min(max_dets, rank.max() + 1)) if D else 0):
        ids = np.nonzero((rank == k) & (cnt > 0))[0]
        if ids.size == 0:
            continue
        M = int(cnt[ids].max())
        col = np.arange(M)[None, :]
        valid = col < cnt[ids][:, None]
        gpos = np.where(valid, lo[ids][:, None] + col, 0)                   # [n, M]
        gb, db = gcorn[gpos], boxes[ids][:, None, :]
        ih = np.fmax(np.fmin(db[..., 2], gb[..., 2]) - np.fmax(db[..., 0], gb[..., 0]), np.float32(0))
        iw = np.fmax(np.fmin(db[..., 3], gb[..., 3]) - np.fmax(db[..., 1], gb[..., 1]), np.float32(0))
        inter = ih * iw
        union = (db[..., 2] - db[..., 0]) * (db[..., 3] - db[..., 1]) + (gb[..., 2] - gb[..., 0]) * (gb[..., 3] - gb[..., 1]) - inter
        with np.errstate(divide='ignore', invalid='ignore'):
            iou = np.where(union > 0, inter / np.where(union > 0, union, np.float32(1)), np.float32(0)).astype(np.float32)
        avail = valid[:, :, None] & ~matched[gpos] & (iou[:, :, None] >= thr[pt][None, None, :])   # [n, M, P]
        gi = ign[gpos]
        neg = np.float32(-1)
        val_n = np.where(avail & ~gi, iou[:, :, None], neg)
        val_i = np.where(avail & gi, iou[:, :, None], neg)
        j_n = M - 1 - np.argmax(val_n[:, ::-1, :], axis=1)                 # the later row among equal maxima
        j_i = M - 1 - np.argmax(val_i[:, ::-1, :], axis=1)
        has_n, has_i = val_n.max(axis=1) >= 0, val_i.max(axis=1) >= 0
        j = np.where(has_n, j_n, j_i)
        has = has_n | has_i
        code = np.where(has_n, 1, np.where(has_i, 2, np.where(outside[ids][:, pr], 2, 0))).astype(np.uint8)
        grow = np.take_along_axis(gpos, j, axis=1)                          # [n, P]
        matched[grow[has], np.broadcast_to(pcol, has.shape)[has]] = True
        match[:, ids] = code.T
    ap, rec = _accumulate_fast(match, scores, cls, npos, C)
    return _result(match, npos, ap, rec, cls, C, thr, rng)


def random_case(seed, n_img, C, det_per_img, gt_per_img, levels=8, cls_per_img=2):
    """a synthetic set built to stress the matcher: each image draws its GT and most detections from `cls_per_img` classes (segments with several rows
    and several detections), box sides from 8 to 160 px (all three size ranges, some areas exactly 32^2 and 96^2), a fifth of the GT rows duplicates of
    their neighbour (equal IoUs), 70 % of the detections jittered GT boxes (IoUs spread over the thresholds) and a tenth exact copies (IoU 1), scores
    quantised to `levels` values (heavy ties), one padding row per image"""
    rng = np.random.default_rng(seed)
    G = n_img * gt_per_img
    side = np.array([8, 16, 32, 32, 48, 64, 96, 96, 128, 160], np.float64)
    yc, xc = rng.uniform(80, 400, G), rng.uniform(80, 400, G)
    h = np.where(rng.random(G) < 0.3, side[rng.integers(0, len(side), G)], rng.uniform(8, 160, G))
    w = np.where(rng.random(G) < 0.3, h, rng.uniform(8, 160, G))
    img_cls = rng.integers(0, C, (n_img, cls_per_img))
    gcls = img_cls[np.repeat(np.arange(n_img), gt_per_img), rng.integers(0, cls_per_img, G)]
    dup = (rng.random(G) < 0.2) & (np.arange(G) % gt_per_img > 0)
    for a in (yc, xc, h, w, gcls):
        a[dup] = a[np.nonzero(dup)[0] - 1]
    gt = np.stack([yc, xc, h, w, gcls], 1).astype(np.float32).reshape(n_img, gt_per_img, 5)
    gt = np.concatenate([gt, -np.ones((n_img, 1, 5), np.float32)], 1)
    D = n_img * det_per_img
    img = np.repeat(np.arange(n_img), det_per_img)
    j = img * gt_per_img + rng.integers(0, gt_per_img, D)
    u = rng.random(D)
    hit, exact = u < 0.8, u < 0.1
    y1 = np.where(hit, yc[j] - h[j] / 2, rng.uniform(0, 400, D))
    x1 = np.where(hit, xc[j] - w[j] / 2, rng.uniform(0, 400, D))
    y2 = np.where(hit, yc[j] + h[j] / 2, y1 + rng.uniform(5, 150, D))
    x2 = np.where(hit, xc[j] + w[j] / 2, x1 + rng.uniform(5, 150, D))
    jit = (hit & ~exact)[:, None] * rng.normal(0, 0.08, (D, 4)) * np.stack([h[j], w[j], h[j], w[j]], 1)
    box = np.stack([y1, x1, y2, x2], 1) + jit
    dcls = np.where(hit & (rng.random(D) < 0.9), gcls[j], img_cls[img, rng.integers(0, cls_per_img, D)])
    dcls = np.where(rng.random(D) < 0.05, rng.integers(0, C, D), dcls)
    score = rng.integers(1, levels + 1, D) / levels
    sc = np.split(score.astype(np.float32), n_img)
    bx = np.split(box.astype(np.float32), n_img)
    cl = np.split(dcls.astype(np.int32), n_img)
    return list(zip(sc, bx, cl)), list(gt)
