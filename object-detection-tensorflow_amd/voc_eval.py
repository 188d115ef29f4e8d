"""PASCAL VOC mean average precision over a validation set (BASELINE.json's "mAP parity"; the reference builds a val_generator and never reads it,
testSSD300.py:56-58).

`VOCEvaluator` stages what `test_one_image` returns, image by image, on the host; `result()` packs everything into one buffer, uploads it once and runs
csrc/voc_eval.hip (odtk_voc_eval: matching, per-class rank order and AP on the device).  `evaluate(model)` drives a model over a generator with the
`train_generator` contract; every detector class has `evaluate()` through `EvaluateMixin`.  The semantics (include/odtk.h) are restated in NumPy in
tests/voc_eval_ref.py.

Ground-truth rows may carry a flag: 0 an ordinary object, 1 ignore (VOC `difficult`), 2 crowd (COCO `iscrowd`) -- a sixth column of the ground truth or
`add(..., flags=)`.  Once any image was given flags the evaluators call odtk_voc_eval_flags / odtk_coco_eval_flags (restated in tests/flag_eval_ref.py);
without flags the calls, the upload and the read-back are the unflagged ones."""
from __future__ import annotations

import numpy as np
import torch

from . import ops

METRICS = ('voc07', 'area')


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


class _StagedEvaluator:
    """what VOCEvaluator and COCOEvaluator share: the per-image staging on the host, the checked flat arrays and the one upload"""

    def _init_common(self, num_classes, device):
        if not 1 <= int(num_classes) <= 1024:
            raise ValueError(f"num_classes must be in [1, 1024], not {num_classes}")
        self.num_classes = int(num_classes)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        self._dets, self._gts, self._flags = [], [], []

    @property
    def num_images(self):
        return len(self._gts)

    @property
    def has_flags(self):
        return any(f is not None for f in self._flags)

    def add(self, detections, ground_truth, flags=None):
        """stage one image: no device work, no synchronisation (device tensors are kept as they are until result()).  ground_truth [pad, 5], or
        [pad, 6] with the flag (0 ordinary, 1 ignore, 2 crowd) in column 5; or flags = an integer / bool array [pad] (True = 1), not both.  The flag
        VALUES are checked in result(), with everything else that needs the host copy."""
        if not isinstance(detections, (list, tuple)) or len(detections) != 3:
            raise ValueError("detections must be [scores [K], bbox [K, 4], class_id [K]] as test_one_image returns them")
        s, b, c = detections
        k = tuple(s.shape)
        if len(k) != 1 or tuple(b.shape) != (k[0], 4) or tuple(c.shape) != k:
            raise ValueError(f"detections: scores {tuple(s.shape)}, bbox {tuple(b.shape)}, class_id {tuple(c.shape)} do not form [K], [K, 4], [K]")
        g = ground_truth
        if g.ndim != 2 or g.shape[1] not in (5, 6):
            raise ValueError(f"ground_truth must be [pad, 5] rows (yc, xc, h, w, cls) or [pad, 6] rows (.., flag), not {tuple(g.shape)}")
        n = self.num_images
        if g.shape[1] == 6:
            if flags is not None:
                raise ValueError(f"image {n}: flags given twice, as column 5 of ground_truth and as flags=")
            g, flags = g[:, :5], g[:, 5]
        elif flags is not None:
            if not isinstance(flags, torch.Tensor):
                flags = np.asarray(flags)
            if flags.ndim != 1 or flags.shape[0] != g.shape[0]:
                raise ValueError(f"image {n}: flags must be [pad] = [{g.shape[0]}] like the ground truth, not {tuple(flags.shape)}")
            kind = 'f' if isinstance(flags, torch.Tensor) and flags.dtype.is_floating_point else (
                'i' if isinstance(flags, torch.Tensor) else flags.dtype.kind)
            if kind not in 'iub':
                raise ValueError(f"image {n}: flags must be an integer or bool array, not {flags.dtype}")
        self._dets.append((s, b, c))
        self._gts.append(g)
        self._flags.append(flags)

    def _pack(self, with_flags=False):
        """the staged images as flat host arrays, checked (vectorised over all images: no per-image work beyond the conversions); with_flags: a
        seventh array, the flags u8 [G] of the rows that stay (images staged without flags: 0)"""
        C = self.num_classes
        sc = [np.asarray(_host(d[0]), np.float32).reshape(-1) for d in self._dets]
        bx = [np.asarray(_host(d[1]), np.float32).reshape(-1, 4) for d in self._dets]
        cl = [_host(d[2]).reshape(-1) for d in self._dets]
        n = len(sc)
        scores = np.concatenate(sc) if n else np.zeros(0, np.float32)
        boxes = np.concatenate(bx) if n else np.zeros((0, 4), np.float32)
        cls_raw = np.concatenate(cl) if n else np.zeros(0, np.int64)
        img = np.repeat(np.arange(n, dtype=np.int32), [len(s) for s in sc]) if n else np.zeros(0, np.int32)
        if cls_raw.size and cls_raw.dtype.kind not in 'iu' and not np.all(cls_raw == np.round(cls_raw)):
            raise ValueError("detections: class_id must hold integers")
        cls = np.asarray(cls_raw, np.int64)
        if not np.all(np.isfinite(scores)):
            raise ValueError(f"detections of image {int(img[np.argmin(np.isfinite(scores))])}: non-finite score")
        bad = (cls < 0) | (cls >= C)
        if bad.any():
            raise ValueError(f"detections of image {int(img[np.argmax(bad)])}: class_id {int(cls[np.argmax(bad)])} outside [0, {C})")
        gl = [np.asarray(_host(g), np.float32).reshape(-1, 5) for g in self._gts]
        rows = np.concatenate(gl) if gl else np.zeros((0, 5), np.float32)
        rimg = np.repeat(np.arange(len(gl), dtype=np.int32), [len(g) for g in gl]) if gl else np.zeros(0, np.int32)
        keep = rows[:, 4] >= 0                                                   # cls < 0: padding
        gt, gi = rows[keep], rimg[keep]
        if with_flags:                                                           # padding rows go together with their flags
            fl = [np.zeros(len(g), np.int64) if f is None else _host(f).reshape(-1) for g, f in zip(gl, self._flags)]
            raw = (np.concatenate([np.asarray(f, np.float64) for f in fl]) if fl else np.zeros(0))[keep]
            bad = ~((raw == 0) | (raw == 1) | (raw == 2))
            if bad.any():
                raise ValueError(f"ground_truth of image {int(gi[np.argmax(bad)])}: flag {raw[np.argmax(bad)]:g} is not 0 (ordinary), 1 (ignore) "
                                 f"or 2 (crowd)")
            flags = raw.astype(np.uint8)
        bad = ~np.all(np.isfinite(gt), 1) | (gt[:, 4] != np.round(gt[:, 4]))
        if bad.any():
            raise ValueError(f"ground_truth of image {int(gi[np.argmax(bad)])}: non-finite value or non-integer class")
        bad = gt[:, 4] >= C
        if bad.any():
            raise ValueError(f"ground_truth of image {int(gi[np.argmax(bad)])}: class {int(gt[np.argmax(bad), 4])} >= num_classes {C}")
        out = scores, boxes, cls.astype(np.int32), img, np.ascontiguousarray(gt), gi
        return out + (flags,) if with_flags else out

    def _upload(self, with_flags=False):
        """_pack() as one host buffer of 4-byte words (scores | boxes | det_cls | det_img | gt_rows | gt_img), uploaded once -> the six device views in
        the argument order of odtk_voc_eval / odtk_coco_eval, and the host class ids.  with_flags: the flag bytes ride at the end of the same buffer
        (padded to whole words) -> (the six views, host class ids, device flags u8 [G], host flagged rows per class i64 [C])"""
        packed = self._pack(with_flags)
        scores, boxes, cls, img, gt, gi = packed[:6]
        D, G = scores.shape[0], gt.shape[0]
        parts = [scores.view(np.int32), boxes.reshape(-1).view(np.int32), cls, img, gt.reshape(-1).view(np.int32), gi]
        if with_flags:
            words = np.zeros((G + 3) // 4 * 4, np.uint8)
            words[:G] = packed[6]
            parts.append(words.view(np.int32))
        host = torch.from_numpy(np.concatenate([np.ascontiguousarray(p, np.int32).reshape(-1) for p in parts]) if D + G else np.zeros(1, np.int32))
        dev = host.to(self.device)
        offs = np.cumsum([0] + [p.size for p in parts])
        seg = [dev[offs[k]: offs[k + 1]] for k in range(len(parts))]
        six = (seg[0].view(torch.float32), seg[1].view(torch.float32).view(-1, 4), seg[2], seg[3], seg[4].view(torch.float32).view(-1, 5), seg[5])
        if not with_flags:
            return six, cls
        nign = np.bincount(gt[:, 4].astype(np.int64)[packed[6] > 0], minlength=self.num_classes).astype(np.int64)
        return six, cls, seg[6].view(torch.uint8)[:G], nign


class VOCEvaluator(_StagedEvaluator):
    """add(detections, ground_truth) per image, result() once.  detections = [scores f32[K], bbox f32[K, 4] (y1, x1, y2, x2 px), class_id i32[K]]
    (what every class's test_one_image returns; numpy or torch, host or device), ground_truth = f32[pad, 5] rows (yc, xc, h, w, cls px; cls < 0 =
    padding).  Input errors raise ValueError; library errors OdtkError.  Flags (a sixth ground-truth column or add(..., flags=)): a row flagged 1
    (VOC `difficult`) or 2 is no positive, and a detection whose best overlap is such a row is neither a true nor a false positive -- the devkit's
    VOCevaldet (include/odtk.h, odtk_voc_eval_flags)."""

    def __init__(self, num_classes, iou_threshold=0.5, metric='voc07', device=None):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
        if not 1 <= int(num_classes) <= 1024:
            raise ValueError(f"num_classes must be in [1, 1024], not {num_classes}")
        if not 0.0 <= float(iou_threshold) < 1.0:
            raise ValueError(f"iou_threshold must be in [0, 1), not {iou_threshold}")
        self.iou_threshold = float(iou_threshold)
        self.metric = metric
        self._init_common(num_classes, device)

    def result(self):
        """one upload, one odtk_voc_eval (odtk_voc_eval_flags once an image was given flags) -> {'mAP', 'AP' f64[C] (NaN: no unflagged GT), 'npos'
        (unflagged GT rows), 'num_ignored_gt' (flagged ones), 'num_detections', 'match' u8[D] in sequence order (0 FP, 1 TP, 2 on a flagged row: not
        counted), 'tp' u8[D] = (match == 1)}"""
        flagged = self.has_flags
        if flagged:
            dev, cls, gfl, _ = self._upload(True)
        else:
            dev, cls = self._upload()
        D, G, C = dev[0].shape[0], dev[4].shape[0], self.num_classes
        I = max(self.num_images, 1)
        ws = ops.voc_eval_workspace(D, G, I, C, self.device)
        tp = torch.empty(D, dtype=torch.uint8, device=self.device)
        npos = torch.empty(C, dtype=torch.int32, device=self.device)
        ap = torch.empty(C, dtype=torch.float64, device=self.device)
        if flagged:
            nign = torch.empty(C, dtype=torch.int32, device=self.device)
            ops.voc_eval_flags(*dev, gfl, I, C, self.iou_threshold, self.metric, ws, tp, npos, nign, ap)
            nign_h = nign.cpu().numpy().astype(np.int64)
        else:
            ops.voc_eval(*dev, I, C, self.iou_threshold, self.metric, ws, tp, npos, ap)
            nign_h = np.zeros(C, np.int64)
        ap_h = ap.cpu().numpy()
        match = tp.cpu().numpy()
        valid = ~np.isnan(ap_h)
        return {'mAP': float(ap_h[valid].mean()) if valid.any() else float('nan'), 'AP': ap_h, 'npos': npos.cpu().numpy().astype(np.int64),
                'num_ignored_gt': nign_h, 'num_detections': np.bincount(cls, minlength=C).astype(np.int64), 'match': match,
                'tp': (match == 1).astype(np.uint8) if flagged else match}


COCO_IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10).astype(np.float32)
COCO_AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float32)       # all, small, medium, large (px^2)


def _nanmean(x):
    x = np.asarray(x, np.float64).reshape(-1)
    ok = ~np.isnan(x)
    return float(x[ok].mean()) if ok.any() else float('nan')


class COCOEvaluator(_StagedEvaluator):
    """COCO-style AP (include/odtk.h, odtk_coco_eval): add() / result() / reset() / num_images as VOCEvaluator.  iou_thresholds: ascending, distinct,
    inside [0, 1) (default 0.50:0.05:0.95); area_ranges [R, 2] (lo, hi in px^2; default all, small < 32^2, medium, large > 96^2), area range 0 is the one
    the summary numbers 'AP', 'AP50', 'AP75', 'AR' are taken at; max_dets: detections that count per (image, class), by descending score;
    len(iou_thresholds) * len(area_ranges) <= 64.  Against the VOC matcher: IoU >= threshold (not >), a detection takes the best row that is NOT yet
    matched (not "the best row, if it is free"), and rows / detections outside the area range are ignored rather than counted.  Flags (a sixth
    ground-truth column or add(..., flags=)): a row flagged 1 is ignored in every range (matched once, its detection gets code 2); a row flagged 2 is a
    crowd region: ignored too, its overlap is intersection / detection area, and it absorbs any number of detections (odtk_coco_eval_flags)."""

    def __init__(self, num_classes, iou_thresholds=None, area_ranges=None, max_dets=100, device=None):
        thr = COCO_IOU_THRESHOLDS if iou_thresholds is None else np.asarray(iou_thresholds, np.float32).reshape(-1)
        rng = COCO_AREA_RANGES if area_ranges is None else np.asarray(area_ranges, np.float32)
        if thr.size < 1 or not np.all((thr >= 0) & (thr < 1)):
            raise ValueError(f"iou_thresholds must be a non-empty list of values in [0, 1), not {thr.tolist()}")
        if np.any(np.diff(thr) <= 0):
            raise ValueError(f"iou_thresholds must be ascending without duplicates, not {thr.tolist()}")
        if rng.ndim != 2 or rng.shape[1] != 2 or rng.shape[0] < 1 or np.any(np.isnan(rng)):
            raise ValueError(f"area_ranges must be [R, 2] rows (lo, hi), R >= 1, not shape {tuple(rng.shape)}")
        if np.any(rng[:, 0] > rng[:, 1]):
            raise ValueError(f"area_ranges: lo > hi in {rng.tolist()}")
        if thr.size * rng.shape[0] > 64:
            raise ValueError(f"len(iou_thresholds) * len(area_ranges) = {thr.size} * {rng.shape[0]} exceeds 64")
        if isinstance(max_dets, bool) or int(max_dets) != max_dets or int(max_dets) < 1:
            raise ValueError(f"max_dets must be an integer >= 1, not {max_dets!r}")
        self.iou_thresholds = np.ascontiguousarray(thr)
        self.area_ranges = np.ascontiguousarray(rng)
        self.max_dets = int(max_dets)
        self._init_common(num_classes, device)

    def result(self):
        """one upload, one odtk_coco_eval, one read-back -> {'AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR', 'AP_per_class' f64[C], 'ap' / 'recall' f64[R, T, C]
        (NaN: no GT), 'npos' [R, C], 'match' u8[R, T, D] in sequence order (0 FP, 1 TP, 2 ignored or dropped), 'num_detections', 'iou_thresholds',
        'area_ranges'}; once an image was given flags the call is odtk_coco_eval_flags and the result has 'num_ignored_gt' i64[C] (rows with a
        non-zero flag) as well"""
        flagged = self.has_flags
        if flagged:
            dev, cls, gfl, nign = self._upload(True)
        else:
            dev, cls = self._upload()
        D, G, C = dev[0].shape[0], dev[4].shape[0], self.num_classes
        T, R = self.iou_thresholds.shape[0], self.area_ranges.shape[0]
        I = max(self.num_images, 1)
        ws = ops.coco_eval_workspace(D, G, I, C, T, R, self.device)
        # one output buffer, one read-back: ap | recall (f64) | npos (i32) | match (u8)
        n_ap, n_pos = R * T * C * 8, R * C * 4
        out = torch.empty(2 * n_ap + n_pos + R * T * D, dtype=torch.uint8, device=self.device)
        ap = out[:n_ap].view(torch.float64).view(R, T, C)
        rec = out[n_ap: 2 * n_ap].view(torch.float64).view(R, T, C)
        npos = out[2 * n_ap: 2 * n_ap + n_pos].view(torch.int32).view(R, C)
        match = out[2 * n_ap + n_pos:].view(R, T, D)
        if flagged:
            ops.coco_eval_flags(*dev, gfl, I, C, self.iou_thresholds, self.area_ranges, self.max_dets, ws, match, npos, ap, rec)
        else:
            ops.coco_eval(*dev, I, C, self.iou_thresholds, self.area_ranges, self.max_dets, ws, match, npos, ap, rec)
        host = out.cpu().numpy()
        ap_h = host[:n_ap].view(np.float64).reshape(R, T, C)
        rec_h = host[n_ap: 2 * n_ap].view(np.float64).reshape(R, T, C)
        npos_h = host[2 * n_ap: 2 * n_ap + n_pos].view(np.int32).reshape(R, C).astype(np.int64)
        match_h = host[2 * n_ap + n_pos:].reshape(R, T, D)

        def at(value, r=0):
            k = np.nonzero(np.abs(self.iou_thresholds - np.float32(value)) < 1e-6)[0]
            return _nanmean(ap_h[r, k[0]]) if k.size else float('nan')
        four = R >= 4
        out = {'AP': _nanmean(ap_h[0]), 'AP50': at(0.5), 'AP75': at(0.75),
                'APs': _nanmean(ap_h[1]) if four else float('nan'), 'APm': _nanmean(ap_h[2]) if four else float('nan'),
                'APl': _nanmean(ap_h[3]) if four else float('nan'), 'AR': _nanmean(rec_h[0]),
                'AP_per_class': np.array([_nanmean(ap_h[0, :, c]) for c in range(C)]), 'ap': ap_h, 'recall': rec_h, 'npos': npos_h, 'match': match_h,
                'num_detections': np.bincount(cls, minlength=C).astype(np.int64), 'iou_thresholds': self.iou_thresholds.copy(),
                'area_ranges': self.area_ranges.copy()}
        if flagged:
            out['num_ignored_gt'] = nign
        return out


def _batches(generator):
    if isinstance(generator, tuple) and len(generator) == 2 and callable(generator[0]):
        initializer, iterator = generator
        initializer()
    else:
        iterator = generator
    return iter(iterator)


def _gt_width(gt, width):
    """the ground-truth batches of one pass are all [B, pad, 5] or all [B, pad, 6] (with the flag column): returns the width, checked against the first"""
    if gt.ndim != 3 or gt.shape[2] not in (5, 6):
        raise ValueError(f"evaluate: ground truth batches must be [B, pad, 5] or [B, pad, 6] (with the flag column), not {tuple(gt.shape)}")
    if width is not None and gt.shape[2] != width:
        raise ValueError(f"evaluate: ground truth batches of {width} and of {gt.shape[2]} columns in one pass (flags for all batches or for none)")
    return gt.shape[2]


def _chunks(generator, batch_size, num_images):
    """the validation batches regrouped into (images [n, ...], ground_truth [n, pad, 5] -- or [n, pad, 6] with the flag column) chunks of `batch_size`
    images, whatever the generator's own batch is: the chunk that reaches `num_images` is cut short, the last chunk of the pass may be partial"""
    pend_i, pend_g, have, left, width = [], [], 0, num_images, None

    def flush(k):
        nonlocal pend_i, pend_g, have
        im = np.concatenate(pend_i) if len(pend_i) > 1 else pend_i[0]
        if any(g.shape[1] != pend_g[0].shape[1] for g in pend_g):         # batches padded to different numbers of boxes: pad rows are cls -1
            pad = max(g.shape[1] for g in pend_g)
            pend_g = [np.concatenate([g, np.full((g.shape[0], pad - g.shape[1], g.shape[2]), -1, g.dtype)], 1) for g in pend_g]
        gt = np.concatenate(pend_g) if len(pend_g) > 1 else pend_g[0]
        out = im[:k], gt[:k]
        pend_i, pend_g, have = ([im[k:]], [gt[k:]], have - k) if have > k else ([], [], 0)
        return out
    for images, gt in _batches(generator):
        images, gt = _host(images), _host(gt)
        if left is not None:
            if left <= have:
                break
            images, gt = images[: left - have], gt[: left - have]
        if images.shape[0] == 0:
            continue
        width = _gt_width(gt, width)
        pend_i.append(images); pend_g.append(gt); have += images.shape[0]
        while have >= batch_size:
            if left is not None:
                left -= batch_size
            yield flush(batch_size)
    if have and (left is None or left > 0):
        yield flush(have)


def evaluate(model, generator=None, num_images=None, iou_threshold=0.5, metric='voc07', batch_size=1, max_dets=100):
    """VOC mAP of `model` (test mode) over `generator`: batches (images [B, H, W, 3] or channels_first, ground_truth [B, pad, 5]) -- the
    train_generator contract -- or an (initializer, iterator) pair.  The ground truth may be [B, pad, 6] with a flag in column 5 (0 ordinary, 1 VOC
    `difficult` / ignore, 2 crowd; voc_data.get_generator(with_difficult=True)), in every batch of the pass or in none.  batch_size 1 (default): each batch is split into single images for
    model.test_one_image.  batch_size B > 1: the batches are regrouped into chunks of B images for model.test_images (the model must have been built with
    test_batch_size >= B, or be one of the classes whose test_images is the documented loop).  Stops after `num_images` images or at the end of one pass.
    Defaults: the model's val_generator and num_val (when > 0).  metric 'coco': the COCO-style protocol (COCOEvaluator with its default thresholds and
    area ranges, `max_dets` detections per image and class; `iou_threshold` has no meaning there and must stay at its default)."""
    if metric == 'coco' and iou_threshold != 0.5:
        raise ValueError("evaluate: metric='coco' averages over its own IoU thresholds; iou_threshold must be left at its default")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"evaluate: batch_size must be >= 1, not {batch_size}")
    if generator is None:
        generator = getattr(model, 'val_generator', None)
        if generator is None:
            generator = (getattr(model, 'data_provider', None) or {}).get('val_generator')
        if generator is None:
            raise ValueError("evaluate: no generator given and the model has no val_generator")
        if num_images is None:
            nv = getattr(model, 'num_val', None)
            if nv is None:
                nv = (getattr(model, 'data_provider', None) or {}).get('num_val')
            num_images = int(nv) if nv and int(nv) > 0 else None
    if num_images is None and getattr(generator, 'endless', False):
        raise ValueError("evaluate: this generator repeats without end (voc_data.get_generator): give num_images, or num_val > 0 in the data provider")
    dev = getattr(model, 'dev', None)
    dev = dev if dev is not None and dev.type == 'cuda' else None
    if metric == 'coco':
        ev = COCOEvaluator(model.config['num_classes'], max_dets=max_dets, device=dev)
    else:
        ev = VOCEvaluator(model.config['num_classes'], iou_threshold, metric, device=dev)
    if batch_size > 1:
        for images, gt in _chunks(generator, batch_size, num_images):
            for det, g in zip(model.test_images(images), gt):
                ev.add(det, g)
        return ev.result()
    n, width = 0, None
    for images, gt in _batches(generator):
        images, gt = _host(images), _host(gt)
        if images.shape[0] and not (num_images is not None and n >= num_images):
            width = _gt_width(gt, width)
        for b in range(images.shape[0]):
            if num_images is not None and n >= num_images:
                break
            ev.add(model.test_one_image(images[b: b + 1]), gt[b])
            n += 1
        if num_images is not None and n >= num_images:
            break
    return ev.result()


class EvaluateMixin:
    """`evaluate()` for the detector classes.  A test-mode model evaluates itself.  A train-mode model builds a test-mode instance of its own
    class once (config with mode 'test', no compute_dtype -> the class's inference default, no pretraining_weight -> nothing read from disk),
    copies the current weights and moving statistics into it (export_params -> load_oracle_params; mid-warm-up the live weights are the twin's)
    before each evaluation, and evaluates that: the training state -- parameters, optimizer state, global_step, a pending warm-up, captured
    graphs -- is left as it was.  `batch_size` B > 1 evaluates B images per forward pass through `test_images`; a train-mode model keeps one test-mode
    copy per batch_size (built with test_batch_size = B) in `self._eval_models`; each copy holds its own weights and activation buffers at N = B on the
    device until the entry is deleted (`del model._eval_models[B]`), so evaluate with ONE batch size per run rather than sweeping them.

    `test_images(images)` here is the fallback form: a LOOP over `test_one_image`, NOT batched (FCOS, YOLOv2, Light-Head R-CNN).  The other seven
    classes -- SSD300, SSD512, YOLOv3, RetinaNet, CenterNet, RefineDet320, PFPNetR -- take both from heads.BatchedInference: one forward pass at
    N = test_batch_size and a batched tail, with test_one_image as its one-image case."""

    NATIVE_TEST_IMAGES = False               # True in heads.BatchedInference

    def test_images(self, images):
        """images [n, H, W, 3] (or channels_first, as test_one_image accepts it) -> list of n [scores, bbox, class_id] triples, each exactly what
        test_one_image returns for that image.  This form calls test_one_image n times: correct, uniform with the native classes, not batched."""
        images = _host(images)
        if images.ndim != 4 or images.shape[0] < 1:
            raise ValueError(f"test_images: images must be [n, H, W, 3] (or channels_first) with n >= 1, not {tuple(images.shape)}")
        return [self.test_one_image(images[b: b + 1]) for b in range(images.shape[0])]

    def evaluate(self, num_images=None, generator=None, **kw):
        if getattr(self, 'is_pretraining', False):
            raise ValueError("evaluate: a classification pre-training model has no detections (RetinaNet.evaluate measures its held-out accuracy)")
        if self.mode == 'test':
            return evaluate(self, generator, num_images, **kw)
        if generator is None:
            generator = getattr(self, 'val_generator', None)
            if generator is None:
                raise ValueError("evaluate: no generator given and the data provider has no val_generator")
            if num_images is None:
                nv = getattr(self, 'num_val', 0)
                num_images = int(nv) if nv and int(nv) > 0 else None
        B = int(kw.get('batch_size', 1))
        if B < 1:
            raise ValueError(f"evaluate: batch_size must be >= 1, not {B}")
        if not hasattr(self, '_eval_models'):
            self._eval_models = {}
        m = self._eval_models.get(B)
        if m is None:
            cfg = dict(self.config, mode='test')
            cfg.pop('compute_dtype', None)
            cfg['pretraining_weight'] = None
            cfg['device'] = self.dev
            if B > 1 and self.NATIVE_TEST_IMAGES:
                cfg['test_batch_size'] = B
            else:
                cfg.pop('test_batch_size', None)
            m = self._eval_models[B] = type(self)(cfg, self.data_provider)
            if B == 1:
                self._eval_model = m
        m.load_oracle_params(self.export_params())
        return evaluate(m, generator, num_images, **kw)
