"""PASCAL VOC mean average precision over a validation set (BASELINE.json's "mAP parity"; the reference builds a val_generator and never reads it,
testSSD300.py:56-58).

`VOCEvaluator` stages what `test_one_image` returns, image by image, on the host; `result()` packs everything into one buffer, uploads it once and runs
csrc/voc_eval.hip (odtk_voc_eval: matching, per-class rank order and AP on the device).  `evaluate(model)` drives a model over a generator with the
`train_generator` contract; every detector class has `evaluate()` through `EvaluateMixin`.  The semantics (include/odtk.h) are restated in NumPy in
tests/voc_eval_ref.py."""
from __future__ import annotations

import numpy as np
import torch

from . import ops

METRICS = ('voc07', 'area')


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


class VOCEvaluator:
    """add(detections, ground_truth) per image, result() once.  detections = [scores f32[K], bbox f32[K, 4] (y1, x1, y2, x2 px), class_id i32[K]]
    (what every class's test_one_image returns; numpy or torch, host or device), ground_truth = f32[pad, 5] rows (yc, xc, h, w, cls px; cls < 0 =
    padding).  Input errors raise ValueError; library errors OdtkError."""

    def __init__(self, num_classes, iou_threshold=0.5, metric='voc07', device=None):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
        if not 1 <= int(num_classes) <= 1024:
            raise ValueError(f"num_classes must be in [1, 1024], not {num_classes}")
        if not 0.0 <= float(iou_threshold) < 1.0:
            raise ValueError(f"iou_threshold must be in [0, 1), not {iou_threshold}")
        self.num_classes = int(num_classes)
        self.iou_threshold = float(iou_threshold)
        self.metric = metric
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        self._dets, self._gts = [], []

    @property
    def num_images(self):
        return len(self._gts)

    def add(self, detections, ground_truth):
        """stage one image: no device work, no synchronisation (device tensors are kept as they are until result())"""
        if not isinstance(detections, (list, tuple)) or len(detections) != 3:
            raise ValueError("detections must be [scores [K], bbox [K, 4], class_id [K]] as test_one_image returns them")
        s, b, c = detections
        k = tuple(s.shape)
        if len(k) != 1 or tuple(b.shape) != (k[0], 4) or tuple(c.shape) != k:
            raise ValueError(f"detections: scores {tuple(s.shape)}, bbox {tuple(b.shape)}, class_id {tuple(c.shape)} do not form [K], [K, 4], [K]")
        g = ground_truth
        if g.ndim != 2 or g.shape[1] != 5:
            raise ValueError(f"ground_truth must be [pad, 5] rows (yc, xc, h, w, cls), not {tuple(g.shape)}")
        self._dets.append((s, b, c))
        self._gts.append(g)

    def _pack(self):
        """the staged images as flat host arrays, checked (vectorised over all images: no per-image work beyond the conversions)"""
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
        bad = ~np.all(np.isfinite(gt), 1) | (gt[:, 4] != np.round(gt[:, 4]))
        if bad.any():
            raise ValueError(f"ground_truth of image {int(gi[np.argmax(bad)])}: non-finite value or non-integer class")
        bad = gt[:, 4] >= C
        if bad.any():
            raise ValueError(f"ground_truth of image {int(gi[np.argmax(bad)])}: class {int(gt[np.argmax(bad), 4])} >= num_classes {C}")
        return scores, boxes, cls.astype(np.int32), img, np.ascontiguousarray(gt), gi

    def result(self):
        """one upload, one odtk_voc_eval -> {'mAP', 'AP' f64[C] (NaN: no GT), 'npos', 'num_detections', 'tp' u8[D] in sequence order}"""
        scores, boxes, cls, img, gt, gi = self._pack()
        D, G, C = scores.shape[0], gt.shape[0], self.num_classes
        I = max(self.num_images, 1)
        # one host buffer of 4-byte words: scores | boxes | det_cls | det_img | gt_rows | gt_img
        parts = [scores.view(np.int32), boxes.reshape(-1).view(np.int32), cls, img, gt.reshape(-1).view(np.int32), gi]
        host = torch.from_numpy(np.concatenate([np.ascontiguousarray(p, np.int32).reshape(-1) for p in parts]) if D + G else np.zeros(1, np.int32))
        dev = host.to(self.device)
        offs = np.cumsum([0] + [p.size for p in parts])
        seg = [dev[offs[k]: offs[k + 1]] for k in range(len(parts))]
        ws = ops.voc_eval_workspace(D, G, I, C, self.device)
        tp = torch.empty(D, dtype=torch.uint8, device=self.device)
        npos = torch.empty(C, dtype=torch.int32, device=self.device)
        ap = torch.empty(C, dtype=torch.float64, device=self.device)
        ops.voc_eval(seg[0].view(torch.float32), seg[1].view(torch.float32).view(-1, 4), seg[2], seg[3], seg[4].view(torch.float32).view(-1, 5),
                     seg[5], I, C, self.iou_threshold, self.metric, ws, tp, npos, ap)
        ap_h = ap.cpu().numpy()
        valid = ~np.isnan(ap_h)
        return {'mAP': float(ap_h[valid].mean()) if valid.any() else float('nan'), 'AP': ap_h, 'npos': npos.cpu().numpy().astype(np.int64),
                'num_detections': np.bincount(cls, minlength=C).astype(np.int64), 'tp': tp.cpu().numpy()}


def _batches(generator):
    if isinstance(generator, tuple) and len(generator) == 2 and callable(generator[0]):
        initializer, iterator = generator
        initializer()
    else:
        iterator = generator
    return iter(iterator)


def _chunks(generator, batch_size, num_images):
    """the validation batches regrouped into (images [n, ...], ground_truth [n, pad, 5]) chunks of `batch_size` images, whatever the generator's own batch
    is: the chunk that reaches `num_images` is cut short, the last chunk of the pass may be partial"""
    pend_i, pend_g, have, left = [], [], 0, num_images

    def flush(k):
        nonlocal pend_i, pend_g, have
        im = np.concatenate(pend_i) if len(pend_i) > 1 else pend_i[0]
        if any(g.shape[1] != pend_g[0].shape[1] for g in pend_g):         # batches padded to different numbers of boxes: pad rows are cls -1
            pad = max(g.shape[1] for g in pend_g)
            pend_g = [np.concatenate([g, np.full((g.shape[0], pad - g.shape[1], 5), -1, g.dtype)], 1) for g in pend_g]
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
        pend_i.append(images); pend_g.append(gt); have += images.shape[0]
        while have >= batch_size:
            if left is not None:
                left -= batch_size
            yield flush(batch_size)
    if have and (left is None or left > 0):
        yield flush(have)


def evaluate(model, generator=None, num_images=None, iou_threshold=0.5, metric='voc07', batch_size=1):
    """VOC mAP of `model` (test mode) over `generator`: batches (images [B, H, W, 3] or channels_first, ground_truth [B, pad, 5]) -- the
    train_generator contract -- or an (initializer, iterator) pair.  batch_size 1 (default): each batch is split into single images for
    model.test_one_image.  batch_size B > 1: the batches are regrouped into chunks of B images for model.test_images (the model must have been built with
    test_batch_size >= B, or be one of the classes whose test_images is the documented loop).  Stops after `num_images` images or at the end of one pass.
    Defaults: the model's val_generator and num_val (when > 0)."""
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
    ev = VOCEvaluator(model.config['num_classes'], iou_threshold, metric, device=dev if dev is not None and dev.type == 'cuda' else None)
    if batch_size > 1:
        for images, gt in _chunks(generator, batch_size, num_images):
            for det, g in zip(model.test_images(images), gt):
                ev.add(det, g)
        return ev.result()
    n = 0
    for images, gt in _batches(generator):
        images, gt = _host(images), _host(gt)
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

    `test_images(images)` here is the fallback form: a LOOP over `test_one_image`, NOT batched (FCOS, YOLOv2, Light-Head R-CNN).  Seven classes override
    it with one forward pass at N = test_batch_size and a batched tail: SSD300, SSD512, YOLOv3, RetinaNet, RefineDet320 and PFPNetR (heads.BatchedTail)
    and CenterNet (heads.CenterNetBatched)."""

    NATIVE_TEST_IMAGES = False               # True in the classes whose test_images is one batched forward + tail

    def test_images(self, images):
        """images [n, H, W, 3] (or channels_first, as test_one_image accepts it) -> list of n [scores, bbox, class_id] triples, each exactly what
        test_one_image returns for that image.  This form calls test_one_image n times: correct, uniform with the native classes, not batched."""
        images = _host(images)
        if images.ndim != 4 or images.shape[0] < 1:
            raise ValueError(f"test_images: images must be [n, H, W, 3] (or channels_first) with n >= 1, not {tuple(images.shape)}")
        return [self.test_one_image(images[b: b + 1]) for b in range(images.shape[0])]

    def _stage_test_images(self, images):
        """native classes: the n <= test_batch_size images into the first n slots of self.images (the tail slots keep what they held: computed, discarded)"""
        images = torch.as_tensor(np.asarray(images), dtype=torch.float32)
        if images.ndim == 4 and self.data_format == 'channels_first' and images.shape[1] == 3:
            images = images.permute(0, 2, 3, 1)
        if self.mode != 'test':
            raise ValueError("test_images: the model was not built in test mode")
        if images.ndim != 4 or not 1 <= images.shape[0] <= self.batch_size or tuple(images.shape[1:]) != tuple(self.images.shape[1:]):
            raise ValueError(f"test_images: images must be [n, {', '.join(str(d) for d in self.images.shape[1:])}] with 1 <= n <= test_batch_size = "
                             f"{self.batch_size}, not {tuple(images.shape)}")
        n = images.shape[0]
        self.images[:n].copy_(images)
        return n

    @staticmethod
    def _test_batch_size(config):
        """config['test_batch_size']: optional, an integer >= 1 (default 1), read in test mode only: the number of image slots of the test-mode buffers"""
        b = config.get('test_batch_size', 1)
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 1:
            raise ValueError(f"test_batch_size must be an integer >= 1, not {b!r}")
        return int(b)

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
