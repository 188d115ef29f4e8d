"""Inference tails of the other detector classes of the reference on libodtk: decode kernel -> per-class score threshold ->
per-class NMS (the SSD300 NMS path) -> [scores f32[K], bbox f32[K,4] y1x1y2x2 px, class_id i32[K]], i.e. what each class
stores in `self.detection_pred` (RetinaNet.py:224-256, YOLOv3.py:320-368, FCOS.py:197-265, CenterNet.py:159-185, RefineDet.py:189-230);
for RefineDet also the training-side chain matching -> ARM hard-negative mining -> two-stage loss (`refinedet_loss`).
ONE inference path for SSD300, SSD512, YOLOv3, RetinaNet, CenterNet, RefineDet320 and PFPNetR: `BatchedInference` (test_images: one forward pass at
N = test_batch_size, the class's decode, `BatchedTail` -- CenterNet: `CenterNetBatched` -- and one read-back; test_one_image is that path with one image).
FCOS, YOLOv2 and Light-Head R-CNN keep a single-image test_one_image on `_per_class_nms` (fcos_detect, yolov2_detect, lhrcnn.py) and the loop of
voc_eval.EvaluateMixin as test_images.  Product path: no CPU fallback, no use of the test oracles."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .voc_eval import EvaluateMixin

NMS_MAX_CANDIDATES = 32768          # odtk_nms_batched: boxes per problem


def _per_class_nms(conf, boxes, cand, num_classes, max_boxes, iou_thr, method='hard', sigma=0.5, min_score=0.0):
    """conf [L, ld] scores (classes 0..num_classes-1 in the first columns), boxes [L, 4], cand [L, ld] uint8.  method 'hard': greedy NMS (odtk_nms_batched);
    'linear' / 'gaussian': soft-NMS (odtk_soft_nms_image_class at one image), the scores returned are the decayed ones."""
    dev = conf.device
    L, ld = conf.shape
    rows = None
    if L > NMS_MAX_CANDIDATES:
        # keep the rows that are a candidate for at least one class, in order (ties in NMS follow the row order)
        rows = torch.nonzero(cand[:, :num_classes].any(dim=1)).flatten()
        if rows.numel() > NMS_MAX_CANDIDATES:
            raise ValueError(f'{rows.numel()} candidate boxes exceed the NMS capacity of {NMS_MAX_CANDIDATES}; raise the score threshold')
        if rows.numel() == 0:
            return (torch.empty(0, device=dev), torch.empty(0, 4, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
        conf, boxes, cand = conf[rows].contiguous(), boxes[rows].contiguous(), cand[rows].contiguous()
        L = rows.numel()
    cap = max(int(max_boxes), 1)
    out_idx = torch.zeros(num_classes, cap, dtype=torch.int32, device=dev)
    out_cnt = torch.zeros(num_classes, dtype=torch.int32, device=dev)
    soft = method != 'hard'
    if soft:
        out_score = torch.zeros(num_classes, cap, device=dev)
        ops.soft_nms_image_class(boxes, 0, conf, 0, 1, ld, cand, 0, 1, ld, 1, L, None, 1, num_classes, int(max_boxes), ops.NMS_METHODS[method], float(iou_thr),
                                 float(sigma), float(min_score), out_idx, out_score, cap, out_cnt)
    else:
        ops.nms_batched(boxes, 0, conf, 1, ld, cand, 1, ld, 1, L, num_classes, None, 0, int(max_boxes), float(iou_thr), out_idx, cap, out_cnt)
    cnt = out_cnt.cpu().tolist()
    scores, bbox, cid = [], [], []
    for c in range(num_classes):                      # ascending class id, NMS pick order inside (the reference's concat order)
        ids = out_idx[c, : cnt[c]].long()
        scores.append(out_score[c, : cnt[c]] if soft else conf[ids, c]); bbox.append(boxes[ids])
        cid.append(torch.full((cnt[c],), c, dtype=torch.int32, device=dev))
    return torch.cat(scores), torch.cat(bbox, 0).reshape(-1, 4), torch.cat(cid)


class BatchedTail:
    """The inference tail behind the decode for N images at once: [order-preserving row compaction when a head has more rows than the NMS takes per problem]
    -> NMS of N * num_classes problems in one launch chain (odtk_nms_image_class) -> detection pack (odtk_detection_pack) -> ONE read-back per batch (the
    per-image counts, their scan and the packed rows, through a pinned host buffer).  Per image the result is what `_per_class_nms` returns for that image
    alone, bit for bit: the same NMS kernels on the same operands, the same order (ascending class id, NMS pick order inside).  Buffers are allocated once
    per (N, A, num_classes, max_boxes).  conf [N, A, ld] scores (classes in the first num_classes columns), boxes [N, A, 4], cand [N, A, ld] uint8.
    The tail also holds what a class's decode writes for it: self.conf [N, A, nc], self.boxes [N, A, 4], self.keep u8 [N, A], self.cand u8 [N, A, nc];
    bool_cand (YOLOv3: the threshold is one torch.ge): cand is a bool tensor and there is no keep.  `launch_own` runs the tail on them.
    method 'hard' (default): exactly the launches above.  'linear' / 'gaussian' (with `sigma`, `min_score`): odtk_soft_nms_image_class and
    odtk_detection_pack_scored in their place -- same picks table, plus out_score [N, nc, cap], the decayed scores the pack hands on."""

    def __init__(self, N, A, num_classes, max_boxes, device, bool_cand=False, method='hard', sigma=0.5, min_score=0.0):
        self.N, self.A, self.nc, self.max_boxes = int(N), int(A), int(num_classes), int(max_boxes)
        self.method, self.sigma, self.min_score = ops.NMS_METHODS[method], float(sigma), float(min_score)
        dev = self.dev = torch.device(device)
        N, A, nc = self.N, self.A, self.nc
        self.conf = torch.zeros(N, A, nc, device=dev)
        self.boxes = torch.zeros(N, A, 4, device=dev)
        self.cand = torch.zeros(N, A, nc, dtype=torch.bool if bool_cand else torch.uint8, device=dev)
        if not bool_cand:
            self.keep = torch.zeros(N, A, dtype=torch.uint8, device=dev)
        cap = self.cap = max(self.max_boxes, 1)
        i32 = dict(dtype=torch.int32, device=dev)
        self.compact = self.A > NMS_MAX_CANDIDATES
        if self.compact:
            R = self.R = NMS_MAX_CANDIDATES
            self.rows = torch.zeros(N, R, **i32)
            self.c_conf = torch.zeros(N, R, nc, device=dev)
            self.c_boxes = torch.zeros(N, R, 4, device=dev)
            self.c_cand = torch.zeros(N, R, nc, dtype=torch.uint8, device=dev)
        self.out_idx = torch.zeros(N, nc, cap, **i32)
        self.out_cnt = torch.zeros(N, nc, **i32)
        self.out_score = torch.zeros(N, nc, cap, device=dev) if self.method else None
        # what travels back, one buffer of 4-byte words: counts [N] | offsets [N + 1] | compaction counts [N] | scores [K] | bbox [K, 4] | class_id [K]
        K = self.K = N * nc * cap
        self.words = torch.zeros(3 * N + 1 + 6 * K, **i32)
        o = 0
        self.counts = self.words[o: o + N]; o += N
        self.offsets = self.words[o: o + N + 1]; o += N + 1
        self.row_cnt = self.words[o: o + N]; o += N
        self._o_scores, self._o_bbox, self._o_cid = o, o + K, o + 5 * K
        self.scores = self.words[o: o + K].view(torch.float32); o += K
        self.bbox = self.words[o: o + 4 * K].view(torch.float32).view(K, 4); o += 4 * K
        self.class_id = self.words[o: o + K]
        self.host = torch.zeros(self.words.shape, dtype=torch.int32, pin_memory=True) if dev.type == 'cuda' else None

    def launch(self, conf, boxes, cand, iou_thr):
        """the device side (no synchronisation): after it self.words holds the batch's detections"""
        N, A, nc = self.N, self.A, self.nc
        assert tuple(conf.shape[:2]) == (N, A) and tuple(boxes.shape) == (N, A, 4) and tuple(cand.shape) == tuple(conf.shape)
        ld = conf.shape[2]
        if self.compact:
            R = self.R
            ops.compact_rows(cand, nc, R, self.rows, self.row_cnt)
            ops.gather_rows(self.rows, self.row_cnt, nc, conf, boxes, cand, self.c_conf, self.c_boxes, self.c_cand)
            conf, boxes = self.c_conf, self.c_boxes
            operands = (boxes, R * 4, conf, R * nc, 1, nc, self.c_cand, R * nc, 1, nc, 1, R, self.row_cnt, N, nc, self.max_boxes)
        else:
            operands = (boxes, A * 4, conf, A * ld, 1, ld, cand, A * ld, 1, ld, 1, A, None, N, nc, self.max_boxes)
        if self.method:
            ops.soft_nms_image_class(*operands, self.method, iou_thr, self.sigma, self.min_score, self.out_idx, self.out_score, self.cap, self.out_cnt)
            ops.detection_pack_scored(self.out_idx, self.out_cnt, self.out_score, conf, boxes, self.counts, self.offsets, self.scores, self.bbox,
                                      self.class_id)
        else:
            ops.nms_image_class(*operands, iou_thr, self.out_idx, self.cap, self.out_cnt)
            ops.detection_pack(self.out_idx, self.out_cnt, conf, boxes, self.counts, self.offsets, self.scores, self.bbox, self.class_id)

    def launch_own(self, iou_thr):
        """launch() on the decode outputs the tail holds itself"""
        self.launch(self.conf, self.boxes, self.cand.view(torch.uint8), iou_thr)

    def read(self, n_images=None):
        """the one read-back: list of [scores f32[K], bbox f32[K, 4], class_id i32[K]] (numpy) of the first n_images images"""
        n_images = self.N if n_images is None else int(n_images)
        if self.host is not None:
            self.host.copy_(self.words, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            h = self.host.numpy()
        else:
            h = self.words.numpy()
        N, K = self.N, self.K
        off = h[N: 2 * N + 1]
        if self.compact:
            for n in range(n_images):
                if h[2 * N + 1 + n] > NMS_MAX_CANDIDATES:
                    raise ValueError(f'image {n}: {int(h[2 * N + 1 + n])} candidate boxes exceed the NMS capacity of {NMS_MAX_CANDIDATES}; raise the score threshold')
        sc = h[self._o_scores: self._o_scores + K].view('float32')
        bb = h[self._o_bbox: self._o_bbox + 4 * K].view('float32').reshape(K, 4)
        ci = h[self._o_cid: self._o_cid + K]
        return [[sc[off[n]: off[n + 1]].copy(), bb[off[n]: off[n + 1]].copy(), ci[off[n]: off[n + 1]].copy()] for n in range(n_images)]

    def __call__(self, conf, boxes, cand, iou_thr, n_images=None):
        self.launch(conf, boxes, cand, iou_thr)
        return self.read(n_images)


class CenterNetBatched:
    """CenterNet's tail for N images at once: odtk_centernet_decode_batched (sigmoid / arg-max over all pixels, then one workgroup per image for the 3x3 peak
    test, the threshold and the top-k) -> ONE read-back per batch through a pinned host buffer.  Per image the result is what odtk_centernet_decode gives for
    that image alone, bit for bit.  One buffer of 4-byte words travels back: counts [N] | scores [N, top_k] | bbox [N, top_k, 4] | class_id [N, top_k]; rows
    behind an image's count are never read."""

    def __init__(self, N, H, W, top_k, device):
        self.N, self.H, self.W, self.K = int(N), int(H), int(W), int(top_k)
        dev = self.dev = torch.device(device)
        N, K = self.N, self.K
        self.words = torch.zeros(N + 6 * N * K, dtype=torch.int32, device=dev)
        self._o_scores, self._o_bbox, self._o_cid = N, N + N * K, N + 5 * N * K
        self.counts = self.words[:N]
        self.scores = self.words[self._o_scores: self._o_bbox].view(torch.float32).view(N, K)
        self.bbox = self.words[self._o_bbox: self._o_cid].view(torch.float32).view(N, K, 4)
        self.class_id = self.words[self._o_cid:].view(N, K)
        self.host = torch.zeros(self.words.shape, dtype=torch.int32, pin_memory=True) if dev.type == 'cuda' else None
        self.ws = None                                  # N score planes + N class planes, allocated with the first launch

    def launch(self, keypoints, offset, size, score_thr, stride=4.0):
        """the device side (no synchronisation): after it self.words holds the batch's detections"""
        assert tuple(keypoints.shape[:3]) == (self.N, self.H, self.W) and tuple(offset.shape) == tuple(size.shape) == (self.N, self.H, self.W, 2)
        if self.ws is None:
            self.ws = ops.centernet_decode_workspace(self.N, self.H, self.W, self.dev)
        ops.centernet_decode_batched(keypoints, offset, size, stride, score_thr, self.K, self.scores, self.bbox, self.class_id, self.counts, self.ws)

    def read(self, n_images=None):
        """the one read-back: list of [scores f32[k], bbox f32[k, 4], class_id i32[k]] (numpy) of the first n_images images, k = that image's count"""
        n_images = self.N if n_images is None else int(n_images)
        if self.host is not None:
            self.host.copy_(self.words, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            h = self.host.numpy()
        else:
            h = self.words.numpy()
        N, K = self.N, self.K
        sc = h[self._o_scores: self._o_bbox].view('float32').reshape(N, K)
        bb = h[self._o_bbox: self._o_cid].view('float32').reshape(N, K, 4)
        ci = h[self._o_cid:].reshape(N, K)
        return [[sc[n, :h[n]].copy(), bb[n, :h[n]].copy(), ci[n, :h[n]].copy()] for n in range(n_images)]

    def __call__(self, keypoints, offset, size, score_thr, stride=4.0, n_images=None):
        self.launch(keypoints, offset, size, score_thr, stride)
        return self.read(n_images)


class BatchedInference(EvaluateMixin):
    """The inference surface of the classes with a batched tail -- SSD300, SSD512, YOLOv3, RetinaNet, CenterNet, RefineDet320, PFPNetR: test_images is
    stage -> ONE forward pass at N = test_batch_size -> the class's decode into its tail (BatchedTail / CenterNetBatched, built with the first call) -> one
    read-back, and test_one_image is test_images of one image.  A class supplies three hooks:
      _forward_test()    the test-mode forward pass with the reference's feed quirk;
      _make_tail()       the tail for self.batch_size image slots;
      _launch_tail(t)    the decode launch(es) and t's own launch, no synchronisation."""

    NATIVE_TEST_IMAGES = True
    _tail_batched = None

    @staticmethod
    def _test_batch_size(config):
        """config['test_batch_size']: optional, an integer >= 1 (default 1), read in test mode only: the number of image slots of the test-mode buffers"""
        b = config.get('test_batch_size', 1)
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 1:
            raise ValueError(f"test_batch_size must be an integer >= 1, not {b!r}")
        return int(b)

    def _stage_test_images(self, images):
        """the n <= test_batch_size images into the first n slots of self.images (the tail slots keep what they held: computed, discarded)"""
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

    def test_images(self, images):
        """images [n, H, W, 3] (or channels_first), n <= test_batch_size -> n [scores f32[K], bbox f32[K, 4], class_id i32[K]] triples (numpy)"""
        n = self._stage_test_images(images)
        self._forward_test()
        t = self._tail_batched
        if t is None:
            t = self._tail_batched = self._make_tail()
        if getattr(t, 'method', 0):
            t.min_score = float(self.soft_nms_min_score)            # (its default follows nms_score_threshold, which may be set between calls)
        self._launch_tail(t)
        return t.read(n)

    def test_one_image(self, images):
        """one image [1, H, W, 3] (or channels_first) -> [scores, bbox, class_id]: test_images with one image (a model built without test_batch_size
        has one image slot and refuses any other count)"""
        return self.test_images(images)[0]


def refinedet_anchors(input_size, device):
    """RefineDet.py:140-143, :399-420: levels conv4_3 / conv5_3 / conv8_2 / conv10_2, strides 8 / 16 / 32 / 64, size = 4 * stride, ratios 0.5 / 1 / 2.
    Returns (y1x1, y2x2, yx, hw, nmsbox) device tensors.  The SSD300 prior kernel is reused: (i + 0.5) * input / side equals (i + 0.5) * stride bit for
    bit here (input / side = stride exactly, every product exact in float32)."""
    s = input_size
    sides = []
    for _ in range(3):
        s = -(-s // 2)
    sides.append(s)
    for _ in range(3):
        s = -(-s // 2)
        sides.append(s)
    flat = []
    for side, stride in zip(sides, (8, 16, 32, 64)):
        assert side * stride == input_size, "RefineDet: the input size must be a multiple of 64"
        size = 4 * stride
        for r in (0.5, 1.0, 2.0):
            flat += [size * (r ** 0.5), size / (r ** 0.5)]
    return ops.ssd_priors(input_size, sides, [3, 3, 3, 3], flat, device)


class RefineDetLoss:
    """RefineDet.py:422-567 for a batch: odtk_retina_match -> odtk_softmax_ce_const (ARM background cross entropy) -> odtk_nms_batched (hard negatives)
    -> odtk_refinedet_loss.  Buffers are allocated once per (N, A, C, P)."""

    def __init__(self, anchors, N, num_classes, P, device):
        self.anc, self.N, self.C, self.P = anchors, N, num_classes, P
        A = anchors[0].shape[0]
        self.A = A
        i32 = dict(dtype=torch.int32, device=device)
        self.ngt = torch.zeros(N, **i32); self.best = torch.zeros(N, P, **i32)
        self.status = torch.zeros(N, A, dtype=torch.uint8, device=device); self.rg = torch.zeros(N, A, **i32)
        self.counts = torch.zeros(N, 4, **i32)
        self.ws = ops.retina_match_workspace(A, N, P, device)
        self.negloss = torch.zeros(N, A, device=device)
        self.sel_idx = torch.zeros(N, A, **i32); self.sel_cnt = torch.zeros(N, **i32)
        self.loss_parts = torch.zeros(N, 8, device=device)
        self.d_arm_loc = torch.zeros(N, A, 4, device=device); self.d_arm_conf = torch.zeros(N, A, 2, device=device)
        self.d_odm_loc = torch.zeros(N, A, 4, device=device); self.d_odm_conf = torch.zeros(N, A, num_classes, device=device)

    def __call__(self, arm_loc, arm_conf, odm_loc, odm_conf, gt, grad_scale):
        """-> loss_parts [N, 8] (column 6 = the per-image loss); the gradients are in self.d_*"""
        y1x1, y2x2, yx, hw, nmsbox = self.anc
        N, A = self.N, self.A
        ops.retina_match(y1x1, y2x2, hw, gt, self.ngt, self.best, self.status, self.rg, self.counts, self.ws)
        ops.softmax_ce_const(arm_conf, N * A, 2, 2, 1, self.negloss)
        ops.nms_batched(nmsbox, 0, self.negloss, A, 1, self.status, A, 1, 2, A, N, self.counts[:, 2:], 4, 0, 0.7, self.sel_idx, A, self.sel_cnt)
        ops.refinedet_loss(arm_loc, arm_conf, odm_loc, odm_conf, yx, hw, gt, self.ngt, self.best, self.status, self.rg, self.counts, self.negloss,
                           self.sel_idx, self.sel_cnt, grad_scale, self.loss_parts, self.d_arm_loc, self.d_arm_conf, self.d_odm_loc, self.d_odm_conf)
        return self.loss_parts


def fcos_detect(conf, reg, center, score_thr, max_boxes, iou_thr, **nms):
    """FCOS.py:197-265.  conf / reg / center: the five level tensors [H, W, C | 4 | 1] of one image; classes 0..C-2.  nms: method / sigma / min_score of
    `_per_class_nms`."""
    pconf, pbbox = ops.fcos_decode_candidates(conf, reg, center)
    cand = (pconf >= score_thr).to(torch.uint8)
    return _per_class_nms(pconf, pbbox, cand, pconf.shape[1] - 1, max_boxes, iou_thr, **nms)


def yolov2_detect(pred0, priors_flat, score_thr, max_boxes, iou_thr, stride=32.0, **nms):
    """YOLOv2.py:177-201.  pred0: [H, W, P, C + 5] of one image.  nms: method / sigma / min_score of `_per_class_nms`."""
    conf, bbox = ops.yolov2_decode_candidates(pred0, priors_flat, stride)
    cand = (conf >= score_thr).to(torch.uint8)
    return _per_class_nms(conf, bbox, cand, conf.shape[1], max_boxes, iou_thr, **nms)


class YOLOv2Loss:
    """YOLOv2.py:102-167 for a batch (odtk_yolov2_loss); the gradient of the prediction tensor is in self.d_pred"""

    def __init__(self, N, H, W, P, C, priors_flat, scales, device):
        self.priors_flat, self.scales = priors_flat, scales
        self.loss_parts = torch.zeros(N, 5, device=device)
        self.d_pred = torch.zeros(N, H * W * P, C + 5, device=device)
        self.shape = (N, H, W, P, C + 5)

    def __call__(self, pred, gt, grad_scale, stride=32.0):
        ops.yolov2_loss(pred.view(self.shape), self.priors_flat, stride, gt, self.scales, grad_scale, self.loss_parts, self.d_pred)
        return self.loss_parts

