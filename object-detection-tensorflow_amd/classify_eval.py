"""Held-out accuracy of the classification pre-training graph (the reference reports the training batch's own accuracy only, RetinaNet.py:128-130).

`ClassificationEvaluator` keeps every accumulator on the device: `update(logits, labels)` is one odtk_classify_eval (csrc/classify.hip: per-row rank and
cross-entropy, then top-1 / top-k hits, the f64 loss sum and per-class counts added into the accumulators) and does not synchronise; `result()` reads all
of it back at once through a pinned buffer.  `RetinaNet.evaluate()` in pre-training mode drives it over a validation generator.  The semantics
(include/odtk.h, "Classification metrics") are restated in NumPy float64 in tests/classify_cases.py."""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class ClassificationEvaluator:
    """reset() / update(logits f32 [N, C] device rows, labels int [N] device) per batch / result() once.  Layout of the accumulator, 4-byte words:
    totals i64[4] | loss_sum f64 | class_seen i32[C] | class_hit i32[C]."""

    def __init__(self, num_classes, top_k=5, device=None):
        C = int(num_classes)
        if not 1 <= C <= 1024:
            raise ValueError(f"num_classes must be in [1, 1024], not {num_classes}")
        if not 1 <= int(top_k) <= C:
            raise ValueError(f"top_k must be in [1, num_classes = {C}], not {top_k}")
        self.num_classes, self.top_k = C, int(top_k)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        dev = self.device = torch.device(device)
        self.words = torch.zeros(10 + 2 * C, dtype=torch.int32, device=dev)
        self.totals = self.words[:8].view(torch.int64)
        self.loss_sum = self.words[8:10].view(torch.float64)
        self.class_seen = self.words[10: 10 + C]
        self.class_hit = self.words[10 + C:]
        self.host = torch.zeros(self.words.shape, dtype=torch.int32, pin_memory=True) if dev.type == 'cuda' else None
        self.rank = self.loss = None

    def reset(self):
        """clears the accumulators on the current stream (no synchronisation)"""
        self.words.zero_()

    def update(self, logits, labels):
        """one batch: logits f32 [N, C] (rows may be pitched: stride(1) == 1, stride(0) >= C), labels integer [N], both on the evaluator's device.
        Afterwards self.rank / self.loss hold the batch's per-row results.  No host work beyond the launch, no synchronisation."""
        C = self.num_classes
        if not (isinstance(logits, torch.Tensor) and isinstance(labels, torch.Tensor)) or logits.device != self.words.device \
                or labels.device != self.words.device:
            raise ValueError(f"update: logits and labels must be tensors on {self.words.device}")
        if logits.dtype != torch.float32 or logits.ndim != 2 or logits.shape[1] != C or logits.shape[0] < 1 or (C > 1 and logits.stride(1) != 1) \
                or logits.stride(0) < C:
            raise ValueError(f"update: logits must be f32 [N, {C}] rows with N >= 1, not {logits.dtype} {tuple(logits.shape)} strides {logits.stride()}")
        N = logits.shape[0]
        if labels.dtype not in (torch.int32, torch.int64) or tuple(labels.shape) != (N,):
            raise ValueError(f"update: labels must be int32 / int64 [{N}], not {labels.dtype} {tuple(labels.shape)}")
        if labels.dtype != torch.int32 or not labels.is_contiguous():
            labels = labels.to(torch.int32).contiguous()
        if self.rank is None or self.rank.shape[0] != N:
            self.rank = torch.zeros(N, dtype=torch.int32, device=self.words.device)
            self.loss = torch.zeros(N, device=self.words.device)
        ops.classify_eval(logits, logits.stride(0), N, C, labels, self.top_k, self.rank, self.loss, self.totals, self.loss_sum, self.class_seen,
                          self.class_hit)

    def result(self):
        """the one read-back -> {'num_images', 'top1', 'topk', 'top_k', 'loss' (mean), 'class_seen' i64[C], 'class_accuracy' f64[C] (NaN where the class was
        not seen), 'invalid_labels'}; rows with a label outside [0, C) are counted in 'invalid_labels' only"""
        if self.host is not None:
            self.host.copy_(self.words, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            h = self.host.numpy().copy()
        else:
            h = self.words.numpy().copy()
        C = self.num_classes
        tot = h[:8].view(np.int64)
        n = int(tot[0])
        seen = h[10: 10 + C].astype(np.int64)
        hit = h[10 + C:].astype(np.int64)
        acc = np.full(C, np.nan)
        np.divide(hit, seen, out=acc, where=seen > 0)
        nan = float('nan')
        return {'num_images': n, 'top1': int(tot[1]) / n if n else nan, 'topk': int(tot[2]) / n if n else nan, 'top_k': self.top_k,
                'loss': float(h[8:10].view(np.float64)[0]) / n if n else nan, 'class_seen': seen, 'class_accuracy': acc, 'invalid_labels': int(tot[3])}
