"""RetinaNet (the reference's pre-activation ResNet + pyramid + ten subnets) behind the reference's class surface, on libodtk.

Reference: /root/reference/RetinaNet.py -- the DETECTION graph (`is_pretraining: False`, testretinanet.py:22-41)
  * constructor, config keys ............. :12-77    (filters_list = [7 * 2^i] is built from the stem's KERNEL SIZE, :27 -- reproduced)
  * input ................................ :101-118  (images - mean; test mode feeds the tensor after the subtraction)
  * backbone ............................. :258-285, :634-643: 7x7 / s2 conv + batch norm + ReLU, 3x3 / s2 max pool, bottleneck units
                                           [BN-ReLU-1x1 f, BN-ReLU-3x3 f (stride), BN-ReLU-1x1 4f] + [BN-ReLU-3x3 4f (stride)] shortcut
  * pyramid, subnets ..................... :138-155, :287-319 (bilinear top-down path, the SUM is handed down; subnets not shared)
  * loss, optimizer ...................... :172-217  (odtk_retina_match / odtk_retina_loss; Momentum 0.9; L2 over all variables)
  * inference ............................ :218-256  (heads.BatchedInference)
  * train / test / checkpoints ........... :488-535
The classification pre-training graph (`is_pretraining: True`, :61-99, :120-135, :476-531, :548-551) is built behind the same class:
  * the backbone alone (l0 .. l64), the LAST unit's sum (no batch norm / ReLU after it) -> global average pool -> softmax cross-entropy
    (odtk_gap_softmax_ce_fwd / _bwd): 4 * FILTERS[-1] = 224 logits, no dense layer, config['num_classes'] plays no part; labels int [N] in [0, 224)
  * train_one_epoch -> (mean loss, mean accuracy); test_one_image -> pred int64 [1]; test_images -> pred int64 [n]; save_weight -> the 260
    trainables of 'feature_extractor'; evaluate -> held-out top-1 / top-k / loss with BATCH statistics (_evaluate_pretraining, classify_eval.py)
  * the moving statistics are NEVER updated (the pre-training train_op has no UPDATE_OPS dependency, :134): they stay 0 / 1, test mode uses them
Same conventions as yolov3.py: layers l0 .. l121 in creation order (layer k = conv k + batch norm k; l0 is conv -> BN -> ReLU, every
other layer BN -> ReLU -> conv with a LIVE bias gradient), one flat f32 parameter buffer, NHWC rows with zero-filled pad columns for
the 7 / 14 / 28-channel maps.  A batch norm whose input feeds several consumers accumulates its dx through a scratch + odtk_add2d.
"""
from __future__ import annotations

import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

from . import graph, heads, ops
from .base import DetectorBase, _Act

MEAN_RGB = (123.68, 116.779, 103.979)
FILTERS = (7, 14, 28, 56)                                     # RetinaNet.py:27 (sic)
ANCHOR_SIZES = (32, 64, 128, 256, 512)                        # :39
ASPECT_RATIOS = (1, 1 / 2, 2)                                 # :40
ANCHOR_SCALES = (2 ** 0, 2 ** (1 / 3), 2 ** (2 / 3))          # :41
PI = 0.01                                                     # :48


def layer_specs(block_list, init_filters, num_classes, num_anchors=9):
    """[(name, cin, cout, k, stride, bn_channels, bias_init)] in creation order (RetinaNet.py:258-301, :634-643)"""
    specs = []

    def add(cin, cout, k, s, bias_init=0.):
        specs.append((f'l{len(specs)}', cin, cout, k, s, cin if specs else cout, bias_init))
        return cout
    c = add(3, init_filters, 7, 2)
    stage_out = []
    for i, blocks in enumerate(block_list):
        f = FILTERS[i]
        for j in range(blocks):
            s = 2 if (i > 0 and j == 0) else 1
            add(c, f, 1, 1); add(f, f, 3, s); add(f, 4 * f, 1, 1)
            add(c, 4 * f, 3, s)
            c = 4 * f
        stage_out.append(c)
    f1, f2, f3 = stage_out[-3:]
    add(f3, 256, 3, 1)
    add(f2, 256, 1, 1); add(256, 256, 3, 1)
    add(f1, 256, 1, 1); add(256, 256, 3, 1)
    add(256, 256, 3, 2); add(256, 256, 3, 2)
    for _ in range(5):
        for _ in range(4):
            add(256, 256, 3, 1)
        add(256, num_classes * num_anchors, 3, 1, -math.log((1 - PI) / PI))
        for _ in range(4):
            add(256, 256, 3, 1)
        add(256, 4 * num_anchors, 3, 1)
    return specs


def level_priors(size):
    """(h, w) of the 9 anchors of one level, python doubles in the reference's loop order (RetinaNet.py:332-338)"""
    out = []
    for ratio in ASPECT_RATIOS:
        for scale in ANCHOR_SCALES:
            out.append((size * scale * (ratio ** 0.5), size * scale / (ratio ** 0.5)))
    return out


class RetinaNet(heads.BatchedInference, graph.SharedGradients, DetectorBase):
    def __init__(self, config, data_provider):
        assert len(config['data_shape']) == 3
        self.is_pretraining = bool(config.get('is_pretraining'))
        assert config['is_bottleneck'], 'only the bottleneck units of testretinanet.py are built'
        self._prologue(config, data_provider, native_test_batch=True)
        self.block_list = list(config['residual_block_list'])
        self.data_shape = config['data_shape']
        if not self.is_pretraining:                 # (the pre-training head has its own 224 logits: config['num_classes'] plays no part)
            ops.check_num_classes('RetinaNet', config['num_classes'], background=True)
        self.num_classes = config['num_classes'] + 1
        self.gamma, self.alpha = config['gamma'], config['alpha']
        self.num_anchors = len(ASPECT_RATIOS) * len(ANCHOR_SCALES)
        # f32 by default: the reference's identity-free residual units amplify bf16's rounding of the stored activations to O(1) by the
        # end of the backbone at random initialisation; 'bf16' runs (3.4x faster) but is not validated for training
        # 'f32x3' (round 4): the f32 engine -- every tensor stays f32 -- whose convolution DESCRIPTORS say ODTK_F32X3: the library runs a layer's three passes as
        # three bf16 MFMA products per f32 product (operand splitting, 2^-17 per product instead of bf16's 2^-9) where that is faster than the exact f32 MFMA
        # kernel, i.e. on the 256-channel pyramid and heads, and exactly on the narrow backbone layers (include/odtk.h).  Default for training: it clears the gate of
        # tests/test_gpu_bf16_gate.py at RANDOM INITIALISATION (every filter gradient within cosine 0.997 of the f32 engine's, 1.000 after 300 steps) at 1.9x the
        # f32 engine's throughput; mode 'test' keeps the exact 'f32'.
        engine = config.get('compute_dtype') or ('f32x3' if config['mode'] == 'train' else 'f32')
        self.x3 = engine == 'f32x3'
        self._set_engine(engine)
        self.specs = layer_specs(self.block_list, config['init_conv_filters'], self.num_classes, self.num_anchors)
        if self.is_pretraining:                     # the backbone alone: stem + units (RetinaNet.py:120-122)
            self.specs = self.specs[: 1 + 4 * sum(self.block_list)]
        self._init_parameters(int(config.get('seed', 0)))
        self._build()
        if self.is_pretraining:                     # the reference swaps its class surface the same way (:61-68)
            self.save_weight = self._save_pretraining_weight
            self.load_weight = self._load_pretraining_model_weight
            self.train_one_epoch = self._train_pretraining_epoch
            self.test_one_image = self._test_one_pretraining_image

    # ------------------------------------------------------------------ parameters
    def _rows(self, specs):
        return [graph.Row(name, (cout, k, k, cin), cout, bnc, True, cin * k * k, bias_init) for name, cin, cout, k, _, bnc, bias_init in specs]

    def _init_parameters(self, seed):
        graph.init_parameters(self, self._rows(self.specs), seed)

    # ------------------------------------------------------------------ the graph
    def _build(self):
        N, dev, dt, ch = self.batch_size, self.dev, self.tdt, self.chunk
        H, W, _ = self.data_shape
        self.images = torch.zeros(N, H, W, 3, device=dev)
        c0 = ops.pad_to(3, ch)
        self.input = _Act('input', N, H, W, 3, c0, dt, dev)
        self.plan, self.desc, self.bnsave, self.acts = [], {}, {}, {}
        it = iter(self.specs)
        self._max_ws = self._max_scr = 0
        self._groups = {}

        def note(a):
            self._max_ws = max(self._max_ws, ops.bn_workspace_bytes(a.M, a.C))
            self._max_scr = max(self._max_scr, a.M * a.ld)

        def bnsave(name, a, bnc):
            self.bnsave[name] = (torch.zeros(bnc, device=dev), torch.zeros(bnc, device=dev))
            note(a)

        def bnconv(x):
            """batch norm -> ReLU -> conv(bias): returns the conv output"""
            name, cin, cout, k, stride, bnc, _ = next(it)
            assert cin == x.C == bnc, (name, cin, x.C)
            y = graph.new_act(self, name + '.y', x.H, x.W, x.C)                  # relu(bn(x)): the conv's operand
            d = graph.conv_desc(self, name, y, cout, k, stride, ops.pad_to(cout, ch))
            out = graph.new_act(self, name, d.Ho, d.Wo, cout)
            bnsave(name, x, bnc)
            note(out)
            self.plan.append(('bnconv', name, x, y, out))
            return out

        # stem: conv -> batch norm -> ReLU -> 3x3 / stride-2 max pool, then the units (RetinaNet.py:260-285)
        feats = graph.preact_resnet(self, it, self.block_list, bnconv, bnsave)
        if self.is_pretraining:
            return self._build_pretraining(feats[-1], it)
        self.levels = graph.fpn(self, bnconv, *feats[-3:])
        self.shapes = [(a.H, a.W) for a in self.levels]
        A = sum(h * w * self.num_anchors for h, w in self.shapes)
        self.num_anchor_boxes = A
        self.pconf = torch.zeros(N, A, self.num_classes, device=dev)
        self.pbox = torch.zeros(N, A, 4, device=dev)
        off = 0
        for lvl in self.levels:
            for target, width in ((self.pconf, self.num_classes), (self.pbox, 4)):
                c = lvl
                for _ in range(5):
                    c = bnconv(c)
                self.plan.append(('pred', c, target, off, width))
            off += lvl.H * lvl.W * self.num_anchors
        assert next(it, None) is None and off == A
        self.ws = torch.zeros(self._max_ws, dtype=torch.uint8, device=dev)
        graph.filter_table(self, self._rows(self.specs[1:]))                     # dgrad-layout filters (every conv but the stem)
        # anchors (RetinaNet.py:328-355; x uses the H rate: data_shape[1] is read as the height, :330)
        flat = [v for s in ANCHOR_SIZES for hw in level_priors(s) for v in hw]
        self.anc = ops.retina_anchors(self.data_shape[1], self.shapes, [self.num_anchors] * 5, flat, dev)     # y1x1, y2x2, yx, hw
        if self.mode == 'train':
            self._build_backward(N, A, dt, dev)
        self._refresh_operand_copies()

    def _build_backward(self, N, A, dt, dev):
        self.dconf, self.dbox = torch.zeros_like(self.pconf), torch.zeros_like(self.pbox)
        self.scr_y = torch.zeros(self._max_scr, dtype=dt, device=dev)          # d(relu(bn(x))): lives inside one layer
        self.scr_x = torch.zeros(self._max_scr, dtype=dt, device=dev)          # dx of a batch norm whose input already holds a gradient
        # the gradient sources write: a 'pred' into its subnet's last layer, the pre-training head ('gap') into the last sum's buffer
        source = lambda op: ([], [op[1]])
        io = dict(graph.TRUNK_IO, pred=source, gap=source, bnconv=lambda op: ([op[4]], [op[2]]))
        self.g = {}
        self.bplan = [op + (acc,) if op[0] in ('bnconv', 'resize_add') else op for op, acc in self._reverse(io) if op[0] != 'add']
        P = 1
        i32 = dict(dtype=torch.int32, device=dev)
        self.m_ngt = torch.zeros(N, **i32)
        self.m_status = torch.zeros(N, A, dtype=torch.uint8, device=dev)
        self.m_rg = torch.zeros(N, A, **i32)
        self.m_counts = torch.zeros(N, 4, **i32)
        self.m_best = None
        self.m_ws = None
        self.loss_parts = torch.zeros(N, 2, device=dev)
        self.gt = None

    # ------------------------------------------------------------------ forward / loss / backward
    def _bn_relu(self, name, x, y, training):
        sm, si = self.bnsave[name]
        if self.is_pretraining and training:
            # deliberate: the pre-training train_op is optimizer.minimize() WITHOUT the UPDATE_OPS dependency of the detection graph (RetinaNet.py:134
            # against :221-222), so under TF the moving statistics stay 0 / 1 for the whole pre-training and test mode normalises with them.
            # odtk_bn_fwd always updates the statistics it is handed: it gets a throwaway scratch
            ops.bn_fwd(x.t, x.M, x.C, x.ld, self.param(name + '.gamma'), self.param(name + '.beta'), self.stat_scratch[: x.C],
                       self.stat_scratch[x.C: 2 * x.C], sm, si, training, 1, y.t, y.ld, x.M, 0, self.ws)
            return
        ops.bn_fwd(x.t, x.M, x.C, x.ld, self.param(name + '.gamma'), self.param(name + '.beta'), self.stat(name + '.mmean'),
                   self.stat(name + '.mvar'), sm, si, training, 1, y.t, y.ld, x.M, 0, self.ws)

    def _forward(self, training, subtract_mean=True):
        ops.preprocess(self.images, MEAN_RGB if subtract_mean else (0., 0., 0.), self.input.ld, self.DT, self.input.t)
        for op in self.plan:
            kind = op[0]
            if kind == 'bnconv':
                _, name, x, y, out = op
                self._bn_relu(name, x, y, training)
                ops.conv2d_fwd(self.desc[name], y.t, self._flat(name + '.w', self.Pc), self.param(name + '.b'), out.t, False)
            elif kind == 'pred':
                _, c, target, off, width = op
                K = self.num_anchors * width
                ops.rows_to_f32(c.t, c.ld, target[0, off:], K, c.H * c.W, target.shape[1] * width, c.M, K)
            elif kind == 'gap':
                self._gap_head(training)
            else:                                               # add, resize_add, pool, the stem's convolution
                graph.trunk_fwd(self, op)
                if kind == 'stem':
                    self._bn_relu(op[1], op[3], op[4], training)

    def _loss(self, grad_scale):
        N, P = self.gt.shape[0], self.gt.shape[1]
        if self.m_best is None or self.m_best.shape[1] != P:
            self.m_best = torch.zeros(N, P, dtype=torch.int32, device=self.dev)
            self.m_ws = ops.retina_match_workspace(self.num_anchor_boxes, N, P, self.dev)
        y1x1, y2x2, yx, hw = self.anc
        ops.retina_match(y1x1, y2x2, hw, self.gt, self.m_ngt, self.m_best, self.m_status, self.m_rg, self.m_counts, self.m_ws)
        ops.retina_loss(self.pconf, self.pbox, yx, hw, self.gt, self.m_ngt, self.m_best, self.m_status, self.m_rg, self.m_counts, self.alpha,
                        self.gamma, grad_scale, self.loss_parts, self.dconf, self.dbox)

    def _backward_iter(self):
        for op in self.bplan:
            kind = op[0]
            if kind == 'pred':
                _, c, target, off, width = op
                d = self.dconf if target is self.pconf else self.dbox
                K = self.num_anchors * width
                ops.rows_from_f32(d[0, off:], K, c.H * c.W, d.shape[1] * width, self.grad_of(c), c.ld, c.M, K)
            elif kind == 'gap':
                f = op[1]
                ops.gap_softmax_ce_bwd(self.dlogits, f.N, f.H * f.W, f.C, self.grad_of(f), f.ld, False)
            elif kind == 'bnconv':
                _, name, x, y, out, acc = op
                dz = self.grad_of(out)
                ops.conv2d_wgrad(self.desc[name], y.t, dz, out.ld, self._flat(name + '.w', self.G), self._flat(name + '.b', self.G))
                dy = self.scr_y[: y.M * y.ld].view(y.M, y.ld)
                ops.conv2d_dgrad(self.desc[name], dz, out.ld, self.wt[name], None, dy, False)
                sm, si = self.bnsave[name]
                dx = self.scr_x[: x.M * x.ld].view(x.M, x.ld) if acc else self.grad_of(x)
                ops.bn_bwd(x.t, y.t, dy, x.M, x.C, x.ld, y.ld, x.M, 0, self.param(name + '.gamma'), sm, si, 1, dx,
                           self._flat(name + '.gamma', self.G), self._flat(name + '.beta', self.G), self.ws)
                if acc:
                    gx = self.grad_of(x)
                    ops.add2d(gx, x.ld, dx, x.ld, gx, x.ld, x.M, x.ld)
                yield name
            elif kind in ('resize_add', 'pool'):
                graph.trunk_bwd(self, op)
            else:                                               # stem: the conv bias feeds batch norm -> zero gradient
                _, name, src, z, y = op
                sm, si = self.bnsave[name]
                dzs = self.scr_y[: z.M * z.ld].view(z.M, z.ld)
                ops.bn_bwd(z.t, y.t, self.grad_of(y), z.M, z.C, z.ld, y.ld, z.M, 0, self.param(name + '.gamma'), sm, si, 1, dzs,
                           self._flat(name + '.gamma', self.G), self._flat(name + '.beta', self.G), self.ws)
                ops.conv2d_wgrad(self.desc[name], src.t, dzs, z.ld, self._flat(name + '.w', self.G), None)
                yield name

    # ------------------------------------------------------------------ public: training
    def set_batch(self, images, ground_truth):
        if self.is_pretraining:                     # (images, labels)
            return self._set_pretraining_batch(images, ground_truth)
        self._set_batch_engine(images, ground_truth)

    def train_step(self, lr):
        """one optimizer step on the batch of set_batch(); returns the loss (data + L2) as a 1-element device tensor"""
        if self.is_pretraining:
            return self._pretraining_step(lr)
        return self._train_step_engine(lr)

    def _step_loss(self):
        return self.loss_parts.sum() / self.batch_size + self.weight_decay * self.l2_sum          # RetinaNet.py:205-213

    # ------------------------------------------------------------------ public: inference
    def test_images(self, images):
        """heads.BatchedInference.test_images (with more anchors than the NMS takes per problem the tail compacts the candidate rows first: odtk_compact_rows +
        odtk_gather_rows); a pre-training model returns the predicted classes instead"""
        if self.is_pretraining:
            return self._test_pretraining_images(images)
        return super().test_images(images)

    def _forward_test(self):
        self._forward(False, subtract_mean=bool(self.config.get('test_subtract_mean', False)))      # reference quirk: the fed tensor is `images - mean`

    def _make_tail(self):
        return heads.BatchedTail(self.batch_size, self.pconf.shape[1], self.num_classes - 1, self.nms_max_boxes, self.dev, **self._nms_params())

    def _launch_tail(self, t):
        ops.retina_decode_batched(self.pconf, self.pbox, self.anc[2], self.anc[3], self.nms_score_threshold, t.conf, t.boxes, t.keep, t.cand)
        t.launch_own(self.nms_iou_threshold)

    def evaluate(self, num_images=None, generator=None, **kw):
        """detection graph: VOC mAP (voc_eval.EvaluateMixin.evaluate).  Pre-training graph: held-out accuracy, see _evaluate_pretraining
        (keyword: top_k = 5)."""
        if self.is_pretraining:
            return self._evaluate_pretraining(num_images, generator, **kw)
        return super().evaluate(num_images, generator, **kw)

    # ------------------------------------------------------------------ checkpoints / data parallel
    OPT_SLOT_SCOPE = 'inference/'           # the momentum slots are created inside the 'inference' scope (RetinaNet.py:172, :206)
    TF_STATS_OPTIONAL = True                # a pre-training checkpoint holds no moving statistics (RetinaNet.py:548-551)

    def tf_variable_map(self):
        """the variables of the reference's detection `tf.train.Saver()` (RetinaNet.py:553-557)"""
        return OrderedDict((ours, tfname) for tfname, ours in reference_variable_map(self.block_list).items())

    def _tf_is_backbone(self, ours, tfname):
        return int(ours[1:].split('.')[0]) < 1 + 4 * sum(self.block_list)          # stem + units, their moving statistics included when the file has them

    def save_weight(self, mode, path):
        """RetinaNet.py:521-531.  config['checkpoint_format'] = 'tf' writes tf.train.Saver files (tf_checkpoint.py)."""
        return self._save_weight_engine(mode, path)

    def load_pretraining_weight(self, path):
        """RetinaNet.py:537-539 restores the 'feature_extractor' variables saved by the pre-training graph: here the backbone layers
        (stem + units) of a saved file"""
        self._load_backbone_weight(path, 'load pretraining weight')

    def attach_data_parallel(self, group=None, bucket_mb=25, grad_dtype='f32', force_collectives=False, collective='torch'):
        if self.is_pretraining:
            raise NotImplementedError('data-parallel training of the classification pre-training graph is not built yet: run it on one device')
        return super().attach_data_parallel(group, bucket_mb, grad_dtype, force_collectives, collective)

    # ------------------------------------------------------------------ classification pre-training (is_pretraining: True)
    def _build_pretraining(self, feat, it):
        """the rest of _build for the pre-training graph (RetinaNet.py:120-135): the last unit's sum -> global average pool -> softmax
        cross-entropy.  No pyramid, subnets or anchors."""
        assert next(it, None) is None
        N, dev, dt = self.batch_size, self.dev, self.tdt
        self.feat = feat                              # C = 4 * FILTERS[-1] = 224 logits (no dense layer, :124-125)
        self.plan.append(('gap', feat))
        self.levels, self.shapes, self.num_anchor_boxes, self.anc = [], [], 0, None
        # zero anchors: the detection loss buffers that _build_backward allocates come out empty
        self.pconf = torch.zeros(N, 0, self.num_classes, device=dev)
        self.pbox = torch.zeros(N, 0, 4, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.labels = torch.zeros(N, **i32)
        self.logits = torch.zeros(N, feat.C, device=dev)
        self.ce = torch.zeros(N, device=dev)
        self.pred = torch.zeros(N, **i32)
        self.correct = torch.zeros(N, device=dev)
        self.dlogits = torch.zeros(N, feat.C, device=dev)
        self.last_accuracy = torch.zeros((), device=dev)
        self.stat_scratch = torch.zeros(2 * max(s[5] for s in self.specs), device=dev)     # the moving statistics odtk_bn_fwd updates (_bn_relu)
        self.ws = torch.zeros(self._max_ws, dtype=torch.uint8, device=dev)
        graph.filter_table(self, self._rows(self.specs[1:]))
        if self.mode == 'train':
            self._build_backward(N, 0, dt, dev)
        self._refresh_operand_copies()

    @property
    def num_pretraining_classes(self):
        return self.feat.C

    def _gap_head(self, with_labels):
        f = self.feat
        if with_labels:
            ops.gap_softmax_ce_fwd(f.t, f.ld, f.N, f.H * f.W, f.C, self.labels, 1.0 / self.loss_divisor_batch, self.logits, self.ce, self.pred,
                                   self.correct, self.dlogits)
        else:
            ops.gap_softmax_ce_fwd(f.t, f.ld, f.N, f.H * f.W, f.C, None, 0., self.logits, None, self.pred, None, None)

    def _set_pretraining_batch(self, images, labels):
        images = torch.as_tensor(images, dtype=torch.float32)
        if self.data_format == 'channels_first' and images.shape[1] == 3:
            images = images.permute(0, 2, 3, 1)
        assert tuple(images.shape) == tuple(self.images.shape), images.shape
        lab = np.asarray(labels.detach().cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
        C = self.feat.C
        if lab.shape[0] != self.batch_size or lab.dtype.kind not in 'iuf' or (lab.dtype.kind == 'f' and not np.array_equal(lab, np.trunc(lab))):
            raise ValueError(f'labels: {self.batch_size} integer class ids expected, got {lab.dtype} {lab.shape}')
        if lab.size and (lab.min() < 0 or lab.max() >= C):
            # the pre-training logits are the {C} channels of the last unit (RetinaNet.py:124-126); TF's GPU kernel would give a NaN loss
            raise ValueError(f'labels must lie in [0, {C}): got [{lab.min()}, {lab.max()}]')
        self.images.copy_(images, non_blocking=True)
        self.labels.copy_(torch.from_numpy(lab.astype(np.int32)), non_blocking=True)

    def _pretraining_step(self, lr):
        """RetinaNet.py:126-135: loss = mean CE + wd * sum l2 over l0 .. l64, Momentum 0.9, global_step + 1.  self.last_accuracy (device scalar)
        is the batch accuracy of this step's training-mode forward pass, before the update."""
        self.G.zero_()
        self._forward(True)
        for _ in self._backward_iter():
            pass
        self._optimizer_step(lr)
        self._fp_batch.run()
        # :128-130 compares pred (int64) with labels (int32), which TF 1.x refuses as written: the evident intent, mean(pred == label), is built
        self.last_accuracy = self.correct.mean()
        return self.ce.sum() / self.batch_size + self.weight_decay * self.l2_sum

    def _train_pretraining_epoch(self, lr):
        """RetinaNet.py:476-486: (mean loss, mean accuracy) over num_train // batch_size steps"""
        if callable(self.train_initializer):
            self.train_initializer()
        mean_loss, mean_acc = [], []
        num_iters = self.num_train // self.batch_size
        it = iter(self.train_iterator)
        for i in range(num_iters):
            try:
                images, labels = next(it)
            except StopIteration:
                it = iter(self.train_iterator)
                images, labels = next(it)
            self.set_batch(images, labels)
            loss = float(self.train_step(lr).item())
            acc = float(self.last_accuracy.item())
            if self.verbose:
                sys.stdout.write('\r>> ' + 'iters ' + str(i) + str('/') + str(num_iters) + ' loss ' + str(loss) + ' acc ' + str(acc))
                sys.stdout.flush()
            mean_loss.append(loss)
            mean_acc.append(acc)
        if self.verbose:
            sys.stdout.write('\n')
        return np.mean(mean_loss), np.mean(mean_acc)

    def _evaluate_pretraining(self, num_images=None, generator=None, top_k=5):
        """Held-out top-1 / top-k accuracy and mean cross-entropy of the pre-training graph over `generator`: batches (images [B, H, W, 3], labels [B]),
        the set_batch contract, or an (initializer, iterator) pair.  Defaults: the data provider's val_generator and num_val (when > 0); a generator
        that repeats without end needs a count.  Returns ClassificationEvaluator.result(): {'num_images', 'top1', 'topk', 'top_k', 'loss',
        'class_seen', 'class_accuracy', 'invalid_labels'}.

        BATCH STATISTICS, on a TRAIN-mode model: as in the reference, this graph never updates its moving statistics (the pre-training train_op has no
        UPDATE_OPS dependency, RetinaNet.py:134; _bn_relu) -- they stay 0 / 1 for the whole run, so a test-mode forward pass classifies at chance
        whatever the weights are.  Held-out accuracy is therefore computed the way the reference computes its training accuracy: set_batch, then the
        training-mode forward pass (batch statistics, whose moving-average update goes to a throwaway scratch), then odtk_classify_eval on the logits.
        Nothing else runs: no backward pass, no optimizer step -- P, Mom, S and global_step are bit-identical afterwards.  It follows that every batch
        must hold exactly batch_size images (another size raises ValueError) and that num_images is rounded DOWN to whole batches; 'num_images' of
        the result is the count actually evaluated.  A test-mode pre-training model cannot be evaluated and says so."""
        from .classify_eval import ClassificationEvaluator
        from .voc_eval import _batches
        if self.mode != 'train':
            raise ValueError("evaluate: a test-mode pre-training model normalises with its moving statistics, which the pre-training graph never updates "
                             "(they are 0 / 1): it classifies at chance whatever the weights.  Call evaluate() on the train-mode model (batch statistics)")
        if generator is None:
            generator = getattr(self, 'val_generator', None)
            if generator is None:
                raise ValueError("evaluate: no generator given and the data provider has no val_generator")
            if num_images is None:
                nv = getattr(self, 'num_val', 0)
                num_images = int(nv) if nv and int(nv) > 0 else None
        if num_images is None and getattr(generator, 'endless', False):
            raise ValueError("evaluate: this generator repeats without end (voc_data.get_generator): give num_images, or num_val > 0 in the data provider")
        B = self.batch_size
        batches = None if num_images is None else int(num_images) // B
        if batches is not None and batches < 1:
            raise ValueError(f"evaluate: num_images = {num_images} is less than one batch of batch_size = {B} images")
        ev = self._classify_evaluator = ClassificationEvaluator(self.feat.C, top_k, device=self.dev)
        done = 0
        for images, labels in _batches(generator):
            if images.shape[0] != B:
                raise ValueError(f"evaluate: a batch of {images.shape[0]} images: the pre-training graph is evaluated with batch statistics at batch_size = "
                                 f"{B} (drop the remainder)")
            self.set_batch(images, labels)
            self._forward(True)
            ev.update(self.logits, self.labels)
            done += 1
            if batches is not None and done >= batches:
                break
        r = ev.result()
        if r['invalid_labels'] > 0:
            raise ValueError(f"evaluate: {r['invalid_labels']} labels outside [0, {self.feat.C})")
        return r

    def _test_pretraining_images(self, images):
        """test_images of a test-mode pre-training model: n <= test_batch_size images in one forward pass at N = test_batch_size -> the predicted
        classes, int64 [n] (moving statistics 0 / 1 as in the reference: see _evaluate_pretraining for held-out accuracy)"""
        n = self._stage_test_images(images)
        self._forward_test()
        return self.pred[:n].cpu().numpy().astype(np.int64)

    def _test_one_pretraining_image(self, images):
        """RetinaNet.py:501-503: the predicted class, int64 [1] (the fed tensor bypasses the mean subtraction unless test_subtract_mean)"""
        return self._test_pretraining_images(images)

    def export_pretraining_tf_variables(self):
        """what the pre-training `tf.train.Saver(tf.trainable_variables('feature_extractor'))` (RetinaNet.py:548-551) writes: the kernels, biases,
        gammas and betas of l0 .. l64 under the detection graph's names -- no moving statistics, no momentum slots, no global_step"""
        return OrderedDict((tfname, self._to_tf(ours, self.P)) for ours, tfname in self.tf_variable_map().items() if ours in self.pinfo)

    def _save_pretraining_weight(self, mode, path):
        """RetinaNet.py:509-519.  'tf': exactly the trainables of the pre-training Saver; torch: the same trainables plus momentum and global_step
        (to resume), marked as a pre-training file.  Both load into a detection model through load_pretraining_weight."""
        assert (mode in ['latest', 'best'])
        dirname = os.path.dirname(path)
        if dirname and not os.path.exists(dirname):
            os.makedirs(dirname)
            print(dirname, 'does not exist, create it done')
        prefix = path + '-' + str(self.global_step)
        if self.config.get('checkpoint_format', 'torch') == 'tf':
            from . import tf_checkpoint
            tf_checkpoint.write_bundle(prefix, self.export_pretraining_tf_variables())
            tf_checkpoint.update_checkpoint_state(prefix)
        else:
            blob = {'params': OrderedDict((k, self.get_param(k)) for k in self.pinfo), 'momentum': self.Mom.detach().cpu(), 'global_step': self.global_step,
                    'layout': {k: (int(o), tuple(int(x) for x in shp)) for k, (o, shp) in self.pinfo.items()}, 'pretraining': True}
            torch.save(blob, prefix)
        print('save', mode, 'model in', path, 'successfully')

    def _load_pretraining_model_weight(self, path):
        """load_weight of the pre-training model: the trainables of l0 .. l64 (the pre-training Saver's variables) from a file of either format
        and either graph; momentum and global_step too from a torch pre-training file of this layout"""
        if os.path.exists(str(path) + '.index'):
            stats = self.S.clone()
            self.load_tf_checkpoint(path, backbone_only=True)
            self.S.copy_(stats)                       # the pre-training Saver restores no moving statistics
            print('load weight', path, 'successfully')
            return
        blob = torch.load(path, map_location='cpu', weights_only=True)
        missing = [k for k in self.pinfo if k not in blob['params']]
        if missing:
            raise ValueError(f'{path}: {len(missing)} parameters of this model are not in the checkpoint (e.g. {missing[:3]})')
        self.load_oracle_params({k: v for k, v in blob['params'].items() if k in self.pinfo})
        if blob.get('pretraining') and dict(blob['layout']) == dict(self.pinfo):
            self.Mom.copy_(blob['momentum'].to(self.dev))
            self.global_step = int(blob.get('global_step', 0))
        print('load weight', path, 'successfully')


def reference_variable_map(block_list=(3, 4, 6, 3)):
    """name of every variable of the reference's detection graph -> our parameter / statistic name.  tf.layers default layer names
    (conv2d, conv2d_1, ...; batch_normalization, _1, ...) are numbered PER ENCLOSING variable scope; scopes: 'feature_extractor' for the stem and the
    pyramid, 'feature_extractor/block<b>_unit<u>/conv_branch|identity_branch' for the units (RetinaNet.py:621-643), 'regressor' for the
    subnets (:145).  Pinned by tests/golden/retinanet_variables.json (collected from the reference's own class)."""
    scopes = ['feature_extractor']
    for b, blocks in enumerate(block_list):
        for u in range(blocks):
            base = f'feature_extractor/block{b + 1}_unit{u + 1}'
            scopes += [base + '/conv_branch'] * 3 + [base + '/identity_branch']
    scopes += ['feature_extractor'] * 7 + ['regressor'] * 50
    m, count = OrderedDict(), {}
    for i, scope in enumerate(scopes):
        k = count.get(scope, 0)                      # default layer names are numbered per enclosing variable scope
        count[scope] = k + 1
        sfx = '' if k == 0 else f'_{k}'
        m[f'{scope}/conv2d{sfx}/kernel'], m[f'{scope}/conv2d{sfx}/bias'] = f'l{i}.w', f'l{i}.b'
        bn = f'{scope}/batch_normalization{sfx}'
        m[bn + '/gamma'], m[bn + '/beta'] = f'l{i}.gamma', f'l{i}.beta'
        m[bn + '/moving_mean'], m[bn + '/moving_variance'] = f'l{i}.mmean', f'l{i}.mvar'
    return m
