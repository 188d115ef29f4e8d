"""CenterNet (DLA backbone + transposed-conv up-sampling tree + centre detector) behind the reference's class surface, on libodtk.

Reference: /root/reference/CenterNet.py
  * constructor, config keys ............. :11-47   (input_size, score_threshold, top_k_results_output; testcenternet.py:20-32)
  * input ................................ :49-70   ((images / 255 - mean) / std; test mode feeds the tensor AFTER that transform, so fed
                                                     pixels bypass it -- reproduced, config 'test_normalize' opts out)
  * network .............................. :72-134, :325-431: every layer conv(bias) -> batch norm -> ReLU; _basic_block's shortcut is
                                           tf.cond(channels == filters, identity, 1x1 conv): TensorFlow builds both branches, so the
                                           1x1 conv + batch norm exist as variables where they are never used ("ghost" layers: in the L2
                                           term, moved by weight decay only); DLA aggregation (one activation feeds several sums);
                                           4x4 / stride-2 transposed convolutions; 2x2 max and average pooling
  * loss, optimizer ...................... :136-157 (odtk_centernet_loss; mean over images + wd * l2(all trainables); AdamOptimizer)
  * inference ............................ :158-185 (heads.CenterNetBatched: 3x3 peak test + top-k, no NMS)
  * train / test / checkpoints ........... :298-323
Layers c0 .. c65 in creation order (layer k = conv k + batch norm k), one flat f32 parameter buffer + Adam's two moment buffers.
A transposed convolution runs as the DGRAD of the stride-2 conv it is the gradient of (its kernel stored as that conv's filter
[cin][4][4][cout]); its own backward is that conv's forward (input gradient) and wgrad with the operands swapped (filter gradient).
Every activation owns its gradient buffer; a consumer either writes it (first) or accumulates (later consumers) -- decided once, when
the plan is built -- so an activation may feed any number of sums and layers (the DLA tree needs that; yolov3.py's shared-buffer
residuals cover one sum per activation only).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

from . import graph, heads, ops
from ._lib import BF16
from .base import DetectorBase, _Act
from .warmup import F32Warmup

MEAN = (0.485, 0.456, 0.406)                                  # CenterNet.py:52-53
STD = (0.229, 0.224, 0.225)
STRIDE = 4.0                                                   # :126
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8                  # tf.train.AdamOptimizer defaults (:154)


def layer_specs(num_classes):
    """[(name, kind, cin, cout, k, stride, relu, ghost)] in creation order (CenterNet.py:72-134, :378-402); kind 'conv' | 'dconv'"""
    specs = []

    def add(kind, cin, cout, k, s, relu=True, ghost=False):
        specs.append((f'c{len(specs)}', kind, cin, cout, k, s, relu, ghost))
        return cout

    def block(cin, f):
        add('conv', cin, f, 3, 1); add('conv', f, f, 3, 1)
        add('conv', cin, f, 1, 1, ghost=(cin == f))

    def dla(cin, f, levels):
        if levels == 1:
            block(cin, f); block(f, f)
        else:
            dla(cin, f, levels - 1); dla(f, f, levels - 1)
        add('conv', f, f, 3, 1)
    add('conv', 3, 16, 7, 1); add('conv', 16, 16, 3, 1); add('conv', 16, 32, 3, 2)
    dla(32, 64, 1)
    dla(64, 128, 2); add('conv', 64, 128, 1, 1)
    dla(128, 256, 2); add('conv', 128, 256, 1, 1)
    dla(256, 512, 1); add('conv', 256, 512, 1, 1)
    add('conv', 512, 256, 1, 1)
    for _ in range(3):
        add('dconv', 256, 256, 4, 2)
    add('conv', 256, 256, 1, 1); add('conv', 256, 256, 3, 1)
    add('dconv', 256, 256, 4, 2); add('dconv', 256, 256, 4, 2)
    add('conv', 128, 256, 1, 1); add('conv', 256, 256, 3, 1)
    add('dconv', 256, 256, 4, 2)
    add('conv', 256, 256, 3, 1); add('conv', 256, 256, 1, 1)
    add('conv', 256, num_classes, 3, 1, relu=False); add('conv', 256, 2, 3, 1, relu=False); add('conv', 256, 2, 3, 1, relu=False)
    return specs


class CenterNet(heads.BatchedInference, F32Warmup, graph.OwnedGradients, DetectorBase):
    OPT_BUFFERS = ('M1', 'M2')                                 # Adam's m and v
    OPT_BLOB_KEYS = ('adam_m', 'adam_v')
    OPT_NOT_RESTORED = 'parameter layout differs from this model ({} vs {} entries): Adam moments NOT restored'
    OPT_SLOTS = ('Adam', 'Adam_1')
    # `optimizer.minimize` runs INSIDE `with tf.variable_scope('center_detector')` (CenterNet.py:131-156), and both the slot creator
    # (`variable_scope(None, primary.op.name + '/Adam')`) and the non-slot accumulators take the enclosing scope as a prefix
    OPT_SLOT_SCOPE = 'center_detector/'
    OPT_SLOTS_STRICT = True
    PROGRESS_FROM = 1                                          # CenterNet.py's epoch loop prints i + 1

    def __init__(self, config, data_provider):
        self._prologue(config, data_provider, native_test_batch=True, nms=False)
        self.input_size = config['input_size']
        self.data_shape = [self.input_size, self.input_size, 3] if config['data_format'] == 'channels_last' else [3, self.input_size, self.input_size]
        self.prob = 1. - config['keep_prob']                   # unused, as in the reference
        assert self.input_size % 32 == 0, "CenterNet needs an input that is a multiple of 32 (five halvings; SAME pooling of odd maps is not implemented)"
        if self.mode == 'test':
            self.score_threshold = config['score_threshold']
            self.top_k_results_output = config['top_k_results_output']
        # engine: bf16 by default on the GPU since round 3 (warmup.py: the first f32_warmup_steps optimizer steps of a run from random initialisation go through
        # an f32 twin); an explicit 'compute_dtype' is taken literally; the CPU stand-in of the library (host-logic tests) stays on f32
        # (mode 'test' keeps f32 unless asked otherwise, as ssd300.py does: the bf16 gate checks training gradients, not thresholded detections)
        self._set_engine(config.get('compute_dtype', 'bf16' if (self.dev.type == 'cuda' and self.mode == 'train') else 'f32'))
        self.specs = layer_specs(self.num_classes)
        self._init_parameters(int(config.get('seed', 0)))
        self._build()
        self._warmup_setup(config, data_provider, 'compute_dtype' in config)

    # ------------------------------------------------------------------ parameters
    @staticmethod
    def _rows(specs):
        """dconv: the filter [cin][k][k][cout] of the conv it is the gradient of"""
        return [graph.Row(name, (cout, k, k, cin) if kind == 'conv' else (cin, k, k, cout), cout, cout, True, cin * k * k)
                for name, kind, cin, cout, k, _, _, _ in specs]

    def _init_parameters(self, seed):
        graph.init_parameters(self, self._rows(self.specs), seed)
        self.Mom = self.M1                                     # (name the data-parallel / checkpoint helpers of the other classes use)

    def _check_oracle_param(self, k, v):
        if k.endswith('.b') and self._layer_kind[k[:-2]] == 'dconv' and float(torch.as_tensor(v).abs().max()) != 0.0:
            raise NotImplementedError('non-zero bias of a transposed convolution (TensorFlow initialises it to 0 and, in front of a '
                                      'batch norm, neither the loss gradient nor the weight decay ever moves it)')

    # ------------------------------------------------------------------ the graph: buffers + launch plan
    def _build(self):
        N, dev, dt, ch = self.batch_size, self.dev, self.tdt, self.chunk
        S_ = self.input_size
        self._layer_kind = {s[0]: s[1] for s in self.specs}
        self.images = torch.zeros(N, S_, S_, 3, device=dev)
        self.input = _Act('input', N, S_, S_, 3, ops.pad_to(3, ch), dt, dev)
        self.plan, self.desc, self.z, self.bnsave, self.acts = [], {}, {}, {}, {'input': self.input}
        it = iter(self.specs)
        self._max_ws = self._max_z = self._max_scr = 0

        def act(name, H_, W_, C_, f32=False):
            a = _Act(name, N, H_, W_, C_, C_ if f32 else ops.pad_to(C_, ch), torch.float32 if f32 else dt, dev)
            self.acts[name] = a
            return a

        def layer(src, out_f32=False):
            """conv / transposed conv + batch norm (+ ReLU): graph.conv_bn without dilation, mask or prediction tensor"""
            name, kind, cin, cout, k, stride, relu, ghost = next(it)
            assert not ghost
            return graph.conv_bn(self, (name, kind, cin, cout, k, stride, 1, relu), src, lambda Ho, Wo: act(name, Ho, Wo, cout, out_f32))

        def ghost():
            spec = next(it)
            assert spec[7], spec

        def add(*ins):
            a = ins[0]
            y = act(f'sum{len(self.plan)}', a.H, a.W, a.C)
            self.plan.append(('add', list(ins), y))
            return y

        def pool(x, kind):
            y = act(f'{kind}{len(self.plan)}', x.H // 2, x.W // 2, x.C)
            self._max_scr = max(self._max_scr, x.M * x.ld)
            self.plan.append((kind, x, y))
            return y

        def block(x, f):
            c = layer(layer(x))
            if x.C == f:
                ghost()
                return add(c, x)
            return add(c, layer(x))

        def dla(x, f, levels):
            if levels == 1:
                b1 = block(x, f); b2 = block(b1, f)
            else:
                b1 = dla(x, f, levels - 1); b2 = dla(b1, f, levels - 1)
            return layer(add(b1, b2))

        x = layer(layer(layer(self.input)))
        stages = [pool(dla(x, 64, 1), 'maxpool')]
        for f, levels in ((128, 2), (256, 2), (512, 1)):
            prev = stages[-1]
            d_ = dla(prev, f, levels)
            res = pool(layer(prev), 'avgpool')
            stages.append(add(pool(d_, 'maxpool'), res))
        s3, s4, s5, s6 = stages
        u6 = layer(s6)
        u6_5 = layer(u6); u6_4 = layer(u6_5); u6_3 = layer(u6_4)
        u5 = layer(s5)
        u5_4 = layer(layer(add(u5, u6_5)))
        u5_3 = layer(u5_4)
        u4 = layer(s4)
        u4_3 = layer(layer(add(u4, u5_4, u6_4)))
        feat = layer(layer(add(u6_3, u5_3, u4_3)))
        self.kp_act, self.off_act, self.size_act = layer(feat, True), layer(feat, True), layer(feat, True)
        assert next(it, None) is None
        self.keypoints = self.kp_act.t.view(N, self.kp_act.H, self.kp_act.W, self.num_classes)
        self.offset = self.off_act.t.view(N, self.off_act.H, self.off_act.W, 2)
        self.size = self.size_act.t.view(N, self.size_act.H, self.size_act.W, 2)
        self.ws = torch.zeros(self._max_ws, dtype=torch.uint8, device=dev)
        # dgrad-layout filters: the backward of every conv but the first, and the FORWARD of every transposed conv
        graph.filter_table(self, self._rows(s for s in self.specs if not s[7] and s[0] != 'c0'))
        self.loss_ws = ops.centernet_workspace(N, self.kp_act.H, self.kp_act.W, self.num_classes, dev)
        if self.mode == 'train':
            self._build_backward(N, dt, dev)
        self._refresh_operand_copies()

    def _build_backward(self, N, dt, dev):
        self._alloc_backward()
        emit, written = self.emit, self._written
        self.d_kp, self.d_off, self.d_size = torch.zeros_like(self.keypoints), torch.zeros_like(self.offset), torch.zeros_like(self.size)
        self.kp_act.g, self.off_act.g, self.size_act.g = (t.view(a.M, a.ld) for t, a in ((self.d_kp, self.kp_act), (self.d_off, self.off_act),
                                                                                        (self.d_size, self.size_act)))
        written.update((id(self.kp_act), id(self.off_act), id(self.size_act)))
        # Round 6: an input of a sum whose ONLY consumer is that sum has d(input) = d(sum) exactly: it SHARES the sum's gradient buffer instead of receiving a
        # copy of it (DLA's aggregation nodes and residual sums: 85 add2d launches per step were 6.5 % of the step, a good part of them such copies).  Nobody
        # writes into a shared buffer again -- every reader (the producer's batch-norm / pool backward, another sum) only reads d(output).
        consumers = {}
        for op in self.plan:
            for a in ([op[3]] if op[0] == 'bn' else op[1] if op[0] == 'add' else [op[1]]):
                consumers[id(a)] = consumers.get(id(a), 0) + 1
        self.bplan = []
        self.shared_grads = 0
        for op in reversed(self.plan):
            kind = op[0]
            if kind == 'bn':
                src, y = op[3], op[5]
                assert id(y) in written, op[1]
                self.bplan.append(op + (emit(src) if src is not self.input else False,))
            elif kind == 'add':
                _, ins, y = op
                assert id(y) in written
                todo = []
                for a in ins:
                    if consumers[id(a)] == 1 and a.g is None and a is not self.input and (a.M, a.ld) == (y.M, y.ld) and self.config.get('share_sum_gradients', True):
                        a.g = y.g                                  # shared: no launch
                        written.add(id(a))
                        self.shared_grads += 1
                    else:
                        todo.append((a, emit(a)))
                self.bplan.append(('add', todo, y))
            else:
                _, x, y = op
                assert id(y) in written
                self.bplan.append((kind, x, y, emit(x)))
        self.loss_parts = torch.zeros(N, 4, device=dev)
        self.gt = None

    # ------------------------------------------------------------------ forward / loss / backward
    def _forward(self, training, normalize=True):
        if normalize:
            ops.preprocess_norm(self.images, 255., MEAN, STD, self.input.ld, self.DT, self.input.t)
        else:
            ops.preprocess(self.images, (0., 0., 0.), self.input.ld, self.DT, self.input.t)
        for op in self.plan:
            kind = op[0]
            if kind == 'bn':
                graph.conv_bn_fwd(self, op, training)
            elif kind == 'add':
                _, ins, y = op
                ops.add2d(ins[0].t, ins[0].ld, ins[1].t, ins[1].ld, y.t, y.ld, y.M, y.ld)
                for a in ins[2:]:
                    ops.add2d(y.t, y.ld, a.t, a.ld, y.t, y.ld, y.M, y.ld)
            elif kind == 'maxpool':
                _, x, y = op
                ops.maxpool_fwd(x.t, y.t, x.N, x.H, x.W, x.C, x.ld, y.H, y.W, 2, 2, 0, 0)
            else:
                _, x, y = op
                ops.avgpool2x2_fwd(x.t, y.t, x.N, x.H, x.W, x.ld)

    def _loss(self, grad_scale):
        ops.centernet_loss(self.keypoints, self.offset, self.size, self.gt, STRIDE, grad_scale, self.loss_parts, self.d_kp, self.d_off, self.d_size,
                           self.loss_ws)

    def _backward_iter(self):
        for op in self.bplan:
            kind = op[0]
            if kind == 'bn':
                graph.conv_bn_bwd(self, op)
                yield op[1]
            elif kind == 'add':
                _, ins, y = op
                for a, acc in ins:                              # (accumulating: d(a) first, d(y) second -- refinedet.py's binary sum passes them the other way round)
                    if acc:
                        ops.add2d(a.g, a.ld, y.g, y.ld, a.g, a.ld, a.M, a.ld)
                    else:
                        ops.add2d(y.g, y.ld, None, 0, a.g, a.ld, a.M, a.ld)
            elif kind == 'maxpool':
                _, x, y, acc = op
                ops.maxpool_bwd(x.t, y.t, y.g, self._into(x, acc), x.N, x.H, x.W, x.C, x.ld, y.H, y.W, 2, 2, 0, 0)
                self._fold(x, acc)
            else:
                _, x, y, acc = op
                ops.avgpool2x2_bwd(y.g, self._into(x, acc), x.N, x.H, x.W, x.ld)
                self._fold(x, acc)

    # ------------------------------------------------------------------ public: training
    def _optimizer_step(self, lr):
        """AdamOptimizer: the step counter first, its bias correction needs t"""
        self.global_step += 1
        t = self.global_step
        lr_t = lr * math.sqrt(1.0 - ADAM_B2 ** t) / (1.0 - ADAM_B1 ** t)
        ops.adam(self.P, self.M1, self.M2, self.G, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, self.weight_decay, 1.0, self.l2_partial,
                 self.Pc if self.DT == BF16 else None)
        ops.sum_f32(self.l2_partial, self.l2_sum)

    def _step_loss(self):
        return self.loss_parts[:, 3].mean() + self.weight_decay * self.l2_sum          # CenterNet.py:152-153 (pre-update weights)

    # ------------------------------------------------------------------ public: inference
    def _forward_test(self):
        # Reference quirk, reproduced by default: test mode re-binds self.images to the normalised tensor and feeds THAT one
        # (CenterNet.py:66-67, :312), so fed pixels bypass the (x / 255 - mean) / std transform.
        self._forward(False, normalize=bool(self.config.get('test_normalize', False)))

    def _make_tail(self):
        return heads.CenterNetBatched(self.batch_size, self.kp_act.H, self.kp_act.W, self.top_k_results_output, self.dev)

    def _launch_tail(self, t):
        t.launch(self.keypoints, self.offset, self.size, self.score_threshold, STRIDE)

    # ------------------------------------------------------------------ checkpoints / data parallel
    def tf_variable_map(self):
        """the variables of the reference's `tf.train.Saver()` (CenterNet.py:296-301)"""
        return OrderedDict((ours, tfname) for tfname, ours in reference_variable_map(self.num_classes).items())

    def _tf_extra_variables(self):
        """AdamOptimizer's accumulators `center_detector/beta1_power` / `beta2_power` (= beta^(t + 1) after t steps)"""
        return {self.OPT_SLOT_SCOPE + 'beta1_power': np.asarray(ADAM_B1 ** (self.global_step + 1), dtype=np.float32),
                self.OPT_SLOT_SCOPE + 'beta2_power': np.asarray(ADAM_B2 ** (self.global_step + 1), dtype=np.float32)}

    def load_pretrained_weight(self, path):
        """CenterNet.py:321-323: `pretrained_saver` restores the trainable variables under 'backone' (c0 .. c49)"""
        self._load_backbone_weight(path, 'load pretrained weight')


def reference_variable_map(num_classes=20):
    """name of every variable of the reference's graph -> our parameter / statistic name: default layer names numbered per enclosing
    variable scope ('backone' sic :73, 'upsampling' :111, 'center_detector' :131); conv2d and conv2d_transpose count separately, the
    batch norms over both.  Pinned by tests/golden/centernet_variables.json (from the reference's own class on the shim)."""
    m, count = OrderedDict(), {}
    for i, (name, kind, *_rest) in enumerate(layer_specs(num_classes)):
        scope = 'backone' if i < 50 else ('upsampling' if i < 63 else 'center_detector')
        base = 'conv2d' if kind == 'conv' else 'conv2d_transpose'
        k = count.get((scope, base), 0); count[(scope, base)] = k + 1
        b = count.get((scope, 'bn'), 0); count[(scope, 'bn')] = b + 1
        cn = f'{scope}/{base}' + (f'_{k}' if k else '')
        bn = f'{scope}/batch_normalization' + (f'_{b}' if b else '')
        m[cn + '/kernel'], m[cn + '/bias'] = name + '.w', name + '.b'
        m[bn + '/gamma'], m[bn + '/beta'] = name + '.gamma', name + '.beta'
        m[bn + '/moving_mean'], m[bn + '/moving_variance'] = name + '.mmean', name + '.mvar'
    return m
