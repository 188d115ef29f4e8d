"""FCOS (the reference's group-normalised pre-activation ResNet + pyramid + per-level heads) behind the reference's class surface, on libodtk.

Reference: /root/reference/FCOS.py
  * constructor, config keys ............. :12-49    (blocks 3, 4, 6, 3 and filters 16 * 2^i are fixed in the class, :29-31)
  * input ................................ :51-68    (images - mean; test mode feeds the tensor after the subtraction)
  * network .............................. :70-110, :350-382, :438-513: EVERY normalisation is tf.contrib.layers.group_norm(groups=8);
                                           stem conv + GN + ReLU + 3x3 / s2 max pool; bottleneck units [GN-ReLU-1x1 f, GN-ReLU-3x3 f (stride),
                                           GN-ReLU-1x1 4f] + [GN-ReLU-3x3 4f (stride)] shortcut; c3 / c4 / c5 1x1; bilinear top-down pyramid (the sum is
                                           handed down); p6 / p7; per level 4 x 3x3 -> classes and centre-ness, 4 x 3x3 -> exp(distances), the head WEIGHTS shared by the
                                           levels (variable_scope(..., reuse=tf.AUTO_REUSE), :351, :358)
  * loss, optimizer ...................... :111-192  (odtk_fcos_loss; mean over images + wd * l2; Momentum 0.9)
  * inference ............................ :193-265  (heads.fcos_detect; classes 0 .. C-2, sic)
  * train / test / checkpoints ........... :401-436
Same conventions as retinanet.py: layers l0 .. l85 in creation order (layer k = conv k + group norm k; l75 .. l85 are the heads, ONE set of
weights applied at all five pyramid levels -- instance names l<k>@<level>), one flat f32 parameter buffer.
Group norm has no batch statistics: nothing like moving averages exists, and data parallel needs no sync-BN.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from . import graph, heads, ops
from .base import DetectorBase, _Act
from .voc_eval import EvaluateMixin
from .warmup import F32Warmup

MEAN_RGB = (123.68, 116.779, 103.979)
BLOCKS = (3, 4, 6, 3)                                          # FCOS.py:30
FILTERS = (16, 32, 64, 128)                                    # :31
GROUPS = 8                                                     # :441
PI = 0.01                                                      # :486


def layer_specs(num_classes):
    """[(name, cin, cout, k, stride, gn_channels, bias_init)] in creation order (FCOS.py:70-110, :350-382, :504-513)"""
    specs = []

    def add(cin, cout, k, s, bias_init=0.):
        specs.append((f'l{len(specs)}', cin, cout, k, s, cin if specs else cout, bias_init))
        return cout
    c = add(3, 16, 7, 2)
    stage_out = []
    for i, blocks in enumerate(BLOCKS):
        f = FILTERS[i]
        for j in range(blocks):
            s = 2 if (i > 0 and j == 0) else 1
            add(c, f, 1, 1); add(f, f, 3, s); add(f, 4 * f, 1, 1)
            add(c, 4 * f, 3, s)
            c = 4 * f
        stage_out.append(c)
    e3, e4, e5 = stage_out[-3:]
    add(e3, 256, 1, 1); add(e4, 256, 1, 1); add(e5, 256, 1, 1)
    add(256, 256, 3, 1)
    add(256, 256, 1, 1); add(256, 256, 3, 1)
    add(256, 256, 1, 1); add(256, 256, 3, 1)
    add(256, 256, 3, 2); add(256, 256, 3, 2)
    bias = -math.log((1 - PI) / PI)
    # ONE set of head layers for all five levels: _detect_head enters variable_scope('classifier_head' / 'regress_head',
    # reuse=tf.AUTO_REUSE) once per level (FCOS.py:351, :358); leaving a variable scope resets the default-name counters of its
    # sub-scopes (variable_scope.py, close_variable_subscopes), so every level asks for conv2d, conv2d_1, ... and GroupNorm,
    # GroupNorm_1, ... again and AUTO_REUSE hands back the variables of the first level: convs AND group norms are shared.
    for _ in range(4):
        add(256, 256, 3, 1)
    add(256, num_classes, 3, 1, bias)
    add(256, 1, 3, 1, bias)
    for _ in range(4):
        add(256, 256, 3, 1)
    add(256, 4, 3, 1)
    return specs


HEAD_LAYERS = 11                                               # the last 11 specs: 6 classifier-head + 5 regress-head layers, shared by the levels


class FCOS(EvaluateMixin, F32Warmup, graph.SharedGradients, DetectorBase):
    def __init__(self, config, data_provider):
        ops.check_num_classes('FCOS', config['num_classes'], background=False)
        self._prologue(config, data_provider)
        self.data_shape = config['data_shape']
        # engine: bf16 by default on the GPU since round 3 (warmup.py: the first f32_warmup_steps optimizer steps of a run from random initialisation go through
        # an f32 twin); an explicit 'compute_dtype' is taken literally; the CPU stand-in of the library (host-logic tests) stays on f32
        # (mode 'test' keeps f32 unless asked otherwise, as ssd300.py does: the bf16 gate checks training gradients, not thresholded detections)
        self._set_engine(config.get('compute_dtype', 'bf16' if (self.dev.type == 'cuda' and self.mode == 'train') else 'f32'))
        self.specs = layer_specs(self.num_classes)
        self._init_parameters(int(config.get('seed', 0)))
        self._build()
        self._warmup_setup(config, data_provider, 'compute_dtype' in config)

    # ------------------------------------------------------------------ parameters
    def _rows(self, specs):                                     # (group norm: no moving statistics, so no S)
        return [graph.Row(name, (cout, k, k, cin), cout, gnc, False, cin * k * k, bias_init) for name, cin, cout, k, _, gnc, bias_init in specs]

    def _init_parameters(self, seed):
        graph.init_parameters(self, self._rows(self.specs), seed)

    # ------------------------------------------------------------------ the graph
    def _build(self):
        N, dev, dt, ch = self.batch_size, self.dev, self.tdt, self.chunk
        H, W, _ = self.data_shape
        self.images = torch.zeros(N, H, W, 3, device=dev)
        c0 = ops.pad_to(3, ch)
        self.input = _Act('input', N, H, W, 3, c0, dt, dev)
        self.plan, self.desc, self.gnsave, self.acts = [], {}, {}, {}
        it = iter(self.specs)
        self._max_scr = 0
        self._groups = {}

        def gnsave(name, a, gnc=None):
            self.gnsave[name] = torch.zeros(N, GROUPS, 2, device=dev)
            self._max_scr = max(self._max_scr, a.M * a.ld)

        def gnconv(x, spec=None, level=None):
            """group norm -> ReLU -> conv(bias): returns the conv output.  `spec`, `level`: a shared head layer applied at one
            pyramid level -- parameters under the layer's name `pname`, buffers / descriptor under the instance name pname@level"""
            pname, cin, cout, k, stride, gnc, _ = next(it) if spec is None else spec
            name = pname if level is None else f'{pname}@{level}'
            assert cin == x.C == gnc and gnc % GROUPS == 0, (name, cin, x.C)
            y = graph.new_act(self, name + '.y', x.H, x.W, x.C)
            d = graph.conv_desc(self, name, y, cout, k, stride, ops.pad_to(cout, ch))
            out = graph.new_act(self, name, d.Ho, d.Wo, cout)
            gnsave(name, y)
            self.plan.append(('gnconv', name, x, y, out, pname))
            return out

        feats = graph.preact_resnet(self, it, BLOCKS, gnconv, gnsave)
        c3, c4, c5 = gnconv(feats[-3]), gnconv(feats[-2]), gnconv(feats[-1])
        self.levels = graph.fpn(self, gnconv, c3, c4, c5)
        self.conf = [torch.zeros(N, a.H, a.W, self.num_classes, device=dev) for a in self.levels]
        self.reg = [torch.zeros(N, a.H, a.W, 4, device=dev) for a in self.levels]
        self.center = [torch.zeros(N, a.H, a.W, 1, device=dev) for a in self.levels]
        head = list(it)                                         # the 11 head layers: one set of weights, five levels
        assert len(head) == HEAD_LAYERS
        for l, lvl in enumerate(self.levels):
            c = lvl
            for j in range(4):
                c = gnconv(c, head[j], l)
            self.plan.append(('pred', gnconv(c, head[4], l), self.conf, l, False))
            self.plan.append(('pred', gnconv(c, head[5], l), self.center, l, False))
            r = lvl
            for j in range(4):
                r = gnconv(r, head[6 + j], l)
            self.plan.append(('pred', gnconv(r, head[10], l), self.reg, l, True))       # tf.exp on the distances (FCOS.py:363)
        graph.filter_table(self, self._rows(self.specs[1:]))            # dgrad-layout filters: one per PARAMETER (shared by the levels)
        if self.mode == 'train':
            self._build_backward(N, dt, dev)
        self._refresh_operand_copies()

    def _build_backward(self, N, dt, dev):
        self.dconf = [torch.zeros_like(t) for t in self.conf]
        self.dreg = [torch.zeros_like(t) for t in self.reg]
        self.dcenter = [torch.zeros_like(t) for t in self.center]
        self.scr_y = torch.zeros(self._max_scr, dtype=dt, device=dev)          # d(relu(gn(x))): lives inside one layer
        self.gn_ws = ops.gn_workspace(N, max(s[5] for s in self.specs), dev)
        io = dict(graph.TRUNK_IO, pred=lambda op: ([], [op[1]]), gnconv=lambda op: ([op[4]], [op[2]]))
        seen_params = set()
        self.g, self.bplan = {}, []
        for op, acc in self._reverse(io):
            kind = op[0]
            if kind == 'gnconv':
                _, name, x, y, out, pname = op
                # a shared head layer: its norm's d(gamma), d(beta) accumulate over the levels (the filter / bias gradients always
                # accumulate); the layer is final -- for the gradient all-reduce -- after the LAST level processed (level 0)
                first_use = pname not in seen_params
                seen_params.add(pname)
                last_use = name == pname or name.endswith('@0')
                self.bplan.append(('gnconv', name, x, y, out, acc, pname, not first_use, last_use))
            elif kind == 'resize_add':
                self.bplan.append(op + (acc,))
            elif kind != 'add':
                self.bplan.append(op)
        self.loss_img = torch.zeros(N, device=dev)
        self.loss_ws = ops.fcos_workspace(self.conf, N, dev)
        self.gt = None

    # ------------------------------------------------------------------ forward / loss / backward
    def _gn_relu(self, name, x, y, pname=None):
        pname = pname or name
        ops.gn_fwd(x.t, x.ld, y.t, y.ld, x.N, x.H * x.W, x.C, GROUPS, self.param(pname + '.gamma'), self.param(pname + '.beta'), 1, self.gnsave[name])

    def _forward(self, training=True, subtract_mean=True):          # (group norm: nothing depends on `training`)
        ops.preprocess(self.images, MEAN_RGB if subtract_mean else (0., 0., 0.), self.input.ld, self.DT, self.input.t)
        for op in self.plan:
            kind = op[0]
            if kind == 'gnconv':
                _, name, x, y, out, pname = op
                self._gn_relu(name, x, y, pname)
                ops.conv2d_fwd(self.desc[name], y.t, self._flat(pname + '.w', self.Pc), self.param(pname + '.b'), out.t, False)
            elif kind == 'pred':
                _, c, targets, l, is_exp = op
                if is_exp:
                    ops.exp_rows_to_f32(c.t, c.ld, targets[l], c.M, c.C)
                else:
                    ops.rows_to_f32(c.t, c.ld, targets[l], c.C, c.M, 0, c.M, c.C)
            else:                                               # add, resize_add, pool, the stem's convolution
                graph.trunk_fwd(self, op)
                if kind == 'stem':
                    self._gn_relu(op[1], op[3], op[4])

    def _loss(self, grad_scale):
        ops.fcos_loss(self.conf, self.reg, self.center, self.gt, grad_scale, self.loss_img, self.dconf, self.dreg, self.dcenter, self.loss_ws)

    def _backward_iter(self):
        for op in self.bplan:
            kind = op[0]
            if kind == 'pred':
                _, c, targets, l, is_exp = op
                if is_exp:
                    ops.exp_rows_bwd(self.dreg[l], self.reg[l], self.grad_of(c), c.ld, c.M, c.C)
                else:
                    d = self.dconf[l] if targets is self.conf else self.dcenter[l]
                    ops.rows_from_f32(d, c.C, c.M, 0, self.grad_of(c), c.ld, c.M, c.C)
            elif kind == 'gnconv':
                _, name, x, y, out, acc, pname, acc_params, last_use = op
                dz = self.grad_of(out)
                ops.conv2d_wgrad(self.desc[name], y.t, dz, out.ld, self._flat(pname + '.w', self.G), self._flat(pname + '.b', self.G))
                dy = self.scr_y[: y.M * y.ld].view(y.M, y.ld)
                ops.conv2d_dgrad(self.desc[name], dz, out.ld, self.wt[pname], None, dy, False)
                ops.gn_bwd(x.t, x.ld, y.t, dy, y.ld, self.grad_of(x), x.ld, x.N, x.H * x.W, x.C, GROUPS, self.param(pname + '.gamma'),
                           self.gnsave[name], 1, int(acc) | (2 if acc_params else 0), self._flat(pname + '.gamma', self.G),
                           self._flat(pname + '.beta', self.G), self.gn_ws)
                if last_use:
                    yield pname
            elif kind in ('resize_add', 'pool'):
                graph.trunk_bwd(self, op)
            else:                                               # stem: conv -> GN -> ReLU (its bias DOES have a gradient: group norm is not
                _, name, src, z, y = op                        # invariant to a per-channel shift inside a group)
                dzs = self.scr_y[: z.M * z.ld].view(z.M, z.ld)
                ops.gn_bwd(z.t, z.ld, y.t, self.grad_of(y), y.ld, dzs, z.ld, z.N, z.H * z.W, z.C, GROUPS, self.param(name + '.gamma'),
                           self.gnsave[name], 1, False, self._flat(name + '.gamma', self.G), self._flat(name + '.beta', self.G), self.gn_ws)
                ops.conv2d_wgrad(self.desc[name], src.t, dzs, z.ld, self._flat(name + '.w', self.G), self._flat(name + '.b', self.G))
                yield name

    # ------------------------------------------------------------------ public: training
    def _step_loss(self):
        return self.loss_img.mean() + self.weight_decay * self.l2_sum                              # FCOS.py:186-187

    # ------------------------------------------------------------------ public: inference
    def test_one_image(self, images):
        self._stage_test_image(images)
        self._forward(False, subtract_mean=bool(self.config.get('test_subtract_mean', False)))
        scores, bbox, cid = heads.fcos_detect([t[0] for t in self.conf], [t[0] for t in self.reg], [t[0] for t in self.center],
                                              self.nms_score_threshold, self.nms_max_boxes, self.nms_iou_threshold, **self._nms_params())
        return [scores.cpu().numpy(), bbox.cpu().numpy().reshape(-1, 4), cid.cpu().numpy()]

    # ------------------------------------------------------------------ checkpoints / data parallel
    OPT_SLOT_SCOPE = 'head/'                # the momentum slots are created under the 'head' scope of the graph (FCOS.py:111, :188)

    def tf_variable_map(self):
        """the variables of the reference's `tf.train.Saver()` (FCOS.py:390-394)"""
        return OrderedDict((ours, tfname) for tfname, ours in reference_variable_map().items())

    def load_pretrained_weight(self, path):
        """FCOS.py:434-436 restores the 'backone' variables: here the stem + unit layers of a saved file"""
        self._load_backbone_weight(path, 'load pretrained weight')


def reference_variable_map():
    """name of every variable of the reference's FCOS graph -> our parameter name.  Default layer names (tf.layers: conv2d, conv2d_1, ...;
    contrib's group_norm: GroupNorm, GroupNorm_1, ...) are numbered PER ENCLOSING variable scope.  Scopes: 'backone' (sic, FCOS.py:71) with
    'block<b>_unit<u>/conv_branch|identity_branch' (:504-513), 'pyramid' (:98), 'head/classifier_head' and 'head/regress_head' (:351, :358) --
    entered once per level with reuse=tf.AUTO_REUSE, which SHARES the 6 + 5 head layers over the five levels (layer_specs).
    Pinned by tests/golden/fcos_variables.json (from the reference's own class on the shim)."""
    scopes = ['backone']
    for b, blocks in enumerate(BLOCKS):
        for u in range(blocks):
            base = f'backone/block{b + 1}_unit{u + 1}'
            scopes += [base + '/conv_branch'] * 3 + [base + '/identity_branch']
    scopes += ['pyramid'] * 10 + ['head/classifier_head'] * 6 + ['head/regress_head'] * 5
    m, count = OrderedDict(), {}
    for i, scope in enumerate(scopes):
        k = count.get(scope, 0)
        count[scope] = k + 1
        sfx = f'_{k}' if k else ''
        m[f'{scope}/conv2d{sfx}/kernel'], m[f'{scope}/conv2d{sfx}/bias'] = f'l{i}.w', f'l{i}.b'
        m[f'{scope}/GroupNorm{sfx}/beta'], m[f'{scope}/GroupNorm{sfx}/gamma'] = f'l{i}.beta', f'l{i}.gamma'
    return m
