"""YOLOv3 (DarkNet-53) behind the reference's class surface, on libodtk.

Reference: /root/reference/YOLOv3.py
  * constructor, config keys, data_provider ... :11-60     (`YOLOv3(config, data_provider)`; test mode forces batch 1)
  * input ..................................... :62-79     (images - mean; test mode feeds the tensor AFTER the subtraction,
                                                            so fed pixels bypass the mean -- reproduced, `test_subtract_mean` opts out)
  * network ................................... :81-95, :389-417, :484-514: every conv = conv2d(same, bias) + batch norm
                                                (+ leaky_relu 0.1), INCLUDING the three prediction convs; lateral convs without activation;
                                                heads built with 1024 / 256 / 128 filters on block5 / block4 / block3
  * loss, optimizer ........................... :96-318    (odtk_yolov3_loss; .5 * mean + wd * l2; Momentum 0.9; BN update ops)
  * inference ................................. :320-368    (heads.BatchedInference)
  * train_one_epoch / test_one_image / save_weight / load_weight ... :437-482
Every convolution, batch norm, residual sum, up-sampling and the box side run in libodtk (no torch compute, no CPU
fallback); this file owns the buffers, the launch order and the gradient bookkeeping:
  * activations are [N*H*W][C] rows (NHWC) in the compute dtype (bf16 default, 'f32' for parity tests), pre-BN conv
    outputs are kept for the backward pass;
  * `conv = conv + conv2` (:489-491): the sum node and its two inputs SHARE one gradient buffer -- d(sum) is read by the
    batch-norm backward of conv2, and the 1x1 conv's dgrad later accumulates into the same rows, which then are d(input);
  * concat(bottom, upsampled lateral) (:412) is one buffer of C1 + C2 channels; its halves are addressed by pitch.
Layers are c0 .. c74 in creation (= forward) order; parameters live in one flat f32 buffer in that order (what the
data-parallel gradient buckets of dist.py rely on).
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import graph, heads, ops
from .base import DetectorBase, _Act
from .warmup import F32Warmup

MEAN_RGB = (123.68, 116.779, 103.979)                                       # YOLOv3.py:65
DARKNET_BLOCKS = ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4))         # :391-395
HEAD_FILTERS = (1024, 256, 128)                                             # :83-86
STRIDE = (8., 16., 32.)                                                     # :38
LEAKY = 2                                                                   # odtk_bn_fwd activation code


class YOLOv3(heads.BatchedInference, F32Warmup, graph.SharedGradients, DetectorBase):
    def __init__(self, config, data_provider):
        assert len(config['data_shape']) == 3
        self._prologue(config, data_provider, native_test_batch=True, num_val_optional=True)      # (this class reads num_val only with a val_generator)
        self.data_shape = config['data_shape']
        self.scales = (config['coord_scale'], config['noobj_scale'], config['obj_scale'], config['class_scale'])
        self.num_priors = config['num_priors']
        priors = config['priors']
        # head l (1 = coarsest) is paired with priors[l-1] / stride[l-1], the reference's own pairing (:111-113 with :37-42)
        self.priors_flat = [float(v) / STRIDE[i] for i in range(3) for hw in priors[i] for v in hw]
        self.final_units = (self.num_classes + 5) * self.num_priors
        # 'f32x3' (round 5): f32 tensors, convolution descriptors of dtype ODTK_F32X3 (three bf16 MFMA products per f32 product where that is faster: include/odtk.h)
        # Round 6: the class went through the bf16 admission gate of the other classes, deterministically (tests/test_gpu_bf16_gate.py;
        # profiles/r06_bf16_gate_table.md): filter-gradient cosine of the bf16 engine against the f32 engine on 16 held-out images, minimum over the layers / median of
        # the input-side third -- 0.47 / 0.48 at random initialisation, 0.854 / 0.895 after 300 f32 steps, 0.853 / 0.874 after 600: the class sits AT the bar
        # (0.8 / 0.88) and does not move away from it as training goes on, where SSD300 / FCOS / CenterNet / YOLOv2 keep rising.  By the gate's rule (admitted
        # = above the bar at 300 AND at 600 steps) the bf16 engine is NOT the default for training: with no engine named a training instance on the GPU runs
        # 'f32x3' (f32 tensors, three bf16 MFMA products per f32 product); 'bf16' -- 2.4x the step rate -- is an explicit choice (`compute_dtype='bf16'`,
        # optionally with `f32_warmup_steps`), and what bench.py's yolov3_bf16 line is quoted on.  Test mode and the CPU stand-in keep their engines.
        self._set_engine(config.get('compute_dtype', 'f32x3' if (self.dev.type == 'cuda' and self.mode == 'train') else 'bf16'))
        h, w, c = self.data_shape
        assert c == 3 and h % 32 == 0 and w % 32 == 0, "YOLOv3 needs an input that is a multiple of 32 (five stride-2 stages)"
        # measured: ~1 000 dependent launches of 5-25 us each -- this class's step is launch-bound, replay is the default
        self.use_graph = bool(config.get('use_graph', True))
        self.sync_bn = None
        self.specs = layer_specs(self.num_classes, self.num_priors)
        self._init_parameters(int(config.get('seed', 0)))
        self._build()
        self._warmup_setup(config, data_provider, 'compute_dtype' in config)

    # ------------------------------------------------------------------ parameters
    @staticmethod
    def _rows(specs):
        return [graph.Row(name, (cout, k, k, cin), cout, cout, True, cin * k * k) for name, cin, cout, k, _, _ in specs]

    @staticmethod
    def param_layout(specs, chunk):
        """(pinfo, nparam, sinfo, nstat) of graph.param_layout (host logic, no device needed: the data-parallel bucketing is tested on CPU with exactly
        this layout)"""
        return graph.param_layout(YOLOv3._rows(specs), chunk)

    def _init_parameters(self, seed):
        # synthetic initialisation: variance-scaling kernels (:501), zero bias, BN gamma 1 / beta 0 / moving (0, 1)
        graph.init_parameters(self, self._rows(self.specs), seed)

    # ------------------------------------------------------------------ the graph: buffers + launch plan
    def _build(self):
        N, dev, dt = self.batch_size, self.dev, self.tdt
        H, W, _ = self.data_shape
        self.images = torch.zeros(N, H, W, 3, device=dev)
        c0 = ops.pad_to(3, self.chunk)
        x = _Act('input', N, H, W, 3, c0, dt, dev)
        self.input = x
        self.plan, self.desc, self.z, self.bnsave = [], {}, {}, {}
        self.acts = {'input': x}
        it = iter(self.specs)
        max_ws = max_z = 0
        self._groups = {}                                      # union-find over gradient groups (graph.SharedGradients)

        def conv(src, out_f32=False):
            nonlocal max_ws, max_z
            name, cin, cout, k, stride, act = next(it)
            assert cin == src.C, (name, cin, src.C)
            ldz = ops.pad_to(cout, self.chunk)
            d = ops.conv_desc(N, src.H, src.W, ops.pad_to(cin, self.chunk), src.ld, cout, ldz, k, stride, 1, self.CDT, self.CDT)
            self.desc[name] = d
            z = _Act(name + '.z', N, d.Ho, d.Wo, cout, ldz, dt, dev)
            y = _Act(name, N, d.Ho, d.Wo, cout, cout if out_f32 else ldz, torch.float32 if out_f32 else dt, dev)
            self.z[name], self.acts[name] = z, y
            self.bnsave[name] = (torch.zeros(cout, device=dev), torch.zeros(cout, device=dev))
            max_ws = max(max_ws, ops.bn_workspace_bytes(z.M, cout))
            max_z = max(max_z, z.M * ldz)
            self.plan.append(('conv', name, src, z, y, LEAKY if act else 0))
            return y

        def add(a, b):
            y = _Act(f'sum{len(self.plan)}', N, a.H, a.W, a.C, a.ld, dt, dev)
            self.acts[y.name] = y
            self.union(b, y)                                  # b, a and y share one gradient buffer
            self.union(a, y)
            self.plan.append(('add', a, b, y))
            return y

        def upcat(bottom, lat):
            y = _Act(f'cat{len(self.plan)}', N, bottom.H, bottom.W, bottom.C + lat.C, bottom.C + lat.C, dt, dev)
            self.acts[y.name] = y
            self.plan.append(('upcat', bottom, lat, y))
            return y

        x = conv(x)
        outs = []
        for f, blocks in DARKNET_BLOCKS:
            x = conv(x)
            for _ in range(blocks):
                x = add(x, conv(conv(x)))
            outs.append(x)
        self.pred_acts, top = [], None
        for lvl, bottom in enumerate((outs[4], outs[3], outs[2])):
            x = bottom
            if top is not None:
                x = upcat(bottom, conv(top))
            x = conv(conv(conv(conv(x))))
            top = conv(x)
            self.pred_acts.append(conv(conv(top), out_f32=True))
        assert next(it, None) is None
        self.ws = torch.zeros(max_ws, dtype=torch.uint8, device=dev)
        E = self.num_classes + 5
        self.preds = [a.t.view(N, a.H, a.W, self.num_priors, E) for a in self.pred_acts]
        # dgrad-layout filters (every conv but the first: the input needs no gradient)
        graph.filter_table(self, self._rows(self.specs[1:]))
        if self.mode == 'train':
            # gradient buffers, one per group (the prediction activations' are the views of dpreds); the backward plan records who writes first and who
            # accumulates: a conv into its source, an upcat into `bottom` (its `lat` half is always written first)
            self.zg = torch.zeros(max_z, dtype=dt, device=dev)            # d(pre-BN conv output): lives for one layer
            self.dpreds = [torch.zeros_like(p) for p in self.preds]
            self.g = {self.find(a.gid): dp.view(a.M, a.ld) for a, dp in zip(self.pred_acts, self.dpreds)}
            io = {'conv': lambda op: ([op[4]], [op[2]]), 'upcat': lambda op: ([op[3]], [op[1], op[2]]), 'add': lambda op: ([op[3]], [])}
            self.bplan = [op + (acc,) for op, acc in self._reverse(io) if op[0] != 'add']
            self.loss_parts = torch.zeros(N, 5, device=dev)
            self.loss_ws = ops.yolov3_workspace(self.preds, N, dev)
            self.gt = None
        self._refresh_operand_copies()

    # ------------------------------------------------------------------ forward / backward
    def _forward(self, training, subtract_mean=True):
        ops.preprocess(self.images, MEAN_RGB if subtract_mean else (0., 0., 0.), self.input.ld, self.DT, self.input.t)
        for op in self.plan:
            if op[0] == 'conv':
                _, name, src, z, y, act = op
                ops.conv2d_fwd(self.desc[name], src.t, self._flat(name + '.w', self.Pc), self.param(name + '.b'), z.t, False)
                sm, si = self.bnsave[name]
                if training and self.sync_bn is not None:
                    self.sync_bn.fwd(z.t, z.M, z.C, z.ld, self.param(name + '.gamma'), self.param(name + '.beta'), self.stat(name + '.mmean'),
                                     self.stat(name + '.mvar'), sm, si, act, y.t, y.ld, z.M, 0, self.ws)
                else:
                    ops.bn_fwd(z.t, z.M, z.C, z.ld, self.param(name + '.gamma'), self.param(name + '.beta'), self.stat(name + '.mmean'),
                               self.stat(name + '.mvar'), sm, si, training, act, y.t, y.ld, z.M, 0, self.ws)
            elif op[0] == 'add':
                _, a, b, y = op
                ops.add2d(a.t, a.ld, b.t, b.ld, y.t, y.ld, y.M, y.C)          # (y.C where graph.trunk_fwd passes y.ld: the same number here, every sum has 64 .. 1024 channels)
            else:
                _, bottom, lat, y = op
                ops.add2d(bottom.t, bottom.ld, None, 0, y.t, y.ld, y.M, bottom.C)
                ops.upsample2x_fwd(lat.t, lat.ld, y.t[:, bottom.C:], y.ld, lat.N, lat.H, lat.W, lat.C)

    def _loss(self, grad_scale):
        ops.yolov3_loss(self.preds, self.priors_flat, (STRIDE[2], STRIDE[1], STRIDE[0]), self.gt, self.scales, grad_scale, self.loss_parts,
                        self.dpreds, self.loss_ws)

    def _backward_iter(self):
        """yields a layer name once every gradient of that layer and of all later layers has been launched"""
        for op in self.bplan:
            if op[0] == 'conv':
                _, name, src, z, y, act, acc = op
                dy = self.grad_of(y)
                zg = self.zg[: z.M * z.ld].view(z.M, z.ld)
                sm, si = self.bnsave[name]
                (self.sync_bn.bwd if self.sync_bn is not None else ops.bn_bwd)(
                    z.t, y.t, dy, z.M, z.C, z.ld, y.ld, z.M, 0, self.param(name + '.gamma'), sm, si, act, zg,
                    self._flat(name + '.gamma', self.G), self._flat(name + '.beta', self.G), self.ws)
                # the bias feeds batch norm: its gradient is exactly zero (only weight decay acts on it)
                ops.conv2d_wgrad(self.desc[name], src.t, zg, z.ld, self._flat(name + '.w', self.G), None)
                if src is not self.input:
                    ops.conv2d_dgrad(self.desc[name], zg, z.ld, self.wt[name], None, self.grad_of(src), acc)
                yield name
            else:
                _, bottom, lat, y, acc = op
                dcat = self.grad_of(y)
                db = self.grad_of(bottom)
                if acc:
                    ops.add2d(db, bottom.ld, dcat, y.ld, db, bottom.ld, y.M, bottom.C)
                else:
                    ops.add2d(dcat, y.ld, None, 0, db, bottom.ld, y.M, bottom.C)
                ops.upsample2x_bwd(dcat[:, bottom.C:], y.ld, self.grad_of(lat), lat.ld, lat.N, lat.H, lat.W, lat.C, False)

    # ------------------------------------------------------------------ public: training
    def _loss_scale(self):
        return 0.5 / self.loss_divisor_batch                   # d(.5 * mean_i loss_i)

    def _step_loss(self):
        return 0.5 * self.loss_parts[:, 4].mean() + self.weight_decay * self.l2_sum        # YOLOv3.py:311-315 (pre-update weights)

    # ------------------------------------------------------------------ public: inference
    def _forward_test(self):
        self._forward(False, subtract_mean=bool(self.config.get('test_subtract_mean', False)))      # reference quirk: the fed tensor is `images - mean`

    def _make_tail(self):
        L = sum(p.shape[1] * p.shape[2] * p.shape[3] for p in self.preds)
        return heads.BatchedTail(self.batch_size, L, self.num_classes, self.nms_max_boxes, self.dev, bool_cand=True, **self._nms_params())

    def _launch_tail(self, t):
        """The decode is a LOOP of the existing launch, odtk_yolov3_decode_candidates, one per image slot into [N, L, C] / [N, L, 4]: that entry point takes the
        three level tensors of an image as a pointer table, a batched form would need a table per image, and the loop costs the host's enqueue time, measured
        0.5 ms for 32 images (15 us per image, DESIGN.md *Evaluation*) beside a forward pass of 26 ms; threshold, NMS (N x classes problems), pack and
        read-back are batched."""
        for b in range(self.batch_size):
            ops.yolov3_decode_candidates([p[b] for p in self.preds], self.priors_flat, (STRIDE[2], STRIDE[2], STRIDE[1]), out=(t.conf[b], t.boxes[b]))
        torch.ge(t.conf, self.nms_score_threshold, out=t.cand)
        t.launch_own(self.nms_iou_threshold)

    # ------------------------------------------------------------------ checkpoints / data parallel
    def tf_variable_map(self):
        """the variables of the reference's `tf.train.Saver()` (YOLOv3.py:377-381); the momentum slots are `<variable>/Momentum`: the optimizer is
        created outside any variable scope (:312)"""
        return OrderedDict((ours, tfname) for tfname, ours in reference_variable_map().items())

    def load_tf_checkpoint(self, path, backbone_trainables_only=False, backbone_only=False):
        """backbone_trainables_only (this class's own keyword for backbone_only): what `pretraining_weight_saver` restores (YOLOv3.py:377-378,
        :480-482: the trainable variables under 'backone')"""
        super().load_tf_checkpoint(path, backbone_only or backbone_trainables_only)

    def load_pretraining_weight(self, path):
        """YOLOv3.py:480-482 restores the trainable 'backone' variables: here the c0 .. c51 entries of a saved file"""
        self._load_backbone_weight(path, 'load pretraining weight')

    def attach_data_parallel(self, group=None, bucket_mb=25, sync_bn=False, grad_dtype='f32', force_collectives=False, collective='torch'):
        """images sharded over ranks (one process per GPU); gradients summed with the bucketed RCCL all-reduce of dist.py,
        overlapped with the backward pass; the loss divisor becomes the GLOBAL batch.  sync_bn: batch statistics over all replicas
        (ops.SyncBN), i.e. exactly the single-device computation on the global batch"""
        from .dist import GradAllReducer
        self.dist = GradAllReducer(self, group, bucket_mb, grad_dtype, force_collectives, collective)
        self.loss_divisor_batch = self.batch_size * self.dist.world
        if sync_bn:
            self.sync_bn = ops.SyncBN(group)
        return self.dist


def layer_specs(num_classes=20, num_priors=3):
    """[(name, cin, cout, k, stride, leaky)] in creation order: DarkNet-53 (52 convs, YOLOv3.py:389-396, :484-491), then per level
    [lateral 1x1 (no activation)], 1x1, 3x3, 1x1, 3x3, 1x1, 3x3, prediction 1x1 (:398-417)"""
    specs = []

    def add(cin, cout, k, s, act=True):
        specs.append((f'c{len(specs)}', cin, cout, k, s, act))
        return cout
    c = add(3, 32, 3, 1)
    outs = []
    for f, blocks in DARKNET_BLOCKS:
        c = add(c, f, 3, 2)
        for _ in range(blocks):
            add(c, f // 2, 1, 1)
            add(f // 2, f, 3, 1)
        outs.append(c)
    top = None
    for lvl, f in enumerate(HEAD_FILTERS):
        cin = outs[4 - lvl]
        if top is not None:
            cin += add(top, f, 1, 1, False)
        add(cin, f // 2, 1, 1); add(f // 2, f, 3, 1); add(f, f // 2, 1, 1); add(f // 2, f, 3, 1)
        top = add(f, f // 2, 1, 1)
        add(f // 2, f, 3, 1)
        add(f, (num_classes + 5) * num_priors, 1, 1)
    return specs


def reference_variable_map():
    """name of every variable of the reference's YOLOv3 graph -> our parameter / statistic name.  tf.layers default layer names
    (conv2d, conv2d_1, ...; batch_normalization, _1, ...) are numbered PER ENCLOSING variable scope (Layer._set_scope ->
    variable_scope(None, default_name=...)); the scopes:
    'backone' (sic, YOLOv3.py:82) / 'backone/block<b>' (:485) / 'head/pyd<l>' (:399).  Pinned by tests/golden/yolov3_variables.json
    (collected from the reference's own class)."""
    scopes = ['backone']
    for b, (_, blocks) in enumerate(DARKNET_BLOCKS):
        scopes += [f'backone/block{b + 1}'] * (1 + 2 * blocks)
    for lvl in range(3):
        scopes += [f'head/pyd{lvl + 1}'] * (7 if lvl == 0 else 8)
    m, count = OrderedDict(), {}
    for i, scope in enumerate(scopes):
        k = count.get(scope, 0)                      # default layer names are numbered per enclosing variable scope
        count[scope] = k + 1
        sfx = '' if k == 0 else f'_{k}'
        m[f'{scope}/conv2d{sfx}/kernel'], m[f'{scope}/conv2d{sfx}/bias'] = f'c{i}.w', f'c{i}.b'
        bn = f'{scope}/batch_normalization{sfx}'
        m[bn + '/gamma'], m[bn + '/beta'] = f'c{i}.gamma', f'c{i}.beta'
        m[bn + '/moving_mean'], m[bn + '/moving_variance'] = f'c{i}.mmean', f'c{i}.mvar'
    return m
