"""The host plumbing every detector class shares: the flat parameter store, the constructor prologue, batch staging, the step skeleton, the epoch
loop, torch and tf.train.Saver checkpoints and the data-parallel hook.  No kernel launch order lives here: a class owns its layer list, `_build`,
`_forward`, `_loss` and `_backward_iter`; what those have in common between classes -- the layout and initialisation loop, the dgrad-filter table, the two
backward planners (shared / owned gradient buffers), the pre-activation ResNet + pyramid of RetinaNet and FCOS, the conv + batch-norm op of CenterNet and
RefineDet320 -- is graph.py.  (ssd300.SSD300 keeps a step of its own: three streams, recorded lists, split graphs.)

What a class provides:
  * `specs` and the layout: `pinfo` (and `sinfo` if it has moving statistics) name -> (offset, shape) into the flat buffers, then `_alloc_flat`
    (graph.init_parameters from the class's graph.Row list);
  * `_logical_cin(layer)`: the un-padded input-channel count of a layer's filter (`get_param` cuts the pad channels off with it);
  * `_prologue(...)` at the top of its constructor, then `_set_engine(...)` with its own engine default;
  * the step: `_forward(training)`, `_loss(grad_scale)`, `_backward_iter()` and `_step_loss()`, the value train_step returns.  Where it differs from the
    default: `_loss_scale()`, `_layer_ready(name)`, `_optimizer_step(lr)`; `use_graph` = True replays forward + loss + backward from one HIP graph;
  * the Saver files: `tf_variable_map()` (our name -> the reference graph's variable name) and OPT_SLOT_SCOPE.  Where it differs: OPT_SLOTS,
    `_to_tf` / `_from_tf` (kernel layouts), `_tf_extra_variables()`, `_tf_is_backbone(ours, tfname)`, TF_STATS_OPTIONAL, OPT_SLOTS_STRICT;
  * optional: `_check_oracle_param(name, value)` (load_oracle_params), PROGRESS_FROM, OPT_BUFFERS / OPT_BLOB_KEYS / OPT_NOT_RESTORED.
A class on the f32 warm-up lists warmup.F32Warmup in front of this one (its `set_batch` / `train_step` / `save_weight` wrap the `_engine` methods here).
"""
from __future__ import annotations

import os
import sys
import warnings
import zipfile
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from ._lib import BF16, F32, F32X3


class _Act:
    """rows x pitch activation.  Its gradient: `gid` names the buffer it shares with its residual partners (YOLOv3, RetinaNet, FCOS), or `g` is the
    buffer itself, allocated by graph.OwnedGradients.emit (CenterNet, RefineDet320).  `vgg`: a bias + ReLU layer's output (its ReLU mask is the
    activation); alloc=False: a prediction layer whose rows live in the class's prediction tensor"""

    def __init__(self, name, N, H, W, C, ld, dtype, dev, vgg=False, alloc=True):
        self.name, self.N, self.H, self.W, self.C, self.ld, self.vgg = name, N, H, W, C, ld, vgg
        self.M = N * H * W
        self.t = torch.zeros(self.M, ld, dtype=dtype, device=dev) if alloc else None
        self.gid = name
        self.g = None


def store_padded(name, dst, value):
    """`value` into `dst`, the view of entry `name` in a flat buffer: a filter ('.w', [K, R, S, Cin]) fills the first Cin of dst's input channels and
    the pad channels are zeroed; anything else is copied reshaped"""
    value = torch.as_tensor(value, dtype=torch.float32).to(dst.device)
    if name.endswith('.w'):
        dst.zero_()
        dst[..., : value.shape[-1]] = value
    else:
        dst.copy_(value.view(dst.shape))


class DetectorBase:
    OPT_BUFFERS = ('Mom',)            # flat optimizer-state buffers laid out like P (CenterNet: ('M1', 'M2')) ...
    OPT_BLOB_KEYS = ('momentum',)     # ... and the keys they have in a torch checkpoint (part of the file format)
    OPT_NOT_RESTORED = ('the parameter layout of the checkpoint differs from this model ({} vs {} entries): '
                        'momentum NOT restored (it stays as it is) although global_step is')
    OPT_SLOTS = ('Momentum',)         # ... and the slot variables `<scope><variable>/<slot>` they are in a tf.train.Saver file (CenterNet: ('Adam', 'Adam_1'))
    OPT_SLOT_SCOPE = ''               # the variable scope that is open where the reference creates its optimizer, with its '/'
    OPT_SLOTS_STRICT = False          # restore: a slot is found by suffix under ANY scope and a missing one is passed over in silence; True (CenterNet):
                                      # only under '' or OPT_SLOT_SCOPE, and missing ones are warned about (global_step drives Adam's bias correction)
    TF_STATS_OPTIONAL = False         # restore: a moving statistic absent from the file is skipped (RetinaNet: a pre-training file holds none)
    PROGRESS_FROM = 0                 # train_one_epoch prints the iteration counted from here: each reference file's own print
    sinfo = {}                        # a class without moving statistics (FCOS) leaves it empty and has no S
    GT_ROWS_LIMIT = ops.GT_ROWS_MAX   # ground-truth rows per image (pad_truth_to) the class's matching / loss kernels take (YOLOv2, LHRCNN: GT_ROWS_MAX_NARROW)
    use_graph = False                 # the step's forward + loss + backward replay from one HIP graph (a class reads it from its config)
    _graph, _graph_gt, _eager_steps = None, None, 0

    # ------------------------------------------------------------------ constructor prologue
    def _prologue(self, config, data_provider, native_test_batch=False, nms=True, num_val_optional=False):
        """the config keys and the data provider every class reads; test mode has one image slot, or config['test_batch_size'] of them in the classes
        with a batched `test_images` (native_test_batch).  The class then picks its engine: `_set_engine`."""
        assert config['mode'] in ['train', 'test']
        assert config['data_format'] in ['channels_first', 'channels_last']
        self.config = config
        self.data_provider = data_provider
        self.num_classes = config['num_classes']
        self.weight_decay = config['weight_decay']
        self.data_format = config['data_format']
        self.mode = config['mode']
        self.batch_size = config['batch_size'] if self.mode == 'train' else (self._test_batch_size(config) if native_test_batch else 1)
        if nms:
            self.nms_score_threshold = config['nms_score_threshold']
            self.nms_max_boxes = config['nms_max_boxes']
            self.nms_iou_threshold = config['nms_iou_threshold']
        self._read_nms_method(config, nms)
        self.verbose = bool(config.get('verbose', True))
        self.dev = torch.device(config.get('device', 'cuda:0'))
        if self.mode == 'train':
            self.num_train = data_provider['num_train']
            if not num_val_optional:
                self.num_val = data_provider['num_val']
            self.train_generator = data_provider['train_generator']
            if isinstance(self.train_generator, tuple) and len(self.train_generator) == 2:
                self.train_initializer, self.train_iterator = self.train_generator
            else:
                self.train_initializer, self.train_iterator = None, self.train_generator
            if data_provider.get('val_generator') is not None:
                if num_val_optional:
                    self.num_val = data_provider['num_val']
                self.val_generator = data_provider['val_generator']
        self.global_step = 0
        self.dist = None
        self.loss_divisor_batch = self.batch_size
        if self.dev.type == 'cuda':          # (a 'cpu' device only gets past ops._p with the mocked library of tests/mock_ops.py: host-logic tests)
            torch.cuda.set_device(self.dev)

    def _read_nms_method(self, config, nms):
        """config['nms_method']: 'hard' (default: the reference's greedy NMS, today's launches) | 'linear' | 'gaussian' (soft-NMS, odtk_soft_nms_image_class);
        config['soft_nms_sigma'] (default 0.5, > 0) and config['soft_nms_min_score'] (>= 0; default: whatever nms_score_threshold is at the time of the call).
        A class without an NMS (CenterNet: top-k decode) takes 'hard' only."""
        method = config.get('nms_method', 'hard')
        if not isinstance(method, str) or method not in ops.NMS_METHODS:
            raise ValueError(f"nms_method must be 'hard', 'linear' or 'gaussian', not {method!r}")
        if not nms:
            if method != 'hard':
                raise ValueError(f"nms_method = {method!r}: {type(self).__name__} has no NMS (its decode is a top-k over peaks); only 'hard' is accepted")
            return

        def number(key, default, ok, rule):
            if key not in config:
                return default
            v = config[key]
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not ok(v):
                raise ValueError(f"{key} must be a number {rule}, not {v!r}")
            return float(v)
        self.nms_method = method
        self.soft_nms_sigma = number('soft_nms_sigma', 0.5, lambda v: v > 0, '> 0')
        self._soft_nms_min_score = number('soft_nms_min_score', None, lambda v: v >= 0, '>= 0')

    @property
    def soft_nms_min_score(self):
        return self.nms_score_threshold if self._soft_nms_min_score is None else self._soft_nms_min_score

    def _nms_params(self):
        """what heads.BatchedTail and heads._per_class_nms take beside the IoU threshold"""
        return dict(method=self.nms_method, sigma=self.soft_nms_sigma, min_score=self.soft_nms_min_score)

    def _set_engine(self, engine):
        """'bf16' | 'f32' | 'f32x3': f32 tensors, convolution descriptors of dtype ODTK_F32X3 (three bf16 MFMA products per f32 product where that is
        faster: include/odtk.h).  Which one a class defaults to, and why, is written in that class."""
        self.DT = {'bf16': BF16, 'f32': F32, 'f32x3': F32}[engine]
        self.CDT = F32X3 if engine == 'f32x3' else self.DT
        self.tdt = torch.bfloat16 if self.DT == BF16 else torch.float32
        self.chunk = ops.chunk(self.DT)

    # ------------------------------------------------------------------ flat parameter store
    def _alloc_flat(self, nparam, nstat=None):
        """P, the optimizer buffers, G, the compute-dtype copy Pc (P itself on the f32 engines), S if the class has statistics, the L2 partials"""
        dev = self.dev
        self.nparam = nparam
        self.P = torch.zeros(nparam, device=dev)
        for name in self.OPT_BUFFERS:
            setattr(self, name, torch.zeros(nparam, device=dev))
        self.G = torch.zeros(nparam, device=dev)
        self.Pc = torch.zeros(nparam, dtype=self.tdt, device=dev) if self.DT == BF16 else self.P
        if nstat is not None:
            self.S = torch.zeros(nstat, device=dev)
        self.l2_partial = torch.zeros(ops.sgd_blocks(nparam), device=dev)
        self.l2_sum = torch.zeros(1, device=dev)

    def param(self, name, buf=None):
        off, shape = self.pinfo[name]
        buf = self.P if buf is None else buf
        return buf[off: off + int(np.prod(shape))].view(shape)

    def stat(self, name):
        off, shape = self.sinfo[name]
        return self.S[off: off + int(np.prod(shape))].view(shape)

    def _flat(self, name, buf):
        off, shape = self.pinfo[name]
        return buf[off: off + int(np.prod(shape))]

    def set_param(self, name, value, buf=None):
        """value in the logical shape (conv kernels [K,R,S,Cin] un-padded) into P, or into an optimizer buffer `buf`"""
        store_padded(name, self.param(name, buf), value)

    def _logical_cin(self, layer):
        return self._cin[layer]

    def get_param(self, name, buf=None):
        v = self.param(name, buf).detach().cpu().clone()
        if name.endswith('.w'):
            v = v[..., : self._logical_cin(name[:-2])].contiguous()
        return v

    def _to_tf(self, name, buf):
        """parameter `name` out of a flat buffer (P or an optimizer buffer) in TensorFlow's layout: kernels HWIO (transposed convs [h, w, out, in]), un-padded"""
        v = self.get_param(name, buf)
        return np.ascontiguousarray((v.permute(1, 2, 3, 0) if name.endswith('.w') else v).numpy())

    def _from_tf(self, name, array):
        """the inverse: a variable of a tf.train.Saver file in the layout set_param takes"""
        v = torch.from_numpy(np.asarray(array))
        return v.permute(3, 0, 1, 2).contiguous() if name.endswith('.w') else v

    def _check_oracle_param(self, name, value):
        """hook of load_oracle_params: raise for a value this class cannot hold"""

    def load_oracle_params(self, p):
        """dict name -> tensor in the oracle's naming ([K,R,S,Cin] kernels); names the model does not have are ignored"""
        if getattr(self, 'f32_warmup_steps', 0):
            self.cancel_warmup()                                   # weights are loaded: the run does not start from random initialisation
        for k, v in p.items():
            if k in self.pinfo:
                self._check_oracle_param(k, v)
                self.set_param(k, v)
            elif k in self.sinfo:
                self.stat(k).copy_(torch.as_tensor(v, dtype=torch.float32).to(self.dev))
        self._refresh_operand_copies()

    def _sync_from_twin(self):
        """(warmup.F32Warmup overrides it: mid-warm-up the live weights are the twin's)"""

    def export_params(self):
        self._sync_from_twin()
        out = OrderedDict((k, self.get_param(k)) for k in self.pinfo)
        for k in self.sinfo:
            out[k] = self.stat(k).detach().cpu().clone()
        return out

    def _refresh_operand_copies(self):
        if self.DT == BF16:
            ops.cast_from_f32(self.P, self.Pc)
        if getattr(self, '_fp_batch', None) is not None:
            self._fp_batch.run()

    # ------------------------------------------------------------------ batch staging, epoch loop
    def _set_batch_engine(self, images, ground_truth):
        images = torch.as_tensor(images, dtype=torch.float32)
        if self.data_format == 'channels_first' and images.shape[1] == 3:
            images = images.permute(0, 2, 3, 1)
        assert tuple(images.shape) == tuple(self.images.shape), images.shape
        self.images.copy_(images, non_blocking=True)
        gt = torch.as_tensor(ground_truth, dtype=torch.float32)
        if self.gt is None or self.gt.shape != gt.shape:
            ops.check_gt_rows(type(self).__name__, gt.shape, self.GT_ROWS_LIMIT)
            self.gt = torch.zeros(gt.shape, device=self.dev)
            self._gt_reshaped(gt.shape)
        self.gt.copy_(gt, non_blocking=True)

    def _gt_reshaped(self, shape):
        """hook of _set_batch_engine: the ground-truth buffer was (re)allocated with this shape"""

    def _stage_test_image(self, images):
        """the one image of a batch-1 test-mode model into self.images (the classes without a batched test_images)"""
        images = torch.as_tensor(np.asarray(images), dtype=torch.float32)
        if self.data_format == 'channels_first' and images.shape[1] == 3:
            images = images.permute(0, 2, 3, 1)
        assert self.batch_size == 1 and tuple(images.shape) == tuple(self.images.shape), images.shape
        self.images.copy_(images)

    # ------------------------------------------------------------------ the optimizer step
    def _loss_scale(self):
        """what the loss kernels scale their gradients with: d(mean over the images of the GLOBAL batch)"""
        return 1.0 / self.loss_divisor_batch

    def _layer_ready(self, name):
        """data parallel: `_backward_iter` yielded `name`, every gradient of that layer and of all later layers has been launched"""
        self.dist.layer_ready(name)

    def _step_body(self):
        self.G.zero_()
        self._forward(True)
        self._loss(self._loss_scale())
        for name in self._backward_iter():
            if self.dist is not None:
                self._layer_ready(name)

    def _optimizer_step(self, lr):
        """MomentumOptimizer(0.9) over the whole flat buffer, the sum of squares of the PRE-update weights into l2_sum, then the step counter"""
        ops.sgd_momentum(self.P, self.Mom, self.G, lr, 0.9, self.weight_decay, 1.0, self.l2_partial, self.Pc if self.DT == BF16 else None)
        ops.sum_f32(self.l2_partial, self.l2_sum)
        self.global_step += 1

    def _train_step_engine(self, lr):
        """one optimizer step on the batch of set_batch(); returns the loss (data + L2) as a 1-element device tensor.
        use_graph, single device: after two eager steps (the library's lazily grown scratch buffers exist by then) forward + loss + backward replay from
        ONE HIP graph -- the dependent launches leave the queue without host round trips; the optimizer launches stay outside (lr is a launch
        argument).  Which classes gain from it is measured, and written where the class reads 'use_graph'.  Data parallel / sync-BN: eager (collectives
        inside the step)."""
        if self.dist is not None:
            self.dist.begin_step()
        if self.use_graph and self.dist is None and self.dev.type == 'cuda' and self._eager_steps >= 2:
            if self._graph is None or self._graph_gt is not self.gt:
                self._graph = torch.cuda.CUDAGraph()
                self._graph_gt = self.gt                       # the captured launches hold this buffer's pointer and pad length
                with torch.cuda.graph(self._graph):
                    self._step_body()
            self._graph.replay()
        else:
            self._step_body()
            self._eager_steps += 1
        if self.dist is not None:
            self.dist.finish_step()
        self._optimizer_step(lr)
        self._fp_batch.run()
        return self._step_loss()

    def train_one_epoch(self, lr):
        if callable(self.train_initializer):
            self.train_initializer()
        mean_loss = []
        num_iters = self.num_train // self.batch_size
        it = iter(self.train_iterator)
        for i in range(num_iters):
            try:
                images, gt = next(it)
            except StopIteration:
                it = iter(self.train_iterator)
                images, gt = next(it)
            self.set_batch(images, gt)
            loss = float(self.train_step(lr).item())
            if self.verbose:
                sys.stdout.write('\r>> ' + 'iters ' + str(i + self.PROGRESS_FROM) + str('/') + str(num_iters) + ' loss ' + str(loss))
                sys.stdout.flush()
            mean_loss.append(loss)
        if self.verbose:
            sys.stdout.write('\n')
        return np.mean(mean_loss)

    # ------------------------------------------------------------------ checkpoints / data parallel
    def _save_weight_engine(self, mode, path):
        """one torch file `<path>-<step>` (parameters, moving statistics, optimizer buffers, step, layout), or with config['checkpoint_format'] = 'tf'
        the reference's own tf.train.Saver files (`<path>-<step>.index` + `.data-00000-of-00001` + `checkpoint`: tf_checkpoint.py)"""
        assert (mode in ['latest', 'best'])
        dirname = os.path.dirname(path)
        if dirname and not os.path.exists(dirname):
            os.makedirs(dirname)
            print(dirname, 'does not exist, create it done')
        prefix = path + '-' + str(self.global_step)
        if self.config.get('checkpoint_format', 'torch') == 'tf':
            from . import tf_checkpoint
            tf_checkpoint.write_bundle(prefix, self.export_tf_variables())
            tf_checkpoint.update_checkpoint_state(prefix)
        else:
            blob = {'params': self.export_params()}
            for key, name in zip(self.OPT_BLOB_KEYS, self.OPT_BUFFERS):
                blob[key] = getattr(self, name).detach().cpu()
            blob['global_step'] = self.global_step
            blob['layout'] = {k: (int(o), tuple(int(x) for x in shp)) for k, (o, shp) in self.pinfo.items()}
            torch.save(blob, prefix)
        print('save', mode, 'model in', path, 'successfully')

    def load_weight(self, path):
        if os.path.exists(str(path) + '.index'):                 # a tf.train.Saver checkpoint prefix
            self.load_tf_checkpoint(path)
            print('load weight', path, 'successfully')
            return
        blob = torch.load(path, map_location='cpu', weights_only=True)
        unknown = sorted(k for k in blob['params'] if k not in self.pinfo and k not in self.sinfo)
        if unknown:
            raise ValueError(f'{path}: {len(unknown)} parameters of the checkpoint are not part of this model (e.g. {unknown[:3]}): '
                             'it was written by a different layer layout')
        self.load_oracle_params(blob['params'])
        state = [(blob[key], getattr(self, name)) for key, name in zip(self.OPT_BLOB_KEYS, self.OPT_BUFFERS)]
        if all(tuple(saved.shape) == tuple(buf.shape) for saved, buf in state) and dict(blob['layout']) == dict(self.pinfo):
            for saved, buf in state:
                buf.copy_(saved.to(self.dev))
        else:
            warnings.warn(f'{path}: ' + self.OPT_NOT_RESTORED.format(len(blob['layout']), len(self.pinfo)), RuntimeWarning)
        self.global_step = int(blob.get('global_step', 0))
        print('load weight', path, 'successfully')

    # ------------------------------------------------------------------ tf.train.Saver checkpoints (tf_checkpoint.py)
    def tf_variable_map(self):
        """OrderedDict our parameter / statistic name -> the variable's name in the reference's graph, in the order the class exports them"""
        raise NotImplementedError

    def _tf_extra_variables(self):
        """what the reference's Saver writes besides weights, statistics, slots and global_step (CenterNet: Adam's beta powers)"""
        return {}

    def _tf_is_backbone(self, ours, tfname):
        """is this one of the variables the reference's pre-training Saver restores: the trainables under 'backone' (sic), in most of its files"""
        return tfname.startswith('backone') and ours in self.pinfo

    def export_tf_variables(self):
        """what the reference's `tf.train.Saver()` writes: every variable of its graph under its name (tf_variable_map) -- weights and moving
        statistics --, the optimizer's slots `<OPT_SLOT_SCOPE><variable>/<slot>` and global_step"""
        self._sync_from_twin()
        out = OrderedDict()
        for ours, tfname in self.tf_variable_map().items():
            if ours in self.pinfo:
                out[tfname] = self._to_tf(ours, self.P)
                for slot, buf in zip(self.OPT_SLOTS, self.OPT_BUFFERS):
                    out[f'{self.OPT_SLOT_SCOPE}{tfname}/{slot}'] = self._to_tf(ours, getattr(self, buf))
            else:
                out[tfname] = self.stat(ours).detach().cpu().numpy().copy()
        out.update(self._tf_extra_variables())
        out['global_step'] = np.asarray(self.global_step, dtype=np.int32)
        return out

    def load_tf_checkpoint(self, path, backbone_only=False):
        """`saver.restore(sess, path)` from tf.train.Saver files (ours or the reference's): weights, moving statistics, optimizer slots, global_step;
        backbone_only: what the reference's pre-training Saver restores (`_tf_is_backbone`), nothing else"""
        from .tf_checkpoint import NewCheckpointReader
        if getattr(self, 'f32_warmup_steps', 0):
            self.cancel_warmup()                                   # weights are loaded: the run does not start from random initialisation
        reader = NewCheckpointReader(str(path))
        names = list(reader.get_variable_to_shape_map())
        missing = []
        for ours, tfname in self.tf_variable_map().items():
            if backbone_only and not self._tf_is_backbone(ours, tfname):
                continue
            if ours in self.sinfo:
                if reader.has_tensor(tfname) or not self.TF_STATS_OPTIONAL:
                    self.stat(ours).copy_(torch.from_numpy(reader.get_tensor(tfname)).to(self.dev))
                continue
            self.set_param(ours, self._from_tf(ours, reader.get_tensor(tfname)))          # KeyError = Saver's NotFoundError
            for slot, buf in () if backbone_only else zip(self.OPT_SLOTS, self.OPT_BUFFERS):
                # the slot's scope prefix is whatever scope the optimizer was created in: match by suffix
                slot = f'{tfname}/{slot}'
                found = [n for n in names if n.endswith(slot) and (not self.OPT_SLOTS_STRICT or n[: len(n) - len(slot)] in ('', self.OPT_SLOT_SCOPE))]
                if found:
                    self.set_param(ours, self._from_tf(ours, reader.get_tensor(found[0])), getattr(self, buf))
                else:
                    missing.append(slot)
        if not backbone_only and reader.has_tensor('global_step'):
            self.global_step = int(reader.get_tensor('global_step'))
        if missing and self.OPT_SLOTS_STRICT:
            warnings.warn(f'{path}: {len(missing)} {self.OPT_SLOTS[0]} slot variables not in the checkpoint (e.g. {missing[0]}): their moments stay as they are, '
                          f'while global_step = {self.global_step} drives the bias correction', RuntimeWarning)
        self._refresh_operand_copies()

    def _load_backbone_weight(self, path, message):
        """the backbone's variables (`_tf_is_backbone`) from a tf.train.Saver checkpoint or from a torch file (a zip archive) of save_weight"""
        if os.path.exists(str(path) + '.index') or not zipfile.is_zipfile(str(path)):
            self.load_tf_checkpoint(path, backbone_only=True)
        else:
            names = self.tf_variable_map()
            blob = torch.load(path, map_location='cpu', weights_only=True)['params']
            self.load_oracle_params({k: v for k, v in blob.items() if k in names and self._tf_is_backbone(k, names[k])})
        print(message, path, 'successfully')

    def attach_data_parallel(self, group=None, bucket_mb=25, grad_dtype='f32', force_collectives=False, collective='torch'):
        from .dist import GradAllReducer
        self.dist = GradAllReducer(self, group, bucket_mb, grad_dtype, force_collectives, collective)
        self.loss_divisor_batch = self.batch_size * self.dist.world
        return self.dist
