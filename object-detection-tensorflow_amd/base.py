"""The host plumbing every detector class shares: the flat parameter store, the constructor prologue, batch staging, the epoch loop, torch
checkpoints and the data-parallel hook.  No kernel launch order lives here: a class still owns its layer list, `_build`, `_forward`, `_loss`,
`_backward_iter` and `_train_step_engine`.

What a class provides:
  * `specs` and the layout: `pinfo` (and `sinfo` if it has moving statistics) name -> (offset, shape) into the flat buffers, then `_alloc_flat`;
  * `_logical_cin(layer)`: the un-padded input-channel count of a layer's filter (`get_param` cuts the pad channels off with it);
  * optional hooks: `_check_oracle_param(name, value)` (load_oracle_params), PROGRESS_FROM, OPT_BUFFERS / OPT_BLOB_KEYS;
  * `_prologue(...)` at the top of its constructor, then `_set_engine(...)` with its own engine default.
A class on the f32 warm-up lists warmup.F32Warmup in front of this one (its `set_batch` / `train_step` / `save_weight` wrap the `_engine` methods here).
"""
from __future__ import annotations

import os
import sys
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from ._lib import BF16, F32, F32X3


class _Act:
    """rows x pitch activation; `gid` names the gradient buffer it shares with its residual partners"""

    def __init__(self, name, N, H, W, C, ld, dtype, dev):
        self.name, self.N, self.H, self.W, self.C, self.ld = name, N, H, W, C, ld
        self.M = N * H * W
        self.t = torch.zeros(self.M, ld, dtype=dtype, device=dev)
        self.gid = name


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
    PROGRESS_FROM = 0                 # train_one_epoch prints the iteration counted from here: each reference file's own print
    sinfo = {}                        # a class without moving statistics (FCOS) leaves it empty and has no S

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

    def _logical(self, name, buf):
        """parameter `name` out of a flat buffer (P or an optimizer buffer) in TensorFlow's layout: kernels HWIO (transposed convs [h, w, out, in]), un-padded"""
        v = self.get_param(name, buf)
        return np.ascontiguousarray((v.permute(1, 2, 3, 0) if name.endswith('.w') else v).numpy())

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
            self.gt = torch.zeros(gt.shape, device=self.dev)
            self._gt_reshaped(gt.shape)
        self.gt.copy_(gt, non_blocking=True)

    def _gt_reshaped(self, shape):
        """hook of _set_batch_engine: the ground-truth buffer was (re)allocated with this shape"""

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
        if tuple(blob['momentum'].shape) == tuple(self.Mom.shape) and dict(blob['layout']) == dict(self.pinfo):
            self.Mom.copy_(blob['momentum'].to(self.dev))
        else:
            import warnings
            warnings.warn(f'{path}: the parameter layout of the checkpoint differs from this model ({len(blob["layout"])} vs {len(self.pinfo)} entries): '
                          'momentum NOT restored (it stays as it is) although global_step is', RuntimeWarning)
        self.global_step = int(blob.get('global_step', 0))
        print('load weight', path, 'successfully')

    def attach_data_parallel(self, group=None, bucket_mb=25, grad_dtype='f32', force_collectives=False, collective='torch'):
        from .dist import GradAllReducer
        self.dist = GradAllReducer(self, group, bucket_mb, grad_dtype, force_collectives, collective)
        self.loss_divisor_batch = self.batch_size * self.dist.world
        return self.dist
