#!/usr/bin/env python
"""Generates tests/golden/retinanet_pretrain.npz and retinanet_pretrain_variables.json by constructing the REFERENCE's own RetinaNet class
with `is_pretraining: True` (RetinaNet.py:61-99, :120-135; testretinanet.py's backbone at 128 x 128 / batch 4) on the eager TF-1.x shim:
  * test mode on the initial parameters (`sess.run(pred)` with is_training False and the fed images bypassing the mean subtraction, :501-503):
    logits / pred of one image;
  * two training steps through its session (`sess.run([train_op, loss, accuracy])`, :476-486): loss and accuracy of each, logits and pred of
    the first forward pass, a subsample of some parameters after the FIRST step;
  * name / shape / trainable of every variable of the graph.
The parameters of oracle/retinanet_net_ref.init_params(37) for l0 .. l64 are pushed into the shim's variables in creation order first.
Labels are spread over [0, 224) with 0 and 223 in both batches; two labels of the first batch are the first forward pass's own predictions so
that the recorded accuracy is not trivially 0.

Two gaps of the shim are bridged here: tf.reduce_mean takes no `name=` (wrapped; the wrapper also keeps `global_pool`, the logits), and
Session.run rebuilds the graph through _define_inputs / _build_graph (the pre-training methods are aliased on the instance).
The shim applies the batch-norm moving-statistic updates whenever train_op is fetched; TF does not for this graph (its train_op has no
UPDATE_OPS dependency, :134), so the moving statistics are put back after every run.

Run in the build container (needs /root/reference):   python tests/golden/make_golden_retinanet_pretrain.py [out_dir]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import retinanet_net_ref as NR    # noqa: E402
from oracle import tf_shim                    # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
NB = 65
KEEP = ['l0.w', 'l0.b', 'l0.gamma', 'l0.beta', 'l1.w', 'l1.gamma', 'l3.w', 'l4.w', 'l4.beta', 'l30.w', 'l30.b', 'l45.gamma', 'l61.w', 'l62.w',
        'l63.w', 'l63.b', 'l64.w', 'l64.b', 'l64.gamma', 'l64.beta']
CONFIG = {'is_bottleneck': True, 'residual_block_list': [3, 4, 6, 3], 'init_conv_filters': 16, 'mode': 'train', 'is_pretraining': True,
          'data_shape': [128, 128, 3], 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'data_format': 'channels_last', 'batch_size': 4,
          'gamma': 2.0, 'alpha': 0.25, 'nms_score_threshold': 0.8, 'nms_max_boxes': 10, 'nms_iou_threshold': 0.45}
SEEDS = (700, 701)
TEST_SEED = 702


def images(seed, n=4):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 128, 128, 3, generator=g) * 255).round()


def main():
    tf = tf_shim.install()
    kept = {}
    plain_mean = tf.reduce_mean

    def reduce_mean(x, axis=None, name=None):
        out = plain_mean(x, axis=axis)
        if name == 'global_pool':
            kept['logits'] = out.detach().clone()
        return out
    tf.reduce_mean = reduce_mean
    ref = tf_shim.load_reference_module('/root/reference/RetinaNet.py', 'reference_RetinaNet')
    state = {'images': images(SEEDS[0]), 'labels': torch.tensor([0, 223, 0, 0], dtype=torch.int32)}

    class It:
        def get_next(self):
            return tf_shim.wrap(state['images'].clone()), tf_shim.wrap(state['labels'].clone())
    prov = {'num_train': 8, 'num_val': 0, 'train_generator': (lambda: None, It()), 'val_generator': None}
    m = ref.RetinaNet(dict(CONFIG), prov)
    m._define_inputs, m._build_graph = m._define_pretraining_inputs, m._build_pretraining_graph
    V = tf_shim.S.variables
    variables = {n: dict(shape=list(v.shape), dtype=str(v.dtype).replace('torch.', ''), trainable=n in tf_shim.S.trainable) for n, v in V.items()}
    kernels = [k for k in V if k.endswith('/kernel')]
    bns = [k[:-len('/gamma')] for k in V if k.endswith('/gamma')]
    assert len(kernels) == len(bns) == NB, (len(kernels), len(bns))
    p = NR.init_params(37)
    with torch.no_grad():
        for i, (kn, bn) in enumerate(zip(kernels, bns)):
            V[kn].copy_(p[f'l{i}.w'].permute(1, 2, 3, 0))
            V[kn[:-len('kernel')] + 'bias'].copy_(p[f'l{i}.b'])
            V[bn + '/gamma'].copy_(p[f'l{i}.gamma']); V[bn + '/beta'].copy_(p[f'l{i}.beta'])
    moving = {n: v.detach().clone() for n, v in V.items() if '/moving_' in n}

    def run(fetches, feed):
        out = m.sess.run(fetches, feed_dict=feed)
        with torch.no_grad():
            for n, v in moving.items():            # TF runs no UPDATE_OPS for this train_op (RetinaNet.py:134)
                V[n].copy_(v)
        return out
    # test mode on the initial parameters: one image (with three companions: inference batch norm is per image) fed past the mean subtraction.
    # The test-mode `labels` placeholder (:97) is fed because the shim builds the loss of the whole graph on every run
    timg = images(TEST_SEED, 1)
    pred_t = run(m.pred, {m.images: torch.cat([timg, images(SEEDS[0])[1:]]).numpy(), m.is_training: False})
    out = {'test_image_seed': np.asarray(TEST_SEED), 'test_logits': kept['logits'][0].numpy().copy(), 'test_pred': np.asarray(pred_t[:1], np.int64)}
    # labels: 0 and 223 in both batches, two of the first batch equal to the first forward pass's predictions
    pred0 = run(m.pred, {m.is_training: True})
    labels = [np.asarray([0, 223, int(pred0[2]), int(pred0[3])], np.int32), np.asarray([223, 17, 0, 131], np.int32)]
    losses, accs = [], []
    for step in range(2):
        state['images'], state['labels'] = images(SEEDS[step]), torch.from_numpy(labels[step])
        _, loss, acc = run([m.train_op, m.loss, m.accuracy], {m.lr: 0.01, m.is_training: True})
        losses.append(float(loss)); accs.append(float(acc))
        if step:
            continue
        out['logits0'] = kept['logits'].numpy().copy()
        out['pred0'] = np.asarray(kept['logits'].argmax(1).numpy(), np.int64)
        for key in KEEP:
            i, kind = int(key[1:].split('.')[0]), key.split('.')[1]
            name = {'w': kernels[i], 'b': kernels[i][:-len('kernel')] + 'bias', 'gamma': bns[i] + '/gamma', 'beta': bns[i] + '/beta'}[kind]
            v = V[name].detach()
            v = v.permute(3, 0, 1, 2) if kind == 'w' else v
            flat = v.contiguous().reshape(-1)
            out[key.replace('.', '__')] = flat[::max(1, flat.numel() // 512)].numpy().copy()
    assert all(torch.equal(V[n], v) for n, v in moving.items())
    out['labels'] = np.stack(labels)
    out['image_seeds'] = np.asarray(SEEDS)
    out['losses'] = np.asarray(losses, np.float64)
    out['accuracy'] = np.asarray(accs, np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, 'retinanet_pretrain.npz'), **out)
    with open(os.path.join(OUT, 'retinanet_pretrain_variables.json'), 'w') as f:
        json.dump(variables, f, indent=0, sort_keys=True)
    print('variables', len(variables), 'trainable', sum(v['trainable'] for v in variables.values()), 'losses', losses, 'accuracy', accs,
          'labels', [list(map(int, lab)) for lab in labels], 'test pred', out['test_pred'])
    tf_shim.uninstall()


if __name__ == '__main__':
    main()
