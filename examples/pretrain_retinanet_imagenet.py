#!/usr/bin/env python
"""The reference's two-stage RetinaNet workflow fed from ImageNet-style records, with held-out accuracy after every epoch:
    1. a directory with one sub-directory per class is converted to `.tfrecord` shards (odtk.imagenet_dataset2tfrecord; files the baseline JPEG decoder
       refuses -- progressive, CMYK -- are left out with one warning), or existing shards are taken as they are; the LAST shard is held out;
    2. classification pre-training of the backbone (`is_pretraining: True`) from odtk.get_imagenet_generator; after every epoch evaluate() measures
       top-1 / top-5 / loss on the held-out shard and save_weight('best') keeps the weights whenever top-1 improves;
    3. a detection model (`is_pretraining: False`) is started from the best backbone with load_pretraining_weight.
Needs an MI355X:   python examples/pretrain_retinanet_imagenet.py <image-dir | tfrecords...> [epochs]

The pre-training graph has 224 logits (the channels of the backbone's last unit: no dense layer), so class ids must lie in [0, 224): a directory of up
to 224 class folders works with the default mapping (sorted names -> 0 .. K-1); give dataset2tfrecord a classname_to_ids mapping for anything else.
evaluate() runs the training-mode forward pass (BATCH statistics) without any update: the reference's pre-training never updates the moving statistics,
so a test-mode pass would classify at chance (RetinaNet._evaluate_pretraining)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import odtk                                   # noqa: E402
from odtk.voc_data import tf_record_iterator  # noqa: E402

args = sys.argv[1:]
epochs = int(args.pop()) if len(args) > 1 and args[-1].isdigit() else 3
if not args:
    sys.exit(__doc__)
out_dir = os.path.join('weights', 'retinanet_pretrain_imagenet')
if len(args) == 1 and os.path.isdir(args[0]):
    shards = odtk.imagenet_dataset2tfrecord(args[0], os.path.join(out_dir, 'records'), 'train', total_shards=8, seed=0, on_unsupported='skip')
else:
    shards = args
assert len(shards) >= 2, 'at least two shards: the last one is held out'
train_shards, val_shards = shards[:-1], shards[-1:]
size, batch_size = 128, 16
num_train = sum(1 for s in train_shards for _ in tf_record_iterator(s, verify=False))
num_val = sum(1 for s in val_shards for _ in tf_record_iterator(s, verify=False))
print(f'{num_train} training records in {len(train_shards)} shard(s), {num_val} held out')

augment = {'data_format': 'channels_last', 'output_shape': [size, size], 'crop_method': 'random', 'flip_prob': [0., 0.5], 'fill_mode': 'BILINEAR',
           'keep_aspect_ratios': False, 'constant_values': 0., 'color_jitter_prob': 0.5}
resize = {'data_format': 'channels_last', 'output_shape': [size, size], 'fill_mode': 'BILINEAR', 'keep_aspect_ratios': False, 'constant_values': 0.}
provider = {'num_train': num_train, 'num_val': num_val,
            'train_generator': odtk.get_imagenet_generator(train_shards, batch_size, 1024, augment, seed=0, on_unsupported='skip'),
            'val_generator': odtk.get_imagenet_generator(val_shards, batch_size, 1, resize, seed=0, on_unsupported='skip')}
base = {'is_bottleneck': True, 'residual_block_list': [3, 4, 6, 3], 'init_conv_filters': 16, 'mode': 'train', 'data_shape': [size, size, 3],
        'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'data_format': 'channels_last', 'batch_size': batch_size, 'gamma': 2.0,
        'alpha': 0.25, 'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.45, 'verbose': False}

pre = odtk.RetinaNet(dict(base, is_pretraining=True), provider)
best, best_ckpt = -1.0, None
for epoch in range(epochs):
    loss, acc = pre.train_one_epoch(0.01)
    val = pre.evaluate()                                          # val_generator, num_val rounded down to whole batches, batch statistics
    print(f"epoch {epoch}: loss {loss:.4f}  accuracy {acc:.3f} | held out ({val['num_images']} pictures): top-1 {val['top1']:.3f}  "
          f"top-{val['top_k']} {val['topk']:.3f}  loss {val['loss']:.4f}")
    pre.save_weight('latest', os.path.join(out_dir, 'latest', 'backbone'))
    if val['top1'] > best:
        best = val['top1']
        pre.save_weight('best', os.path.join(out_dir, 'best', 'backbone'))
        best_ckpt = os.path.join(out_dir, 'best', f'backbone-{pre.global_step}')
print(f'best held-out top-1 {best:.3f}: {best_ckpt}')

rng = np.random.default_rng(0)
imgs = rng.uniform(0, 255, (batch_size, size, size, 3)).astype(np.float32)
gt = np.full((batch_size, 10, 5), -1.0, np.float32)
gt[:, 0] = [size / 2, size / 2, size / 3, size / 3, 0]
det = odtk.RetinaNet(dict(base, is_pretraining=False), {'num_train': batch_size, 'num_val': 0, 'train_generator': [(imgs, gt)], 'val_generator': None})
det.load_pretraining_weight(best_ckpt)
print('detection epoch from the pre-trained backbone: loss', float(det.train_one_epoch(1e-3)))
