#!/usr/bin/env python
"""The reference's two-stage RetinaNet workflow (RetinaNet.py:61-76, :537-539) on synthetic pictures:
    1. classification pre-training of the backbone (`is_pretraining: True`): train_one_epoch -> (mean loss, mean accuracy), save_weight
       (the 260 trainable tensors of 'feature_extractor'), test_one_image -> the predicted class;
    2. a detection model (`is_pretraining: False`) started from that backbone with load_pretraining_weight, then train_one_epoch.
Needs an MI355X:   python examples/pretrain_retinanet_synthetic.py [epochs] [out_dir]

The provider contract of the pre-training graph is that of utils/tfrecord_imagenet_utils.py: an iterable of (images [N, H, W, 3], labels [N])
batches, labels int in [0, 224) -- the 224 logits are the channels of the backbone's last unit (4 * 56: no dense layer, num_classes is not used).
The moving statistics of the batch norms are not updated by pre-training (the reference's pre-training train_op has no UPDATE_OPS
dependency): they stay 0 / 1, and the detection model keeps its own when it loads the backbone.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import odtk                                   # noqa: E402

epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join('weights', 'retinanet_pretrain')
size, batch_size, classes = 128, 16, 8            # the first 8 of the 224 classes are used
rng = np.random.default_rng(0)
tints = rng.uniform(40, 215, (classes, 3))

base = {'is_bottleneck': True, 'residual_block_list': [3, 4, 6, 3], 'init_conv_filters': 16, 'mode': 'train', 'data_shape': [size, size, 3],
        'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'data_format': 'channels_last', 'batch_size': batch_size, 'gamma': 2.0,
        'alpha': 0.25, 'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.45, 'verbose': False}


def labelled_batches(n):
    """pictures whose class is their tint, plus noise"""
    out = []
    for _ in range(n):
        labels = rng.integers(0, classes, batch_size)
        imgs = np.clip(tints[labels][:, None, None, :] + rng.normal(0, 30, (batch_size, size, size, 3)), 0, 255).astype(np.float32)
        out.append((imgs, labels))
    return out


def detection_batches(n):
    """[yc, xc, h, w, class] boxes padded with -1 rows: the detection provider contract"""
    out = []
    for _ in range(n):
        imgs = rng.uniform(0, 255, (batch_size, size, size, 3)).astype(np.float32)
        gt = np.full((batch_size, 10, 5), -1.0, np.float32)
        for i in range(batch_size):
            k = int(rng.integers(1, 4))
            h, w = rng.uniform(20, 100, k), rng.uniform(20, 100, k)
            gt[i, :k] = np.stack([h / 2 + rng.uniform(0, 1, k) * (size - h), w / 2 + rng.uniform(0, 1, k) * (size - w), h, w, rng.integers(0, 20, k)], 1)
        out.append((imgs, gt))
    return out


train = labelled_batches(4)
pre = odtk.RetinaNet(dict(base, is_pretraining=True), {'num_train': 4 * batch_size, 'num_val': 0, 'train_generator': train, 'val_generator': None})
for epoch in range(epochs):
    loss, acc = pre.train_one_epoch(0.01)
    print(f'pre-training epoch {epoch}: loss {loss:.4f}  accuracy {acc:.3f}')
pre.save_weight('latest', os.path.join(out_dir, 'backbone'))
ckpt = os.path.join(out_dir, f'backbone-{pre.global_step}')

test = odtk.RetinaNet(dict(base, is_pretraining=True, mode='test'), None)
test.load_weight(ckpt)
img, label = train[0][0][:1], train[0][1][0]
print('test_one_image: predicted class', int(test.test_one_image(img)[0]), 'label', int(label))

det = odtk.RetinaNet(dict(base, is_pretraining=False), {'num_train': 2 * batch_size, 'num_val': 0, 'train_generator': detection_batches(2),
                                                         'val_generator': None})
det.load_pretraining_weight(ckpt)
print('detection epoch from the pre-trained backbone: loss', float(det.train_one_epoch(1e-3)))
