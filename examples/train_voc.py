#!/usr/bin/env python
"""The reference's driver flow (testSSD300.py) on real data: tfrecord shards -> odtk.get_generator -> model -> train_one_epoch -> save_weight.
    python examples/train_voc.py <ssd300|yolov3|retinanet> <directory of .tfrecord files | VOC directory with Annotations/ and JPEGImages/> [epochs]
A VOC directory is converted first (odtk.dataset2tfrecord into <dir>/tfrecords, with the objects' `difficult` flags).  After the last epoch the model is
scored on the same records, un-augmented, with the flags in the ground truth's sixth column: the printed VOC07 mAP follows the PASCAL VOC protocol
(difficult objects are no positives and their detections are not counted).  Shards written without the flags score every object as ordinary.  Needs an MI355X.  No data set ships with the project: this script has been
exercised on shards generated from the fixture pictures of tests/golden/jpeg only (tests/test_gpu_voc_data.py runs the same flow)."""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import odtk                                    # noqa: E402
from odtk.voc_data import get_generator, tf_record_iterator, dataset2tfrecord      # noqa: E402

which, data_dir = sys.argv[1], sys.argv[2]
epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 1
size = {'ssd300': 300, 'yolov3': 416, 'retinanet': 512}[which]
batch_size, buffer_size, lr = 32, 1024, 0.01

tfrecords = sorted(glob.glob(os.path.join(data_dir, '*.tfrecord')))
if not tfrecords:
    tfrecords = dataset2tfrecord(os.path.join(data_dir, 'Annotations'), os.path.join(data_dir, 'JPEGImages'), os.path.join(data_dir, 'tfrecords'), 'voc',
                                 with_difficult=True)
num_train = sum(1 for p in tfrecords for _ in tf_record_iterator(p, verify=False))
batch_size = min(batch_size, num_train)

image_augmentor_config = {                     # testSSD300.py:34-46
    'data_format': 'channels_last', 'output_shape': [size, size], 'crop_method': 'random', 'flip_prob': [0., 0.5], 'fill_mode': 'BILINEAR',
    'keep_aspect_ratios': False, 'constant_values': 0., 'color_jitter_prob': 0.5, 'rotate': [0.5, -5., -5.], 'pad_truth_to': 60,
}
train_gen = get_generator(tfrecords, batch_size, buffer_size, image_augmentor_config)
val_config = {'data_format': 'channels_last', 'output_shape': [size, size], 'fill_mode': 'BILINEAR', 'keep_aspect_ratios': False, 'constant_values': 0.,
              'pad_truth_to': 60}
val_gen = get_generator(tfrecords, 1, 1, val_config, with_difficult=True)          # [1, 60, 6] ground truth: column 5 = difficult
provider = {'data_shape': [size, size, 3], 'num_train': num_train, 'num_val': num_train, 'train_generator': train_gen, 'val_generator': val_gen}
config = {'mode': 'train', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': batch_size,
          'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': './vgg_16.ckpt'}
if which == 'retinanet':
    config.update(is_bottleneck=True, residual_block_list=[3, 4, 6, 3], init_conv_filters=64, init_conv_kernel_size=7, init_conv_strides=2,
                  init_pooling_pool_size=3, init_pooling_strides=2, is_pretraining=False)
model = {'ssd300': odtk.SSD300, 'yolov3': odtk.YOLOv3, 'retinanet': odtk.RetinaNet}[which](config, provider)
for i in range(epochs):
    print('-' * 25, 'epoch', i, '-' * 25)
    print('>> mean loss', model.train_one_epoch(lr))
    model.save_weight('latest', './' + which + '/voc')
r = model.evaluate()
print('>> VOC07 mAP %.4f over %d pictures (%d objects, %d difficult ones not counted)' % (r['mAP'], num_train, r['npos'].sum(), r['num_ignored_gt'].sum()))
