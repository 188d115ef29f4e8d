"""GPU tier of odtk.voc_data: tfrecord shards -> get_generator -> batches on the device, and a model trained from them."""
import numpy as np
import pytest
import torch

import jpeg_cases as JC

pytestmark = pytest.mark.gpu

SSD_STYLE = {'data_format': 'channels_last', 'output_shape': [64, 64], 'crop_method': 'random', 'flip_prob': [0., 0.5], 'fill_mode': 'BILINEAR',
             'keep_aspect_ratios': False, 'constant_values': 0., 'color_jitter_prob': 0.5, 'rotate': [0.5, -5., -5.], 'pad_truth_to': 60}
RESIZE_ONLY = {'data_format': 'channels_last', 'output_shape': [64, 64], 'fill_mode': 'BILINEAR', 'keep_aspect_ratios': False, 'constant_values': 0.,
               'pad_truth_to': 60}


def test_three_batches_with_the_ssd_style_config(dev, tmp_path):
    from odtk.voc_data import get_generator
    paths, _ = JC.write_fixture_shards(tmp_path)
    gen = get_generator(paths, 4, 8, SSD_STYLE, device=dev, seed=3)
    it = iter(gen)
    for _ in range(3):
        img, gt = next(it)
        assert img.shape == (4, 64, 64, 3) and img.dtype == torch.float32 and img.device.type == 'cuda' and bool(torch.isfinite(img).all())
        assert gt.shape == (4, 60, 5) and gt.dtype == torch.float32 and bool(torch.isfinite(gt).all())
        g = gt.cpu().numpy()
        pad = (g == -1).all(-1)
        ok = (g[..., 4] >= 0) & (g[..., 4] <= 19) & (g[..., 2] > 0) & (g[..., 3] > 0)
        assert (pad | ok).all() and (~pad).any()
    it.close()
    assert not it._thread.is_alive()


def test_resize_only_equals_the_augmentor_on_pil_pictures(dev, tmp_path):
    """buffer_size 1 keeps file order; with a config that only resizes every output pixel is a convex combination of decoded pixels, so each picture's
    decode bound carries over unscaled (1 grayscale, 3 for 4:4:4, 5 subsampled: jpeg_cases.max_bound; 1e-3 for the float32 interpolation); the ground
    truth does not depend on the pixels and is exact"""
    from odtk.augment import Augmentor
    from odtk.voc_data import get_generator
    paths, records = JC.write_fixture_shards(tmp_path)
    it = iter(get_generator(paths, 4, 1, RESIZE_ONLY, device=dev, seed=0))
    aug = Augmentor(**RESIZE_ONLY)
    for b in range(3):
        img, gt = next(it)
        recs = records[4 * b: 4 * b + 4]
        ref_img, ref_gt = aug([torch.from_numpy(JC.fixture_rgb(n)).to(dev) for n, _ in recs], [torch.from_numpy(g) for _, g in recs])
        for k, (name, _) in enumerate(recs):
            d = float((img[k] - ref_img[k]).abs().max())
            print(f'batch {b} picture {k} ({name}): max |diff| against the augmentor on the PIL picture {d:.3f} (bound {JC.max_bound(name)})')
            assert d <= JC.max_bound(name) + 1e-3, (name, d)
        assert torch.equal(gt, ref_gt)
    it.close()


def test_ssd300_trains_two_steps_from_the_generator(dev, tmp_path):
    import odtk
    from odtk.voc_data import get_generator
    paths, _ = JC.write_fixture_shards(tmp_path)
    cfg = dict(SSD_STYLE, output_shape=[300, 300])
    gen = get_generator(paths, 2, 8, cfg, device=dev, seed=1)
    prov = {'data_shape': [300, 300, 3], 'num_train': 4, 'num_val': 0, 'train_generator': gen, 'val_generator': None}
    m = odtk.SSD300({'mode': 'train', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 2,
                     'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': './vgg_16.ckpt', 'verbose': False}, prov)
    loss = m.train_one_epoch(0.001)
    assert m.global_step == 2 and np.isfinite(float(loss))


def test_generator_serves_as_val_generator_for_evaluate(dev, tmp_path):
    """the same object with a config that has no random part, as data_provider['val_generator']: evaluate() reads num_val pictures from it and ends"""
    import odtk
    from odtk.voc_data import get_generator
    paths, records = JC.write_fixture_shards(tmp_path)
    val = get_generator(paths, 2, 1, dict(RESIZE_ONLY, output_shape=[300, 300]), device=dev, seed=0)
    m = odtk.SSD300({'mode': 'test', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 1,
                     'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': './vgg_16.ckpt', 'verbose': False},
                    {'num_val': 4, 'val_generator': val})
    r = m.evaluate()
    assert np.isfinite(r['mAP']) and int(r['npos'].sum()) == sum(len(g) for _, g in records[:4])
    r2 = odtk.evaluate(m, val, num_images=3)
    assert np.isfinite(r2['mAP']) and int(r2['npos'].sum()) == sum(len(g) for _, g in records[:3])
    with pytest.raises(ValueError, match='repeats without end'):
        odtk.evaluate(m, val)
