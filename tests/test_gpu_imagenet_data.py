"""GPU tier of odtk.imagenet_data and of the pre-training graph's evaluate() / test_images(): class folders of fixture pictures -> dataset2tfrecord ->
get_generator -> batches on the device; a pre-training RetinaNet trained from them and evaluated with batch statistics."""
import os
import shutil

import numpy as np
import pytest
import torch

import classify_cases as CC
import jpeg_cases as JC
import test_gpu_retinanet_pretraining as G

pytestmark = pytest.mark.gpu

RESIZE_ONLY = {'data_format': 'channels_last', 'output_shape': [64, 64], 'fill_mode': 'BILINEAR', 'keep_aspect_ratios': False, 'constant_values': 0.}


def _shards(tmp_path, per_class=1, shards=3, seed=2):
    """one class folder per decodable fixture (label k <-> JC.DECODABLE[k]: a distinct picture per class) -> shards"""
    from odtk.imagenet_data import dataset2tfrecord
    root = tmp_path / 'img'
    for k, name in enumerate(JC.DECODABLE):
        os.makedirs(root / f'n{k:02d}')
        for j in range(per_class):
            shutil.copy(os.path.join(JC.GOLDEN, name + '.jpg'), root / f'n{k:02d}' / f'{j}.jpg')
    return dataset2tfrecord(str(root), str(tmp_path / 'rec'), 'fixtures', total_shards=shards, seed=seed)


def test_generator_end_to_end_pictures_and_labels(dev, tmp_path):
    """every picture is the augmentor's output on PIL's decode of the fixture its LABEL names, to the decode bounds of jpeg_cases.py (a config that only
    resizes: each output pixel is a convex combination of decoded pixels; 1e-3 for the float32 interpolation)"""
    from odtk.augment import Augmentor
    from odtk.imagenet_data import get_generator
    paths = _shards(tmp_path)
    n = len(JC.DECODABLE)
    gen = get_generator(paths, 4, 5, RESIZE_ONLY, device=dev, seed=3)
    aug = Augmentor(**RESIZE_ONLY)
    it = iter(gen)
    seen = []
    for b in range(n // 4):                                      # one pass
        img, labels = next(it)
        assert img.shape == (4, 64, 64, 3) and img.dtype == torch.float32 and img.device.type == 'cuda'
        assert labels.dtype == torch.int64 and labels.device.type == 'cpu' and tuple(labels.shape) == (4,)
        names = [JC.DECODABLE[int(v)] for v in labels]
        ref = aug([torch.from_numpy(JC.fixture_rgb(nm)).to(dev) for nm in names], None)
        for k, nm in enumerate(names):
            d = float((img[k] - ref[k]).abs().max())
            print(f'batch {b} picture {k} ({nm}, label {int(labels[k])}): max |diff| {d:.3f} (bound {JC.max_bound(nm)})')
            assert d <= JC.max_bound(nm) + 1e-3, (nm, d)
        seen += labels.tolist()
    it.close()
    assert not it._thread.is_alive() and len(set(seen)) == len(seen) == n // 4 * 4 and gen.skipped == 0


class Tap:
    """`batches` batches of a generator; after each one has been evaluated (the consumer asks for the next) the model's own buffers are recorded"""

    def __init__(self, gen, model, batches):
        self.gen, self.m, self.batches, self.rec = gen, model, batches, []

    def __iter__(self):
        it = iter(self.gen)
        try:
            for _ in range(self.batches):
                yield next(it)
                torch.cuda.synchronize()
                m = self.m
                self.rec.append(tuple(t.detach().cpu().clone() for t in (m.pred, m.labels, m.ce, m.logits)))
        finally:
            it.close()


def test_pretraining_trains_from_the_generator_and_evaluates(dev, tmp_path):
    from odtk.imagenet_data import get_generator
    paths = _shards(tmp_path, per_class=3, shards=2)
    cfg = dict(RESIZE_ONLY, output_shape=[128, 128])
    train = get_generator(paths[:1], 4, 8, dict(cfg, flip_prob=[0., 0.5]), device=dev, seed=1)
    val = get_generator(paths[1:], 4, 1, cfg, device=dev, seed=0)
    m = G._model(provider={'num_train': 8, 'num_val': 12, 'train_generator': train, 'val_generator': val})
    loss, acc = m.train_one_epoch(0.01)
    assert m.global_step == 2 and np.isfinite(loss) and 0.0 <= acc <= 1.0
    torch.cuda.synchronize()
    before = (m.P.clone(), m.Mom.clone(), m.S.clone(), m.global_step)
    tap = Tap(val, m, 3)
    r = m.evaluate(generator=tap)                                # a finite generator: one pass of 3 batches
    torch.cuda.synchronize()
    assert torch.equal(m.P, before[0]) and torch.equal(m.Mom, before[1]) and torch.equal(m.S, before[2]) and m.global_step == before[3]
    assert len(tap.rec) == 3 and r['num_images'] == 12 and r['invalid_labels'] == 0
    pred = torch.cat([t[0] for t in tap.rec]).numpy()
    labels = torch.cat([t[1] for t in tap.rec]).numpy()
    ce = torch.cat([t[2] for t in tap.rec]).numpy().astype(np.float64)
    logits = torch.cat([t[3] for t in tap.rec]).numpy()
    assert r['top1'] == float((pred == labels).mean()) and r['top1'] <= r['topk']
    ref = CC.reference(logits, logits.shape[1], labels, 5)       # float64 on the model's own logits: both f32 losses are within bound(n) of it
    print(f"evaluate: loss {r['loss']:.9f}, mean of the head's ce {ce.mean():.9f}, |diff| {abs(r['loss'] - ce.mean()):.3e}, bound {2 * ref['bound'].mean():.3e}")
    assert abs(r['loss'] - ce.mean()) <= 2 * ref['bound'].mean()
    assert abs(r['loss'] - ref['loss'].mean()) <= ref['bound'].mean()
    assert r['topk'] == ref['totals'][2] / 12 and np.array_equal(r['class_seen'], ref['seen'])
    r2 = m.evaluate(generator=Tap(val, m, 3))                    # the validation stream restarts: the same pictures, the same bits
    assert r2['loss'] == r['loss'] and r2['top1'] == r['top1'] and r2['topk'] == r['topk'] and np.array_equal(r2['class_seen'], r['class_seen'])
    assert np.array_equal(r2['class_accuracy'], r['class_accuracy'], equal_nan=True)
    r3 = m.evaluate()                                            # the provider's val_generator and num_val = 12
    assert r3['num_images'] == 12 and r3['loss'] == r['loss']
    with pytest.raises(ValueError, match='repeats without end'):
        m.evaluate(generator=val)


def test_test_images_equals_the_batch_1_model(dev):
    g = torch.Generator().manual_seed(12)
    imgs = (torch.rand(3, 128, 128, 3, generator=g) * 255).round()
    m3 = G._model(mode='test', test_batch_size=3)
    m1 = G._model(mode='test')
    m1.load_oracle_params(m3.export_params())
    batched = m3.test_images(imgs.numpy())
    assert batched.dtype == np.int64 and batched.shape == (3,)
    singles = np.concatenate([m1.test_one_image(imgs[k: k + 1].numpy()) for k in range(3)])
    assert np.array_equal(batched, singles), (batched, singles)
    one = m3.test_one_image(imgs[1:2].numpy())
    assert one.shape == (1,) and one[0] == batched[1]
    assert np.array_equal(m3.test_images(imgs[1:].numpy()), batched[1:])
    with pytest.raises(ValueError, match='moving statistics'):
        m3.evaluate(generator=[(imgs, torch.zeros(3, dtype=torch.int64))])
