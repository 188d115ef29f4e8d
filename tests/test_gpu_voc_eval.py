"""VOC mAP on the MI355X: csrc/voc_eval.hip against the NumPy restatement (tests/voc_eval_ref.py) from one image to 100 000 images and a class of
2 M detections (the multi-block radix sort), bit-identical reruns, exact answers, the capacity limits, and evaluate() end to end on SSD300 and
YOLOv3 (test mode) and on a training SSD300 (its test-mode copy; the training state left as it was)."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import voc_eval_ref as R                  # noqa: E402
from oracle import ssd300_ref as SR       # noqa: E402


def _case(seed, n_img, C, det_per_img, gt_per_img, levels=16, one_class=None):
    """vectorised synthetic set: per image `gt_per_img` GT rows (+1 padding row), `det_per_img` detections, 70 % of them jittered GT boxes;
    scores quantised to `levels` values (heavy ties).  one_class: every detection and GT row of that class"""
    rng = np.random.default_rng(seed)
    G = n_img * gt_per_img
    yc, xc = rng.uniform(20, 280, G), rng.uniform(20, 280, G)
    h, w = rng.uniform(8, 80, G), rng.uniform(8, 80, G)
    gcls = rng.integers(0, C, G) if one_class is None else np.full(G, one_class)
    gt = np.stack([yc, xc, h, w, gcls], 1).astype(np.float32).reshape(n_img, gt_per_img, 5)
    gt = np.concatenate([gt, -np.ones((n_img, 1, 5), np.float32)], 1)
    D = n_img * det_per_img
    img = np.repeat(np.arange(n_img), det_per_img)
    j = img * gt_per_img + rng.integers(0, gt_per_img, D)
    hit = rng.random(D) < 0.7
    y1 = np.where(hit, yc[j] - h[j] / 2, rng.uniform(0, 260, D))
    x1 = np.where(hit, xc[j] - w[j] / 2, rng.uniform(0, 260, D))
    y2 = np.where(hit, yc[j] + h[j] / 2, y1 + rng.uniform(5, 60, D))
    x2 = np.where(hit, xc[j] + w[j] / 2, x1 + rng.uniform(5, 60, D))
    box = np.stack([y1, x1, y2, x2], 1) + hit[:, None] * rng.normal(0, 0.15, (D, 4)) * np.stack([h[j], w[j], h[j], w[j]], 1)
    dcls = np.where(hit & (rng.random(D) < 0.8), gcls[j], rng.integers(0, C, D)) if one_class is None else np.full(D, one_class)
    score = rng.integers(1, levels + 1, D) / levels
    sc = np.split(score.astype(np.float32), n_img)
    bx = np.split(box.astype(np.float32), n_img)
    cl = np.split(dcls.astype(np.int32), n_img)
    return list(zip(sc, bx, cl)), list(gt)


def _gpu(dets, gts, C, metric, dev):
    import odtk
    ev = odtk.VOCEvaluator(C, 0.5, metric, device=dev)
    for d, g in zip(dets, gts):
        ev.add(list(d), g)
    return ev.result()


def _check(r, ref):
    assert np.array_equal(r['tp'], ref['tp'])
    assert r['npos'].tolist() == ref['npos'].tolist()
    assert r['num_detections'].tolist() == ref['num_detections'].tolist()
    assert np.array_equal(np.isnan(r['AP']), np.isnan(ref['AP']))
    ok = ~np.isnan(ref['AP'])
    assert np.max(np.abs(r['AP'][ok] - ref['AP'][ok]), initial=0.0) <= 1e-12, np.max(np.abs(r['AP'][ok] - ref['AP'][ok]))


CASES = [  # seed, images, classes, detections / image, GT / image, score levels, one class
    (0, 1, 3, 40, 5, 4, None),
    (1, 64, 20, 30, 3, 8, None),
    (2, 4952, 20, 100, 3, 16, None),          # VOC07-test sized
    (3, 20000, 1000, 12, 2, 1000, None),      # many classes
    (4, 100000, 1, 21, 2, 64, 0),             # one class of 2.1 M detections: the multi-block radix passes
]


@pytest.mark.parametrize('case', CASES, ids=[f'{c[1]}img-{c[2]}cls' for c in CASES])
def test_kernel_vs_ref(dev, case):
    seed, n, C, dpi, gpi, levels, one = case
    dets, gts = _case(seed, n, C, dpi, gpi, levels, one)
    for metric in ('voc07', 'area'):
        ref = R.evaluate_fast(dets, gts, C, metric=metric)
        r = _gpu(dets, gts, C, metric, dev)
        _check(r, ref)
        if one is not None:
            assert r['num_detections'][one] >= 2_000_000 and r['tp'].sum() > 0


def test_reruns_bit_identical(dev):
    dets, gts = _case(5, 3000, 20, 60, 3, 4)
    for metric in ('voc07', 'area'):
        a, b = _gpu(dets, gts, 20, metric, dev), _gpu(dets, gts, 20, metric, dev)
        assert np.array_equal(a['tp'], b['tp']) and a['AP'].tobytes() == b['AP'].tobytes()


def test_exact_answers(dev):
    _, gts = _case(6, 200, 10, 1, 3)
    dets = []
    for g in gts:
        real = g[g[:, 4] >= 0]
        corners = R.gt_corners(real)
        dets.append((np.ones(len(real), np.float32), corners, real[:, 4].astype(np.int32)))
    empty = [(np.zeros(0, np.float32), np.zeros((0, 4), np.float32), np.zeros(0, np.int32)) for _ in gts]
    for metric in ('voc07', 'area'):
        r = _gpu(dets, gts, 10, metric, dev)
        has = r['npos'] > 0
        assert has.any() and np.all(np.abs(r['AP'][has] - 1.0) <= 1e-15) and np.all(np.isnan(r['AP'][~has])) and np.all(r['tp'] == 1)
        r = _gpu(empty, gts, 10, metric, dev)
        assert np.all(r['AP'][has] == 0.0) and r['mAP'] == 0.0


def test_capacity_limit_errors(dev):
    import odtk
    from odtk import ops
    assert ops.voc_eval_workspace(0, 0, 1, 1024, dev).numel() > 0
    for args, text in [(((8 << 20) + 1, 0, 1, 20), 'num_det=8388609'), ((0, (2 << 20) + 1, 1, 20), 'num_gt=2097153'),
                       ((0, 0, (1 << 20) + 1, 20), 'num_images=1048577'), ((0, 0, 1, 1025), 'num_classes=1025')]:
        with pytest.raises(odtk.OdtkError, match=text + '.*outside the supported range'):
            ops.voc_eval_workspace(*args, dev)
    ev = odtk.VOCEvaluator(20, device=dev)
    ev.add([np.zeros(1, np.float32), np.zeros((1, 4), np.float32), np.zeros(1, np.int32)], np.zeros((0, 5), np.float32))
    ev.num_classes = 2000                                          # past the constructor's check: the library's own
    with pytest.raises(odtk.OdtkError, match='num_classes=2000'):
        ev.result()


# ---------------------------------------------------------------- evaluate() end to end
SSD_CONFIG = {
    'mode': 'test', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 1,
    'nms_score_threshold': 0.01, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': '', 'verbose': False,
}


def _ssd_val(n_images, B=4, seed=300):
    return [tuple(t.numpy() for t in SR.synthetic_batch(B, seed + i)) for i in range(n_images // B)]


def _recording(m):
    rec = []
    orig = m.test_one_image

    def f(images):
        out = orig(images)
        rec.append(out)
        return out
    m.test_one_image = f
    return rec


def test_ssd300_evaluate_end_to_end(dev):
    import odtk
    torch.set_num_threads(16)
    p = SR.init_params(3)
    imgs, _ = SR.synthetic_batch(2, 7)
    SR.calibrate_bn(p, imgs, subtract_mean=False)
    val = _ssd_val(64)
    m = odtk.SSD300(dict(SSD_CONFIG, compute_dtype='f32'), {'num_val': 64, 'val_generator': val})
    m.load_oracle_params(p)
    rec = _recording(m)
    for metric in ('voc07', 'area'):
        rec.clear()
        r = m.evaluate(generator=val, metric=metric)
        assert len(rec) == 64 and sum(len(d[0]) for d in rec) > 0
        _check(r, R.evaluate_fast(rec, [g for _, gt in val for g in gt], 20, metric=metric))
    rec.clear()
    r2 = odtk.evaluate(m, val, num_images=10)                       # the free function, stopped inside a batch
    assert len(rec) == 10
    _check(r2, R.evaluate_fast(rec, [g for _, gt in val for g in gt][:10], 20))


def test_yolov3_evaluate_end_to_end(dev):
    import odtk
    from oracle import yolov3_net_ref as NR
    from oracle import yolov3_ref as YR
    torch.set_num_threads(16)
    size = 416
    p = NR.init_params(8)
    g = torch.Generator().manual_seed(1)
    imgs = (torch.rand(2, size, size, 3, generator=g) * 255).round()
    stats = {}
    with torch.no_grad():
        NR.forward(p, imgs, True, stats, subtract_mean=False)
    for k, (mean, var) in stats.items():
        p[k + '.mmean'], p[k + '.mvar'] = mean.clone(), var.clone()
    val = []
    for i in range(8):
        gi = torch.Generator().manual_seed(50 + i)
        val.append((((torch.rand(4, size, size, 3, generator=gi) * 255).round()).numpy(), YR.synthetic_gt(4, size, 70 + i, max_obj=3).numpy()))
    cfg = {'mode': 'test', 'data_shape': [size, size, 3], 'num_classes': 20, 'weight_decay': 5e-4, 'keep_prob': 0.5, 'data_format': 'channels_last',
           'batch_size': 1, 'coord_scale': 1, 'noobj_scale': 1, 'obj_scale': 5., 'class_scale': 1., 'num_priors': 3, 'nms_score_threshold': 0.01,
           'nms_max_boxes': 10, 'nms_iou_threshold': 0.5, 'priors': YR.PRIORS_PX, 'verbose': False, 'compute_dtype': 'f32'}
    m = odtk.YOLOv3(cfg, {'num_val': 32, 'val_generator': val})
    m.load_oracle_params(p)
    rec = _recording(m)
    r = m.evaluate(generator=val)
    assert len(rec) == 32 and sum(len(d[0]) for d in rec) > 0
    _check(r, R.evaluate_fast(rec, [g for _, gt in val for g in gt], 20))


def test_train_mode_evaluate_uses_a_copy_and_leaves_training_alone(dev, tmp_path):
    import odtk
    torch.set_num_threads(16)
    train = [tuple(t.numpy() for t in SR.synthetic_batch(4, 900 + i)) for i in range(2)]
    val = _ssd_val(16, seed=400)
    cfg = dict(SSD_CONFIG, mode='train', batch_size=4, compute_dtype='f32')
    prov = {'data_shape': [300, 300, 3], 'num_train': 8, 'num_val': 16, 'train_generator': train, 'val_generator': val}
    a = odtk.SSD300(cfg, prov)
    b = odtk.SSD300(cfg, prov)
    a.train_one_epoch(1e-3)
    b.train_one_epoch(1e-3)
    P, Mom, S, step = a.P.clone(), a.Mom.clone(), a.S.clone(), a.global_step
    r = a.evaluate()
    assert torch.equal(a.P, P) and torch.equal(a.Mom, Mom) and torch.equal(a.S, S) and a.global_step == step
    assert a._eval_model.mode == 'test' and a._eval_model.DT == odtk.F32
    a.save_weight('best', str(tmp_path / 'ssd'))
    t = odtk.SSD300(dict(SSD_CONFIG, compute_dtype='f32'), prov)
    t.load_weight(str(tmp_path / f'ssd-{step}'))
    r_t = odtk.evaluate(t, val)
    assert np.array_equal(r['tp'], r_t['tp']) and r['AP'].tobytes() == r_t['AP'].tobytes()
    assert r['num_detections'].sum() > 0
    # the next epoch of the evaluated model returns the loss of the one that never evaluated, bit for bit
    la, lb = a.train_one_epoch(1e-3), b.train_one_epoch(1e-3)
    assert la == lb
    assert torch.equal(a.P, b.P)
    # a second evaluation reuses the copy with the new weights
    m0 = a._eval_model
    a.evaluate(num_images=4)
    assert a._eval_model is m0
