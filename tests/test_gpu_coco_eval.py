"""COCO-style AP on the MI355X: odtk_coco_eval against the NumPy restatement (tests/coco_eval_ref.py) on the hand-worked sets of
tests/test_cpu_coco_eval.py and on random sets up to 500 images x 120 detections with the detection cap biting in every image, bit-identical reruns,
exact answers, the limits, and evaluate(metric='coco') end to end on SSD300 (test mode, and a training model's test-mode copy at batch_size 4).

Comparison rule: match and npos equal, the NaN pattern equal, |AP - ref| <= 1e-12 and the same for recall (f64; 101 terms <= 1, error <= 101 * 2^-53)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import coco_eval_ref as R                 # noqa: E402
import test_cpu_coco_eval as TC           # noqa: E402
import test_gpu_voc_eval as GV            # noqa: E402

_same = TC._same


def _gpu(dets, gts, C, dev, **kw):
    import odtk
    ev = odtk.COCOEvaluator(C, device=dev, **kw)
    for d, g in zip(dets, gts):
        ev.add(list(d), g)
    return ev.result()


@pytest.mark.parametrize('make', TC.HAND, ids=[f.__name__ for f in TC.HAND])
def test_kernel_on_the_hand_worked_sets(dev, make):
    dets, gts, C, kw = make()
    _same(_gpu(dets, gts, C, dev, **kw), R.evaluate(dets, gts, C, **kw))


CASES = dict(TC.EMU_CASES)
CASES['500img-20cls-120det-cap100'] = ((7, 500, 20, 120, 6, 16, 1), dict(max_dets=100))      # one class per image: every image has a segment > 100


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_vs_ref(dev, name):
    (seed, n, C, dpi, gpi, levels, cpi), kw = CASES[name]
    dets, gts = R.random_case(seed, n, C, dpi, gpi, levels, cpi)
    r, ref = _gpu(dets, gts, C, dev, **kw), R.evaluate_fast(dets, gts, C, **kw)
    _same(r, ref)
    assert {0, 1} <= set(np.unique(r['match'][0])) and (r['match'].shape[0] == 1 or (r['match'] == 2).any())
    if 'cap100' in name:
        dropped = (r['match'] == 2).all(axis=(0, 1)).reshape(n, dpi)
        assert dropped.any(axis=1).all()                              # the cap bites in every image


def test_reruns_bit_identical(dev):
    dets, gts = R.random_case(11, 300, 20, 60, 5, 4, 2)
    a, b = _gpu(dets, gts, 20, dev), _gpu(dets, gts, 20, dev)
    assert a['match'].tobytes() == b['match'].tobytes() and a['ap'].tobytes() == b['ap'].tobytes() and a['recall'].tobytes() == b['recall'].tobytes()


def test_exact_answers(dev):
    _, gts = R.random_case(12, 100, 10, 1, 4)
    dets = []
    for g in gts:
        real = g[g[:, 4] >= 0]
        dets.append((np.ones(len(real), np.float32), R.V.gt_corners(real), real[:, 4].astype(np.int32)))
    r = _gpu(dets, gts, 10, dev)
    has = r['npos'][0] > 0
    # every row found by its own box (IoU 1, or an identical duplicate row): all TP in 'all'; precision n / (n + eps) is 1 - O(2^-52)
    assert has.any() and np.all(r['match'][0] == 1) and np.all(np.abs(r['ap'][0][:, has] - 1.0) <= 1e-12) and np.all(r['recall'][0][:, has] == 1.0)
    assert np.all(np.isnan(r['ap'][0][:, ~has])) and abs(r['AP'] - 1.0) <= 1e-12 and abs(r['AP50'] - 1.0) <= 1e-12 and r['AR'] == 1.0
    empty = [(np.zeros(0, np.float32), np.zeros((0, 4), np.float32), np.zeros(0, np.int32)) for _ in gts]
    r = _gpu(empty, gts, 10, dev)
    ok = r['npos'] > 0
    assert np.all(r['ap'][np.broadcast_to(ok[:, None, :], r['ap'].shape)] == 0.0) and np.all(r['recall'][np.broadcast_to(ok[:, None, :], r['ap'].shape)] == 0.0)
    assert r['AP'] == 0.0 and r['AR'] == 0.0 and r['match'].shape == (4, 10, 0)


def test_limits_fail_before_any_launch(dev):
    import odtk
    from odtk import ops
    with pytest.raises(odtk.OdtkError, match='num_thr=65 num_areas=1.*num_thr \\* num_areas <= 64'):
        ops.coco_eval_workspace(4, 1, 1, 2, 65, 1, dev)
    dets, gts, C, _ = TC.hand_worked_ap()
    ev = odtk.COCOEvaluator(1, device=dev)
    ev.add(list(dets[0]), gts[0])
    args, _ = ev._upload()
    ws = ops.coco_eval_workspace(3, 2, 1, 1, 64, 1, dev)

    def outputs(Rn, T):
        return (torch.full((Rn, T, 3), 7, dtype=torch.uint8, device=dev), torch.full((Rn, 1), -5, dtype=torch.int32, device=dev),
                torch.full((Rn, T, 1), -5.0, dtype=torch.float64, device=dev), torch.full((Rn, T, 1), -5.0, dtype=torch.float64, device=dev))
    for thr, rng, max_dets, text in [(np.linspace(0.1, 0.9, 65), [[0, 1e10]], 100, 'num_thr=65 num_areas=1'), ([0.5], [[0, 1e10]], 0, 'max_dets 0')]:
        out = outputs(1, len(thr))
        with pytest.raises(odtk.OdtkError, match=text):
            ops.coco_eval(*args, 1, 1, thr, rng, max_dets, ws, *out)
        torch.cuda.synchronize()
        assert (out[0] == 7).all() and (out[1] == -5).all() and (out[2] == -5).all() and (out[3] == -5).all()      # nothing was launched


# ---------------------------------------------------------------- evaluate(metric='coco') end to end
def _np(rec):
    return [tuple(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in d) for d in rec]


def test_ssd300_evaluate_coco_end_to_end(dev):
    import odtk
    torch.set_num_threads(16)
    p = GV.SR.init_params(3)
    imgs, _ = GV.SR.synthetic_batch(2, 7)
    GV.SR.calibrate_bn(p, imgs, subtract_mean=False)
    val = GV._ssd_val(16)
    m = odtk.SSD300(dict(GV.SSD_CONFIG, compute_dtype='f32'), {'num_val': 16, 'val_generator': val})
    m.load_oracle_params(p)
    rec = GV._recording(m)
    r = m.evaluate(generator=val, metric='coco')
    assert len(rec) == 16 and sum(len(d[0]) for d in rec) > 0
    _same(r, R.evaluate_fast(_np(rec), [g for _, gt in val for g in gt], 20))


def test_train_mode_evaluate_coco_batched_leaves_training_alone(dev, monkeypatch):
    import odtk
    torch.set_num_threads(16)
    train = [tuple(t.numpy() for t in GV.SR.synthetic_batch(4, 900))]
    val = GV._ssd_val(8, seed=400)
    cfg = dict(GV.SSD_CONFIG, mode='train', batch_size=4, compute_dtype='f32')
    a = odtk.SSD300(cfg, {'data_shape': [300, 300, 3], 'num_train': 4, 'num_val': 8, 'train_generator': train, 'val_generator': val})
    a.train_one_epoch(1e-3)
    P, Mom, S, step = a.P.clone(), a.Mom.clone(), a.S.clone(), a.global_step
    rec = []
    orig = odtk.SSD300.test_images

    def recording(self, images):
        out = orig(self, images)
        rec.extend(out)
        return out
    monkeypatch.setattr(odtk.SSD300, 'test_images', recording)
    r = a.evaluate(metric='coco', batch_size=4)
    assert torch.equal(a.P, P) and torch.equal(a.Mom, Mom) and torch.equal(a.S, S) and a.global_step == step
    assert len(rec) == 8 and a._eval_models[4].mode == 'test' and r['num_detections'].sum() > 0
    _same(r, R.evaluate_fast(_np(rec), [g for _, gt in val for g in gt], 20))
