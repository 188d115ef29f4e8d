"""GPU: soft-NMS.  Kernel level through the C-ABI (bodies in tests/soft_nms_cases.py, shared with the CPU tier): `hard` against odtk_nms_image_class, `linear`
bit for bit and `gaussian` within the derived bound against the float32 oracle, refusals, odtk_detection_pack_scored.  Model level: SSD300's batched tail with
nms_method 'linear' / 'gaussian' against the oracle on the tail's own operands, 'hard' == no key, YOLOv2 (the per-class fallback tail), evaluate() on a
train-mode model."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import soft_nms_cases as SC              # noqa: E402
from oracle import ssd300_ref as R       # noqa: E402


# ---------------------------------------------------------------- kernel level
@pytest.mark.parametrize('with_n_dev', [False, True])
@pytest.mark.parametrize('n', sorted(SC.HARD_SHAPES))
def test_hard_equals_nms_image_class(n, with_n_dev, dev):
    cnt = SC.check_hard(dev, n, with_n_dev)
    print(f'n={n} n_dev={with_n_dev}: picks per (image, class)\n{cnt}')


@pytest.mark.parametrize('n', [65, 1025])
def test_linear_equals_the_oracle_bit_for_bit(n, dev):
    print(SC.check_linear(dev, n))


@pytest.mark.parametrize('n,sigma', sorted(SC.GAUSS_SEEDS))
def test_gaussian_within_the_derived_bound(n, sigma, dev):
    SC.check_gaussian(dev, n, sigma)


def test_two_runs_give_identical_bytes(dev):
    boxes, scores, valid = SC.gauss_case(1025, 0.5, 3)
    a, b = (SC.Launch(dev, boxes, scores, valid, 3, 20, 20, 2, 0.5, 0.5, 0.1).tables() for _ in range(2))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_refusals(dev):
    assert SC.check_refusals(dev) == 14


def test_detection_pack_scored(dev):
    SC.check_pack_scored(dev)


# ---------------------------------------------------------------- model level: SSD300
@pytest.fixture(scope='module')
def ssd_case():
    import test_gpu_batched_inference as TB
    torch.set_num_threads(16)
    p = R.init_params(3)
    imgs, _ = R.synthetic_batch(4, 7)
    R.calibrate_bn(p, imgs[:2], subtract_mean=False)           # (the weights of test_gpu_batched_inference.ssd300_case)
    models = {}

    def model(**kw):
        import odtk
        key = tuple(sorted(kw.items()))
        if key not in models:
            models[key] = odtk.SSD300(dict(TB.SSD_CONFIG, test_batch_size=3, **kw), None)
            models[key].load_oracle_params(p)
        return models[key]
    return TB, imgs[:3], model


def _tail_reference(m, n_images, method):
    t = m._tail_batched
    conf, boxes, cand = t.conf.cpu().numpy(), t.boxes.cpu().numpy(), t.cand.view(torch.uint8).cpu().numpy()
    return [SC.tail_reference(conf[n], boxes[n], cand[n], m.nms_max_boxes, {'linear': 1, 'gaussian': 2}[method], m.nms_iou_threshold, m.soft_nms_sigma,
                              m.soft_nms_min_score) for n in range(n_images)]


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_ssd300_soft_nms_against_the_oracle_on_the_tails_operands(method, ssd_case, dev):
    TB, imgs, model = ssd_case
    # the candidates' threshold is the configuration's 0.5, where most classes stay below nms_max_boxes: decayed rows are picked and stay in play down to 0.125
    # (at 0.3 and below every class fills its 20 slots with undecayed rows and 'linear' returns what 'hard' returns)
    m, hard = model(nms_method=method, soft_nms_min_score=0.125), model()
    assert m.nms_method == method and m._nms_params()['min_score'] == 0.125 and m.nms_score_threshold == 0.5
    x = imgs.numpy()
    differs = 0
    for n_images in (3, 2):
        got = m.test_images(x[:n_images])
        assert m._tail_batched.method == {'linear': 1, 'gaussian': 2}[method] and m._tail_batched.out_score is not None
        want = _tail_reference(m, n_images, method)
        plain = hard.test_images(x[:n_images])
        assert len(got) == n_images and sum(len(d[0]) for d in got) > 0
        for n in range(n_images):
            SC.compare_detections(got[n], want[n], method)
            differs += int(len(got[n][0]) != len(plain[n][0]) or not np.array_equal(got[n][0], plain[n][0]))
    assert differs > 0, "no score differs from what 'hard' returns"
    print(f'{method}: detections per image {[len(d[0]) for d in got]}, hard {[len(d[0]) for d in plain]}')
    TB._independence(m, imgs)


def test_hard_is_the_default(ssd_case, dev):
    TB, imgs, model = ssd_case
    default, hard = model(), model(nms_method='hard')
    assert default is not hard and default.nms_method == hard.nms_method == 'hard'
    a, b = default.test_images(imgs.numpy()), hard.test_images(imgs.numpy())
    assert sum(len(d[0]) for d in a) > 0 and hard._tail_batched.out_score is None and hard._tail_batched.method == 0
    for x, y in zip(a, b):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))


# ---------------------------------------------------------------- model level: the per-class fallback tail (heads._per_class_nms)
def test_yolov2_linear_equals_the_oracle_on_the_decode_outputs(dev):
    import test_gpu_yolov2 as TY
    from odtk import ops
    from odtk.yolov2 import STRIDE
    m = TY._model('test', 1, data_shape=[64, 64, 3], nms_score_threshold=0.005, nms_method='linear', nms_iou_threshold=0.3)
    # a freshly initialised net saturates (scores of 0 or 1, boxes of astronomic size: one candidate per class, nothing to decay): with the last layer scaled
    # down the logits are small, every row is a candidate of every class and the five priors of a cell overlap
    p = m.export_params()
    scaled = [k for k in p if k in ('pred.gamma', 'pred.w')][:1]
    assert scaled
    m.load_oracle_params({scaled[0]: p[scaled[0]] * 0.05})
    g = torch.Generator().manual_seed(11)
    img = (torch.rand(1, 64, 64, 3, generator=g) * 255).round()
    got = m.test_one_image(img.numpy())
    H, W = m.grid
    conf, bbox = ops.yolov2_decode_candidates(m.pred[0].view(H, W, m.num_priors, m.num_classes + 5), m.priors_flat, STRIDE)
    conf, bbox = conf.cpu().numpy(), bbox.cpu().numpy()
    want = SC.tail_reference(conf, bbox, (conf >= np.float32(0.005)).astype(np.uint8), m.nms_max_boxes, 1, 0.3, 0.5, 0.005)
    assert len(got[0]) > 0
    SC.compare_detections(got, want, 'linear')
    hard = [conf[:, c].max() for c in range(conf.shape[1])]
    decayed = sum(float(s) not in set(conf[:, c].tolist()) for s, c in zip(got[0], got[2]))
    print(f'YOLOv2 64 x 64 linear: {len(got[0])} detections, {decayed} with a decayed score; best raw score {max(hard):.4f}')
    assert decayed > 0


# ---------------------------------------------------------------- evaluate() of a train-mode model
def test_evaluate_on_a_training_model_carries_the_method(dev):
    """the cached test-mode copy is built from the training model's config (voc_eval.EvaluateMixin.evaluate): it carries nms_method and the two parameters"""
    import test_gpu_refinedet_model as T
    batches = [T._batch(2, 300), T._batch(2, 302), T._batch(1, 304)]
    prov = dict(T._provider(batches[:2]), num_val=5, val_generator=batches)
    t = T._model('train', 2, prov, nms_score_threshold=0.01, nms_method='linear', soft_nms_min_score=0.005)
    t.train_one_epoch(1e-3)
    torch.cuda.synchronize()
    before = (t.P.clone(), t.Mom.clone(), t.S.clone(), t.global_step)
    r2 = t.evaluate(batch_size=2)
    torch.cuda.synchronize()
    assert torch.equal(t.P, before[0]) and torch.equal(t.Mom, before[1]) and torch.equal(t.S, before[2]) and t.global_step == before[3]
    e = t._eval_models[2]
    assert e.mode == 'test' and e.batch_size == 2 and e.nms_method == 'linear' and e.soft_nms_min_score == 0.005 and e.soft_nms_sigma == 0.5
    assert e._tail_batched.method == 1 and e._tail_batched.min_score == 0.005 and e._tail_batched.out_score is not None
    print(f"detections {int(r2['num_detections'].sum())}")
    assert int(r2['num_detections'].sum()) > 0
