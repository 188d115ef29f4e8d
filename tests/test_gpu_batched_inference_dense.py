"""GPU: batched inference of CenterNet, RefineDet320 and PFPNetR -- odtk_centernet_decode_batched / odtk_refinedet_decode_batched through the C-ABI against
the single-image entry points (torch.equal), test_images() of the three classes against a model built without test_batch_size, independence of the image
slots, evaluate(batch_size=2) on train-mode models."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from test_gpu_batched_inference import _independence, _same     # noqa: E402

import batched_dense_cases as DC     # noqa: E402


# ---------------------------------------------------------------- 1: the CenterNet tail through the C-ABI
@pytest.mark.parametrize('H,W,C,top_k', [(5, 7, 3, 5), (16, 16, 20, 10), (128, 128, 2, 100), (16, 16, 20, 1)])
def test_centernet_decode_batched_equals_single_image_decode(H, W, C, top_k, dev):
    """N = 3: an image with no pixel above the threshold, one with more peaks than top_k, one with a plateau of equal logits (DC.centernet_logits); the last
    shape is the H * W cap"""
    DC.check_centernet(H, W, C, top_k, dev)


def test_centernet_read_back_class(dev):
    from odtk import ops
    tail, kp, off, size = DC.check_centernet_read_back(dev)
    for bad in (0, 65536):
        with pytest.raises(Exception, match=f'centernet_decode_batched: N={bad} out of range'):
            ops.call('odtk_centernet_decode_batched', ops._p(kp), ops._p(off), ops._p(size), bad, 16, 16, 20, DC.STRIDE, DC.THR, 10, ops._p(tail.scores),
                     ops._p(tail.bbox), ops._p(tail.class_id), ops._p(tail.counts), ops._p(tail.ws), ops._stream())


# ---------------------------------------------------------------- 2: the RefineDet decode through the C-ABI, then the batched tail
@pytest.mark.parametrize('N,A,C', [(3, 37, 4), (2, 6375, 21)])
def test_refinedet_decode_batched_equals_single_image_decode(N, A, C, dev):
    DC.check_refinedet(N, A, C, dev)


def test_refinedet_decode_batched_rejects_n_out_of_range(dev):
    from odtk import ops
    A, C = 37, 4
    z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)
    arm_loc, arm_conf, odm_loc, odm_conf, yx, hw = z(1, A, 4), z(1, A, 2), z(1, A, 4), z(1, A, C), z(A, 2), z(A, 2) + 1.0
    conf, boxes, keep, cand = z(1, A, C - 1), z(1, A, 4), z(1, A, dt=torch.uint8), z(1, A, C - 1, dt=torch.uint8)
    for bad in (0, 65536):
        with pytest.raises(Exception, match=f'refinedet_decode_batched: N={bad} out of range'):
            ops.call('odtk_refinedet_decode_batched', ops._p(arm_loc), ops._p(arm_conf), ops._p(odm_loc), ops._p(odm_conf), bad, A, C, ops._p(yx), ops._p(hw), 0.3,
                     ops._p(conf), ops._p(boxes), ops._p(keep), ops._p(cand), ops._stream())


# ---------------------------------------------------------------- 3 - 5: the three classes
def _calibrated(NR, p, imgs, **kw):
    """moving statistics from a training-mode forward pass of the oracle over `imgs`, as a trained checkpoint would hold them"""
    stats = {}
    with torch.no_grad():
        NR.forward(p, imgs, True, stats_out=stats, **kw)
    for name, (mean, unb) in stats.items():
        p[name + '.mmean'], p[name + '.mvar'] = mean.clone(), unb.clone()
    return p


def _pair(T, p, **kw):
    m = T._model('test', 1, test_batch_size=3, **kw)
    m.load_oracle_params(p)
    one = T._model('test', 1, **kw)
    one.load_oracle_params(p)
    assert m.batch_size == 3 and one.batch_size == 1 and m.NATIVE_TEST_IMAGES
    return m, one


@pytest.fixture(scope='module')
def centernet_case():
    import test_gpu_centernet_model as T
    torch.set_num_threads(16)
    p = T.NR.init_params(19)
    p['c63.beta'] = p['c63.beta'] + 1.0                     # lift the keypoint logits so that peaks pass the score threshold (test_gpu_centernet_model.py)
    imgs, _ = T._batch(3, 150)
    _calibrated(T.NR, p, imgs, normalize=False)
    return _pair(T, p) + (imgs,)


@pytest.fixture(scope='module')
def refinedet_case():
    import test_gpu_refinedet_model as T
    torch.set_num_threads(16)
    p = T.NR.init_params(29)
    imgs, _ = T._batch(3, 220)
    _calibrated(T.NR, p, imgs, subtract_mean=False)
    return _pair(T, p) + (imgs,)


@pytest.fixture(scope='module')
def pfpnet_case():
    import test_gpu_pfpnet_model as T
    torch.set_num_threads(16)
    p = T.NR.init_params(39)
    imgs, _ = T._batch(3, 220)
    _calibrated(T.NR, p, imgs, subtract_mean=False)
    return _pair(T, p) + (imgs,)


CASES = ['centernet_case', 'refinedet_case', 'pfpnet_case']


@pytest.mark.parametrize('case', CASES)
def test_batched_equals_the_batch_1_model(case, request, dev):
    """the comparison and the bound of test_gpu_batched_inference.py::test_ssd300_batched_equals_the_batch_1_model: the forward pass at N = 3 + batched tail
    against a model built WITHOUT test_batch_size (N = 1, test_one_image's own tail) on the same weights -- every array ==; a full and a partial batch"""
    m, one, imgs = request.getfixturevalue(case)
    want = [one.test_one_image(imgs[n: n + 1].numpy()) for n in range(3)]
    for n_img in (3, 2):
        got = m.test_images(imgs[:n_img].numpy())
        assert len(got) == n_img
        for n in range(n_img):
            print(f'{case} image {n} of {n_img}: {len(want[n][0])} detections (batch-1 model), {len(got[n][0])} (batched)')
            assert len(want[n][0]) > 0 and _same(got[n], want[n]), (n_img, n)


def test_pfpnet_inherits_the_batched_path(pfpnet_case):
    import odtk
    assert 'test_images' not in vars(odtk.PFPNetR) and odtk.PFPNetR.test_images is odtk.RefineDet320.test_images
    m = pfpnet_case[0]
    assert all(a.N == 3 for a in m.acts.values()) and tuple(m.odm_conf.shape) == (3, 6375, 21)


@pytest.mark.parametrize('case', CASES)
def test_images_are_independent(case, request, dev):
    m, _, imgs = request.getfixturevalue(case)
    _independence(m, imgs)


@pytest.mark.parametrize('case', CASES)
def test_one_image_of_a_batched_model_is_the_batched_path(case, request, dev):
    m, _, imgs = request.getfixturevalue(case)
    for n in range(2):
        a = m.test_one_image(imgs[n: n + 1].numpy())
        b = m.test_images(imgs[n: n + 1].numpy())
        assert len(b) == 1 and len(a[0]) > 0 and _same(a, b[0]), n


# ---------------------------------------------------------------- 6: evaluate(batch_size=2) on train-mode models
@pytest.mark.parametrize('name', ['centernet', 'refinedet'])
def test_evaluate_batch_size_2_on_a_training_model(name, dev):
    """the rule of test_evaluate_batch_size (AP, npos and tp equal as arrays) between evaluate(batch_size=2) and evaluate(batch_size=1), and the training
    state untouched as in test_evaluate_batch_size_leaves_the_training_state"""
    if name == 'centernet':
        import test_gpu_centernet_model as T
        kw, opt = {'score_threshold': 0.01}, ('M1', 'M2')
    else:
        import test_gpu_refinedet_model as T
        kw, opt = {'nms_score_threshold': 0.01}, ('Mom',)
    batches = [T._batch(2, 300), T._batch(2, 302), T._batch(1, 304)]
    prov = dict(T._provider(batches[:2]), num_val=5, val_generator=batches)
    t = T._model('train', 2, prov, **kw)
    t.train_one_epoch(1e-3)
    torch.cuda.synchronize()
    before = (t.P.clone(), [getattr(t, k).clone() for k in opt], t.S.clone(), t.global_step)
    r2 = t.evaluate(batch_size=2)
    r2b = t.evaluate(batch_size=2)
    r1 = t.evaluate(batch_size=1)
    torch.cuda.synchronize()
    assert torch.equal(t.P, before[0]) and all(torch.equal(getattr(t, k), b) for k, b in zip(opt, before[1])) and torch.equal(t.S, before[2])
    assert t.global_step == before[3]
    assert sorted(t._eval_models) == [1, 2] and t._eval_models[2].batch_size == 2 and t._eval_models[1].batch_size == 1
    assert t._eval_models[2].mode == 'test' and tuple(t._eval_models[2].images.shape[:1]) == (2,)
    print(f'{name}: detections {int(r2["num_detections"].sum())} (batch_size 2), {int(r1["num_detections"].sum())} (batch_size 1)')
    assert int(r2['num_detections'].sum()) > 0
    assert np.array_equal(r2['tp'], r2b['tp']) and np.array_equal(r2['AP'], r2b['AP'], equal_nan=True)
    assert np.array_equal(r2['AP'], r1['AP'], equal_nan=True) and np.array_equal(r2['npos'], r1['npos']) and np.array_equal(r2['tp'], r1['tp'])
