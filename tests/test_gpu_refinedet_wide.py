"""GPU: ODM rows of 97 .. 256 logits (RefineDet320 / PFPNetR with more than 95 object classes) -- odtk_refinedet_loss, odtk_refinedet_decode and
odtk_refinedet_decode_batched through the C-ABI against the float64 restatements of tests/refinedet_wide_cases.py (bounds derived there), the refusal at
257, bit-identical reruns, the one-thread kernels at 96 and 21 logits against bytes recorded from the commit before the wide kernels; then RefineDet320 and
PFPNetR built with num_classes = 120 on the f32 engine: one training step against the oracles under the bounds of the 20-class model tests, test_images of 2
images against test_one_image, and evaluate(metric='coco')."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import refinedet_wide_cases as R     # noqa: E402


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


# ---------------------------------------------------------------- the kernels through the C-ABI
@pytest.mark.parametrize('A', R.SIZES)
@pytest.mark.parametrize('C', R.CLASSES)
@pytest.mark.parametrize('batched', [False, True])
def test_decode(C, A, batched, dev):
    R.check_decode(C, A, dev, batched)


@pytest.mark.parametrize('C', R.CLASSES)
def test_batched_decode_equals_two_single_calls(C, dev):
    R.check_batched_equals_single(C, 301, dev)


@pytest.mark.parametrize('C', R.CLASSES)
def test_first_of_two_equal_maxima_wins(C, dev):
    R.check_tie_rows_are_kept(C, 301, dev)


@pytest.mark.parametrize('A', R.SIZES)
@pytest.mark.parametrize('C', R.CLASSES)
def test_loss(C, A, dev):
    R.check_loss(C, A, dev)


def test_no_odm_negative_gives_the_nan_of_the_one_thread_kernel(dev):
    R.check_nan_kind(129, 301, dev)


def test_reruns_are_bit_identical(dev):
    R.check_rerun(dev)


def test_refusal_names_the_limit(dev):
    R.check_refusals(dev)


def test_up_to_96_logits_the_outputs_are_those_of_the_previous_version(dev):
    """every output of the three entry points at C = 96 and C = 21 has the bytes the commit before the wide kernels (4bc7589, library version 107) wrote for
    the same operands on an MI355X: SHA-256 per output, tests/golden/refinedet_limit_sha256.json, recorded with R.sha256_of(R.limit_outputs(dev)) on that
    commit's build"""
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'refinedet_limit_sha256.json')))
    got = R.sha256_of(R.limit_outputs(dev))
    assert sorted(got) == sorted(want) and len(got) == 52
    assert [k for k in got if got[k] != want[k]] == []


# ---------------------------------------------------------------- the two classes at 120 classes
NUM = 120


def _spread(gt):
    """the oracle's synthetic ground truth draws 20 labels: spread them over 0 .. 119 (label 19 -> 119, the last class)"""
    gt = gt.clone()
    valid = gt[..., 0] >= 0
    gt[..., 4] = torch.where(valid, gt[..., 4] * 6 + 5, gt[..., 4])
    assert float(gt[..., 4].max()) <= NUM - 1
    return gt


def _rel(a, b):
    return float((a - b).norm()) / (float(b.norm()) + 1e-30)


def _model_at_120(T, NR, seed, l2_bound):
    """T: the 20-class model test module (its _model / _batch / _provider), NR: the oracle.  The comparisons and bounds are those of T's own test: predictions
    2e-3 of the largest + 1, loss 2e-3, every gradient 6e-2 (relative Frobenius), the L2-norm scalars as there."""
    torch.set_num_threads(16)
    p = NR.init_params(seed, num_classes=NUM + 1)
    imgs, gt = T._batch(2, 210 + seed)
    gt = _spread(gt)
    m = T._model('train', 2, T._provider([(imgs, gt)]), num_classes=NUM)
    assert m.num_classes == NUM + 1 and tuple(m.odm_conf.shape) == (2, m.A, NUM + 1)
    m.load_oracle_params(p)
    m.set_batch(imgs, gt)
    loss = float(m.train_step(0.001).item())
    torch.cuda.synchronize()
    with torch.no_grad():
        want = NR.forward(p, imgs, True)
    for got, w, tag in zip((m.arm_loc, m.arm_conf, m.odm_loc, m.odm_conf), want, ('arm_loc', 'arm_conf', 'odm_loc', 'odm_conf')):
        assert float((got.cpu() - w).abs().max()) < 2e-3 * (float(w.abs().max()) + 1), tag
    q = {k: v.clone() for k, v in p.items()}
    mom = {k: torch.zeros_like(p[k]) for k in NR.trainable_names(p)}
    total, data, grads = NR.train_step(q, mom, imgs, gt, 0.001)
    print(f'{m.NAME} {NUM} classes: loss', loss, 'oracle', total)
    assert abs(loss - total) < 2e-3 * abs(total), (loss, total)
    worst = ('', 0.)
    for k in NR.trainable_names(p):
        if k.endswith('.b') and (k[:-2] + '.gamma') in p:
            assert float(m.get_param(k, m.G).abs().max()) == 0.0
            continue
        w = grads[k] - 1e-4 * p[k]
        if not l2_bound(k, m.get_param(k, m.G), w, grads):
            err = _rel(m.get_param(k, m.G), w)
            worst = max(worst, (k, err), key=lambda t: t[1])
            assert err < 6e-2, (k, err)
    print(f'{m.NAME} {NUM} classes: worst relative gradient error', worst)
    # inference: moving statistics of a training-mode pass over the raw pixels; test_images of two images against test_one_image of a model without the key
    stats = {}
    with torch.no_grad():
        NR.forward(p, imgs, True, stats_out=stats, subtract_mean=False)
    for name, (mean, unb) in stats.items():
        p[name + '.mmean'], p[name + '.mvar'] = mean.clone(), unb.clone()
    one = T._model('test', 1, num_classes=NUM, nms_score_threshold=0.01)
    one.load_oracle_params(p)
    two = T._model('test', 1, num_classes=NUM, nms_score_threshold=0.01, test_batch_size=2)
    two.load_oracle_params(p)
    got = two.test_images(imgs.numpy())
    assert len(got) == 2
    total = 0
    for n in range(2):
        ref = one.test_one_image(imgs[n:n + 1].numpy())
        for a, b in zip(got[n], ref):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        total += len(ref[0])
    print(f'{m.NAME} {NUM} classes: {total} detections in two images')
    r = two.evaluate(generator=[(imgs, gt)], metric='coco')
    # AP per class, length 120: finite for every class that has ground truth (the evaluator's NaN means "no ground truth of this class", voc_eval.py)
    ap, has_gt = np.asarray(r['AP_per_class'], dtype=np.float64), r['npos'][0] > 0
    assert ap.shape == (NUM,) and has_gt.shape == (NUM,) and has_gt.any() and bool(has_gt[NUM - 1]) == bool((gt[..., 4] == NUM - 1).any())
    assert np.isfinite(ap[has_gt]).all() and np.isnan(ap[~has_gt]).all() and np.isfinite(r['AP'])


def _zero_gradients(k, got, want, grads):
    """the parameters whose true gradient is ~0 (both sides hold round-off), held as the 20-class tests hold them; True if k is one of them"""
    import re
    if k.endswith('_l2_norm'):                       # every consumer starts with conv + batch norm, invariant to the scale of its input
        assert float((got - want).abs().max()) <= 0.3 * float(want.abs().max()) + 1e-4, (k, got, want)
        return True
    if re.fullmatch(r'fl\d_\dd\.beta', k):           # PFPNetR: an offset that the NEXT batch norm removes
        assert float((got - want).abs().max()) <= 1e-2 * float(grads[k[:-5] + '.gamma'].abs().max()) + 1e-5, k
        return True
    return False


def test_refinedet320_with_120_classes(dev):
    import test_gpu_refinedet_model as T
    _model_at_120(T, T.NR, 23, _zero_gradients)


def test_pfpnetr_with_120_classes(dev):
    import test_gpu_pfpnet_model as T
    _model_at_120(T, T.NR, 33, _zero_gradients)
