"""GPU: batched inference -- the tail of csrc/detect_batched.hip through the C-ABI, test_images() of the native classes and of a fallback class, a default
model's test_one_image against the test-side single-image tail (tests/single_image_tail.py), evaluate(batch_size=B).  The tail and compaction bodies are tests/batched_inference_cases.py (shared with the CPU tier, where the same kernels run from
source under the emulation)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import batched_inference_cases as BC     # noqa: E402
from oracle import ssd300_ref as R       # noqa: E402

SSD_CONFIG = {'mode': 'test', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 2,
              'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': './vgg_16.ckpt', 'verbose': False,
              'compute_dtype': 'f32'}


def _same(a, b):
    return len(a) == 3 and len(b) == 3 and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1, 2: the tail and the compaction through the C-ABI
@pytest.mark.parametrize('kind', ['ssd', 'retina'])
def test_tail_equals_single_image_tail(kind, dev):
    per = BC.check_tail(kind, dev)
    print(f'{kind}: detections per (image, class)\n{per}')


def test_compaction_equals_nonzero(dev):
    BC.check_compaction(dev)


def test_compaction_overflow_names_the_image(dev):
    """more candidate rows than the NMS takes per problem: the existing ValueError, with the image's index"""
    from odtk import heads
    N, A, nc = 3, 33000, 2
    conf = torch.rand(N, A, nc, device=dev); boxes = torch.rand(N, A, 4, device=dev)
    cand = torch.zeros(N, A, nc, dtype=torch.uint8, device=dev)
    cand[1] = 1
    cand[0, :100] = 1
    tail = heads.BatchedTail(N, A, nc, 5, dev)
    with pytest.raises(ValueError, match=r'image 1: 33000 candidate boxes exceed the NMS capacity of 32768'):
        tail(conf, boxes, cand, 0.5)
    assert len(tail(conf, boxes, cand, 0.5, n_images=1)) == 1            # (image 1 is a discarded tail slot here)


# ---------------------------------------------------------------- 3: model level against the oracle, tolerances of the batch-1 parity tests
@pytest.fixture(scope='module')
def ssd300_case():
    import odtk
    torch.set_num_threads(16)
    p = R.init_params(3)
    imgs, gt = R.synthetic_batch(4, 7)
    R.calibrate_bn(p, imgs[:2], subtract_mean=False)           # (test_gpu_ssd300.py::test_inference_parity_f32's weights)
    m = odtk.SSD300(dict(SSD_CONFIG, test_batch_size=4), None)
    m.load_oracle_params(p)
    one = odtk.SSD300(dict(SSD_CONFIG), None)
    one.load_oracle_params(p)
    return p, imgs, gt, m, one


def test_ssd300_test_images_vs_oracle(ssd300_case, dev):
    """tolerances of tests/test_gpu_ssd300.py::test_inference_parity_f32 (exact f32 engine), unchanged and all asserted: class ids equal, scores 5e-4
    absolute, boxes 0.1 px absolute and 3e-3 of the box size over the boxes of >= 16 px.  The batch is three images whose detections stay inside a few
    hundred pixels.  The absolute reading does not hold for every picture: a random-weight net also emits boxes over 1 000 px across (h = prior_h * exp(z):
    a box is as accurate as its logit), and on such a box engine and oracle differ by 0.12 - 0.29 px at a relative 3e-4 -- in test_one_image exactly as in
    test_images (test_ssd300_batched_equals_the_batch_1_model holds the two paths bit-identical on those pictures too; DESIGN.md, Evaluation)."""
    p, _, _, m, _ = ssd300_case
    imgs = R.synthetic_batch(4, 8)[0]
    B = 3
    for thr in (0.5, 0.2):
        m.nms_score_threshold = thr
        got = m.test_images(imgs[:B].numpy())
        assert len(got) == B
        for n in range(B):
            s, b, c = got[n]
            s_ref, b_ref, c_ref = R.test_one_image(p, imgs[n: n + 1], thr, 20, 0.5)
            assert c.tolist() == c_ref.tolist(), (thr, n)
            assert len(s_ref) > 0
            size = np.sqrt(np.maximum((b_ref[:, 2] - b_ref[:, 0]) * (b_ref[:, 3] - b_ref[:, 1]), 0.0))
            big = size >= 16.0
            rel = float((np.abs(b - b_ref).max(axis=1)[big] / size[big]).max()) if big.any() else 0.0
            print(f'thr {thr} image {n}: {len(s_ref)} detections, scores {float(np.abs(s - s_ref).max()):.2e}, boxes {float(np.abs(b - b_ref).max()):.3f} px, '
                  f'{rel:.2e} of the box size over the {int(big.sum())} boxes of >= 16 px')
            assert float(np.abs(s - s_ref).max()) < 5e-4
            assert float(np.abs(b - b_ref).max()) < 0.1
            assert rel < 3e-3
    m.nms_score_threshold = 0.5


def test_ssd300_batched_equals_the_batch_1_model(ssd300_case, dev):
    """two models, two engines' worth of dispatch: the forward pass at N = 4 + batched tail against a model built WITHOUT test_batch_size (N = 1,
    test_one_image's own tail) on the same weights -- every array ==, for eight pictures, including the ones whose far-out boxes miss the 0.1 px absolute
    reading against the oracle (seed 7 images 2, 3 and seed 8 image 3: 0.12 / 0.27 / 0.29 px, the same number on both paths)"""
    _, _, _, m, one = ssd300_case
    try:
        for seed in (7, 8):
            imgs = R.synthetic_batch(4, seed)[0]
            for thr in (0.5, 0.2):
                one.nms_score_threshold = m.nms_score_threshold = thr
                got = m.test_images(imgs.numpy())
                for n in range(4):
                    want = one.test_one_image(imgs[n: n + 1].numpy())
                    assert len(want[0]) > 0 and _same(got[n], want), (seed, thr, n)
    finally:
        one.nms_score_threshold = m.nms_score_threshold = 0.5


def test_ssd512_test_images_vs_oracle(dev):
    """tolerances of tests/test_gpu_ssd512.py (inference part): class ids equal, scores 1e-3, boxes 1e-3 * 512"""
    import odtk
    from oracle import ssd512_ref as R5
    torch.set_num_threads(16)
    imgs, _ = R5.synthetic_batch(4, 45)
    p = R5.init_params(3)
    R5.calibrate_bn(p, imgs[:2], subtract_mean=False)
    t = odtk.SSD512(dict(SSD_CONFIG, test_batch_size=2), None)
    t.load_oracle_params(p)
    for thr in (0.5, 0.2):
        t.nms_score_threshold = thr
        got = t.test_images(imgs[:2].numpy())
        for n in range(2):
            s, b, c = got[n]
            s_ref, b_ref, c_ref = R5.test_one_image(p, imgs[n: n + 1], thr, 20, 0.5)
            assert c.tolist() == c_ref.tolist(), (thr, n)
            if len(s_ref):
                assert float(np.abs(s - s_ref).max()) < 1e-3 and float(np.abs(b - b_ref).max()) < 1e-3 * 512


@pytest.fixture(scope='module')
def yolov3_case():
    import test_gpu_yolov3 as TY
    NR = TY.NR
    torch.set_num_threads(16)
    p = NR.init_params(8)
    imgs, _ = TY._batch(3, 128, 60)
    stats = {}
    with torch.no_grad():
        NR.forward(p, imgs[:1] + 20 * torch.randn(imgs[:1].shape, generator=torch.Generator().manual_seed(2)), True, stats, subtract_mean=False)
    for k, (mean, var) in stats.items():
        p[k + '.mmean'], p[k + '.mvar'] = mean.clone(), var.clone()
    m = TY._model('test', 'f32', 1, 128, nms_score_threshold=0.5, test_batch_size=3)
    m.load_oracle_params(p)
    return NR, p, imgs, m


def test_yolov3_test_images_vs_oracle(yolov3_case, dev):
    """tolerances of tests/test_gpu_yolov3.py::test_f32_inference_detections_equal_oracle: class ids equal, scores 2e-3, boxes 0.5 px"""
    NR, p, imgs, m = yolov3_case
    got = m.test_images(imgs.numpy())
    total = 0
    for n in range(3):
        want = NR.test_one_image(p, imgs[n: n + 1], 0.5, 10, 0.5)
        total += len(want[0])
        assert len(got[n][0]) == len(want[0]) and np.array_equal(got[n][2], want[2].numpy()), n
        np.testing.assert_allclose(got[n][0], want[0].numpy(), atol=2e-3)
        np.testing.assert_allclose(got[n][1], want[1].numpy(), atol=0.5)
    assert total > 0


@pytest.fixture(scope='module')
def retinanet_case():
    import test_gpu_retinanet_model as TR
    NR = TR.NR
    torch.set_num_threads(16)
    p = NR.init_params(9)
    imgs, _ = TR._batch(2, 160, 95)
    stats = {}
    with torch.no_grad():
        NR.forward(p, imgs[:1] + 20 * torch.randn(imgs[:1].shape, generator=torch.Generator().manual_seed(2)), True, stats, subtract_mean=False)
    for k, (mean, var) in stats.items():
        p[k + '.mmean'], p[k + '.mvar'] = mean.clone(), var.clone()
    for i in (81, 91, 101, 111, 121):
        p[f'l{i}.w'] = p[f'l{i}.w'] * 0.02
    m = TR._model('test', 'f32', 1, 160, nms_score_threshold=0.15, test_batch_size=2)
    m.load_oracle_params(p)
    return TR, p, imgs, m


def test_retinanet_test_images_vs_oracle(retinanet_case, dev):
    """the bounds of tests/test_gpu_retinanet_model.py::test_f32_inference_detections_equal_oracle per image: logits 2e-3 of their range against the oracle's
    forward pass; against the free-running oracle's detections the same count and class ids, scores 2e-3, at least 95 % of the rows within 2 px + 5e-3; and
    the oracle's decode + per-class NMS on the engine's own logits give the engine's detections row for row (class ids and order identical, scores 1e-5,
    boxes 0.05 px)"""
    TR, p, imgs, m = retinanet_case
    NR, RR, DC = TR.NR, TR.RR, TR.DC
    thr = 0.15
    anc = RR.anchors([160, 160, 3], RR.pyramid_shapes(160, 160))
    # the free-running oracle's detections, tolerances of the batch-1 parity test, in BOTH slots of the batch: on the picture that test is calibrated on (its
    # score bound of 2e-3 is a property of that picture: on the second picture of this batch the engine's own per-image path is 3.2e-3 from the oracle on one
    # score of 200 with the logits inside their bound; recorded in DESIGN.md, Evaluation).  Distinct pictures follow below and in the independence cases
    x = imgs[:1]
    got = m.test_images(torch.cat([x, x]).numpy())
    with torch.no_grad():
        pc, pb = NR.forward(p, x, False, subtract_mean=False)
    conf, boxes, keep, _ = RR.decode_candidates(pb[0, :, :2], pb[0, :, 2:], pc[0], anc, thr)
    want = DC.per_class_nms(conf, boxes, 20, thr, 10, 0.45, row_mask=keep)
    for n in range(2):
        assert len(want[0]) > 0 and len(got[n][0]) == len(want[0]), (n, len(got[n][0]), len(want[0]))
        assert np.array_equal(got[n][2], want[2].numpy()), n
        np.testing.assert_allclose(got[n][0], want[0].numpy(), atol=2e-3)
        w = want[1].numpy()
        row_ok = (np.abs(got[n][1] - w) <= 2.0 + 5e-3 * np.abs(w)).all(axis=1)
        assert row_ok.mean() >= 0.95, (n, row_ok.mean())
    got = m.test_images(imgs.numpy())
    total = 0
    for n in range(2):
        with torch.no_grad():
            pc, pb = NR.forward(p, imgs[n: n + 1], False, subtract_mean=False)
        assert float((m.pconf[n].cpu() - pc[0]).abs().max()) < 2e-3 * (float(pc.abs().max()) + 1)
        pc_e, pb_e = m.pconf.cpu()[n], m.pbox.cpu()[n]
        conf_e, boxes_e, keep_e, _ = RR.decode_candidates(pb_e[:, :2], pb_e[:, 2:], pc_e, anc, thr)
        same = DC.per_class_nms(conf_e, boxes_e, 20, thr, 10, 0.45, row_mask=keep_e)
        total += len(same[0])
        assert np.array_equal(got[n][2], same[2].numpy()) and len(got[n][0]) == len(same[0]), n
        np.testing.assert_allclose(got[n][0], same[0].numpy(), atol=1e-5)
        assert float(np.abs(got[n][1] - same[1].numpy()).max(initial=0.0)) <= 0.05 + 1e-5 * float(np.abs(same[1].numpy()).max(initial=0.0))
    assert total > 0


def _above_the_nms_capacity(TR, p, B):
    """RetinaNet at 448 x 448 has 37 629 anchors, more than the NMS takes per problem: the tail goes through odtk_compact_rows / odtk_gather_rows.  On the
    model's own head outputs the single-image tail (single_image_tail.retina_detect: torch.nonzero + gathers) must give the same arrays, ==, for every
    image.  B = None: a model built WITHOUT test_batch_size, fed one image at a time through test_one_image."""
    from single_image_tail import retina_detect
    imgs, _ = TR._batch(2, 448, 96)
    m = TR._model('test', 'f32', 1, 448, nms_score_threshold=0.999, **({} if B is None else {'test_batch_size': B}))
    m.load_oracle_params(p)
    x = imgs.numpy()
    run = m.test_images if B else (lambda xs: [m.test_one_image(xs[n: n + 1]) for n in range(xs.shape[0])])
    run(x[:B or 1])
    t = m._tail_batched
    assert m.batch_size == (B or 1) and m.pconf.shape[1] == 37629 and t.compact
    # a threshold that leaves ~3 000 candidate rows per image (random weights: at the parity test's 0.15 nearly every anchor is one): from the decoded scores
    best = t.conf.max(dim=2).values * t.keep
    thr = float(torch.topk(best.flatten(), 3000 * (B or 1)).values[-1])
    assert 0.0 < thr < 0.999
    m.nms_score_threshold = thr
    total = 0
    if B:
        got = run(x)
        assert 0 < int(t.row_cnt.max()) <= 32768 and int(t.row_cnt.sum()) >= 6000
        for n in range(2):
            s, b, c = retina_detect(m.pconf[n], m.pbox[n], m.anc[2], m.anc[3], thr, m.nms_max_boxes, m.nms_iou_threshold)
            assert _same(got[n], [s.cpu().numpy(), b.cpu().numpy().reshape(-1, 4), c.cpu().numpy()]), n
            total += len(got[n][0])
        rev = run(x[::-1].copy())
        assert _same(rev[0], got[1]) and _same(rev[1], got[0])
    else:
        for n in range(2):
            got = m.test_one_image(x[n: n + 1])
            assert 0 < int(t.row_cnt[0]) <= 32768 and (n == 1 or int(t.row_cnt[0]) >= 3000)
            s, b, c = retina_detect(m.pconf[0], m.pbox[0], m.anc[2], m.anc[3], thr, m.nms_max_boxes, m.nms_iou_threshold)
            assert _same(got, [s.cpu().numpy(), b.cpu().numpy().reshape(-1, 4), c.cpu().numpy()]), n
            total += len(got[0])
    assert total > 0
    return m, x


def test_retinanet_test_images_above_the_nms_capacity(retinanet_case, dev):
    TR, p, _, _ = retinanet_case
    _above_the_nms_capacity(TR, p, 2)


def test_retinanet_default_model_above_the_nms_capacity_and_overflow(retinanet_case, dev):
    """the same comparison for a model built without test_batch_size: test_one_image takes odtk_compact_rows / odtk_gather_rows where the single-image tail
    takes torch.nonzero.  Then more candidate rows than the NMS takes per problem: the ValueError of the batched tail, naming image 0"""
    TR, p, _, _ = retinanet_case
    m, x = _above_the_nms_capacity(TR, p, None)
    best = m._tail_batched.conf.max(dim=2).values * m._tail_batched.keep
    m.nms_score_threshold = float(torch.topk(best.flatten(), 33000).values[-1])          # at least 33 000 of the 37 629 rows are candidates
    with pytest.raises(ValueError, match=r'image 0: \d+ candidate boxes exceed the NMS capacity of 32768'):
        m.test_one_image(x[1:2])


# ---------------------------------------------------------------- 4: independence of the images
def _independence(m, imgs):
    B = imgs.shape[0]
    x = imgs.numpy()
    fwd = m.test_images(x)
    rev = m.test_images(x[::-1].copy())
    assert sum(len(d[0]) for d in fwd) > 0
    for n in range(B):
        assert _same(fwd[n], rev[B - 1 - n]), n
    m.test_images(x[::-1].copy())                                   # the tail slots hold OTHER images than the full batch has there
    part = m.test_images(x[: B - 1])
    assert len(part) == B - 1
    for n in range(B - 1):
        assert _same(part[n], fwd[n]), n
    again = m.test_images(x)
    assert all(_same(a, b) for a, b in zip(again, fwd))


def test_ssd300_images_are_independent(ssd300_case, dev):
    _, imgs, _, m, _ = ssd300_case
    m.nms_score_threshold = 0.2
    try:
        _independence(m, imgs)
    finally:
        m.nms_score_threshold = 0.5


def test_yolov3_images_are_independent(yolov3_case, dev):
    _independence(yolov3_case[3], yolov3_case[2])


def test_retinanet_images_are_independent(retinanet_case, dev):
    _independence(retinanet_case[3], retinanet_case[2])


# ---------------------------------------------------------------- 5: the default model (no test_batch_size): test_one_image is the batched path with one image
def _default_model(name, ssd300_case, yolov3_case, retinanet_case):
    """-> (model built WITHOUT test_batch_size at the smallest input its tests build it at, on calibrated oracle weights; two pictures; two thresholds)"""
    import odtk
    import test_gpu_batched_inference_dense as TD
    if name == 'SSD300':
        return ssd300_case[4], ssd300_case[1][:2].numpy(), (0.5, 0.2)
    if name == 'SSD512':
        from oracle import ssd512_ref as R5
        imgs, _ = R5.synthetic_batch(2, 45)
        p = R5.init_params(3)
        R5.calibrate_bn(p, imgs, subtract_mean=False)
        m = odtk.SSD512(dict(SSD_CONFIG), None)
        m.load_oracle_params(p)
        return m, imgs.numpy(), (0.5, 0.2)
    if name == 'YOLOv3':
        import test_gpu_yolov3 as TY
        m = TY._model('test', 'f32', 1, 64, nms_score_threshold=0.5)
        m.load_oracle_params(yolov3_case[1])
        return m, TY._batch(2, 64, 60)[0].numpy(), (0.5, 0.3)
    if name == 'RetinaNet':
        TR = retinanet_case[0]
        m = TR._model('test', 'f32', 1, 128, nms_score_threshold=0.15)
        m.load_oracle_params(retinanet_case[1])
        return m, TR._batch(2, 128, 95)[0].numpy(), (0.15, 0.05)
    T = __import__({'CenterNet': 'test_gpu_centernet_model', 'RefineDet320': 'test_gpu_refinedet_model', 'PFPNetR': 'test_gpu_pfpnet_model'}[name])
    p = T.NR.init_params({'CenterNet': 19, 'RefineDet320': 29, 'PFPNetR': 39}[name])
    imgs, _ = T._batch(3, 150 if name == 'CenterNet' else 220)
    if name == 'CenterNet':
        p['c63.beta'] = p['c63.beta'] + 1.0
        TD._calibrated(T.NR, p, imgs, normalize=False)
        m = T._model('test', 1, top_k_results_output=10)
    else:
        TD._calibrated(T.NR, p, imgs, subtract_mean=False)
        m = T._model('test', 1)
    m.load_oracle_params(p)
    return m, imgs[:2].numpy(), DEFAULT_THRESHOLDS[name]


DEFAULT_THRESHOLDS = {'CenterNet': (0.3, 0.1), 'RefineDet320': (0.3, 0.1), 'PFPNetR': (0.3, 0.1)}


@pytest.mark.parametrize('name', ['SSD300', 'SSD512', 'YOLOv3', 'RetinaNet', 'CenterNet', 'RefineDet320', 'PFPNetR'])
def test_default_model_test_one_image_equals_test_images_of_one(name, ssd300_case, yolov3_case, retinanet_case, dev):
    """BC.check_default_model: test_one_image of a default model == the test-side single-image tail on the model's own head tensors == test_images(...)[0]"""
    m, imgs, thresholds = _default_model(name, ssd300_case, yolov3_case, retinanet_case)
    assert type(m).__name__ == name
    BC.check_default_model(m, imgs, thresholds, m.top_k_results_output if name == 'CenterNet' else m.nms_max_boxes)
    if name == 'SSD300':
        assert tuple(m.images.shape) == (1, 300, 300, 3) and tuple(m._tail_batched.conf.shape) == (1, 8828, 20)
        with pytest.raises(ValueError, match='test_batch_size'):
            import odtk
            odtk.SSD300(dict(SSD_CONFIG, test_batch_size=0), None)


# ---------------------------------------------------------------- 6: evaluate
def test_evaluate_batch_size(ssd300_case, dev):
    import odtk
    p, _, _, m, one = ssd300_case
    imgs, gt = R.synthetic_batch(21, 31)
    gen = [(imgs[s: s + 7], gt[s: s + 7]) for s in range(0, 21, 7)]               # 3 batches of 7 images
    m.nms_score_threshold = one.nms_score_threshold = 0.2
    try:
        r = m.evaluate(generator=gen, num_images=18, batch_size=4)
        ev = odtk.VOCEvaluator(20)
        dets = []
        for s in range(0, 18, 4):
            dets += m.test_images(imgs[s: min(s + 4, 18)].numpy())
        assert len(dets) == 18 and sum(len(d[0]) for d in dets) > 0
        for d, g in zip(dets, gt.numpy()):
            ev.add(d, g)
        want = ev.result()
        assert np.array_equal(r['AP'], want['AP'], equal_nan=True) and np.array_equal(r['npos'], want['npos']) and np.array_equal(r['tp'], want['tp'])
        assert r['num_detections'].sum() == sum(len(d[0]) for d in dets)
        # the default: the per-image path, bit-identical to a hand loop of test_one_image
        r1 = one.evaluate(generator=gen, num_images=18)
        ev = odtk.VOCEvaluator(20)
        for n in range(18):
            ev.add(one.test_one_image(imgs[n: n + 1].numpy()), gt[n].numpy())
        w1 = ev.result()
        assert np.array_equal(r1['AP'], w1['AP'], equal_nan=True) and np.array_equal(r1['npos'], w1['npos']) and np.array_equal(r1['tp'], w1['tp'])
    finally:
        m.nms_score_threshold = one.nms_score_threshold = 0.5


def test_evaluate_batch_size_leaves_the_training_state(dev):
    import odtk
    imgs, gt = R.synthetic_batch(8, 51)
    prov = {'data_shape': [300, 300, 3], 'num_train': 8, 'num_val': 8, 'train_generator': [(imgs[:4], gt[:4]), (imgs[4:], gt[4:])],
            'val_generator': [(imgs[:4], gt[:4]), (imgs[4:], gt[4:])]}
    t = odtk.SSD300(dict(SSD_CONFIG, mode='train', batch_size=4, compute_dtype='bf16', use_graph=False, nms_score_threshold=0.05), prov)
    t.train_one_epoch(1e-3)
    torch.cuda.synchronize()
    before = (t.P.clone(), t.Mom.clone(), t.S.clone(), t.global_step)
    r4 = t.evaluate(batch_size=4)
    r4b = t.evaluate(batch_size=4)
    r1 = t.evaluate()
    torch.cuda.synchronize()
    assert torch.equal(t.P, before[0]) and torch.equal(t.Mom, before[1]) and torch.equal(t.S, before[2]) and t.global_step == before[3]
    assert sorted(t._eval_models) == [1, 4] and t._eval_models[4].batch_size == 4 and t._eval_models[1].batch_size == 1 and t._eval_model is t._eval_models[1]
    assert t._eval_models[4].mode == 'test' and t._eval_models[4].DT == odtk.F32
    assert np.array_equal(r4['tp'], r4b['tp']) and np.array_equal(r4['AP'], r4b['AP'], equal_nan=True)
    assert np.array_equal(r4['npos'], r1['npos'])


# ---------------------------------------------------------------- 7: the fallback loop
def test_fallback_class_test_images_is_the_loop(dev):
    import test_gpu_fcos_model as TF
    imgs, _ = TF._batch(3, 23)
    m = TF._model('test', 1, nms_score_threshold=0.05)
    assert not m.NATIVE_TEST_IMAGES
    got = m.test_images(imgs.numpy())
    assert len(got) == 3
    for n in range(3):
        assert _same(got[n], m.test_one_image(imgs[n: n + 1].numpy())), n
