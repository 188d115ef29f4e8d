"""GPU: rows of 33 .. 256 logits (SSD300 / SSD512 / RetinaNet with more than 31 object classes) and FCOS with more than 64 classes -- the seven entry points
through the C-ABI against the float64 restatements of tests/wide_row_cases.py (bounds derived there), the refusal at 257, bit-identical reruns, the one-thread kernels at their
limit against bytes recorded from the commit before the wide kernels; then SSD300, RetinaNet and FCOS built with num_classes = 80 on the f32 engine: one
training step and test_images of 2 images against the oracles under the tolerances of the 20-class model tests, and evaluate(metric='coco')."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import wide_row_cases as W     # noqa: E402


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


# ---------------------------------------------------------------- the kernels through the C-ABI
@pytest.mark.parametrize('C', W.CLASSES)
@pytest.mark.parametrize('batched', [False, True])
def test_ssd_decode(C, batched, dev):
    W.check_ssd_decode(C, dev, batched)


@pytest.mark.parametrize('C', W.CLASSES)
@pytest.mark.parametrize('batched', [False, True])
def test_retina_decode(C, batched, dev):
    W.check_retina_decode(C, dev, batched)


@pytest.mark.parametrize('C', W.CLASSES)
def test_ssd_loss(C, dev):
    W.check_ssd_loss(C, dev)


@pytest.mark.parametrize('C', W.CLASSES)
def test_retina_loss(C, dev):
    W.check_retina_loss(C, dev)


@pytest.mark.parametrize('C', W.CLASSES)
def test_fcos_loss(C, dev):
    W.check_fcos_loss(C, dev)


def test_one_thread_kernels_at_their_limit(dev):
    """C = 32 stays on the one-thread-per-row kernels (C = 64 on FCOS's one-word kernel: in W.CLASSES): the same restatement, the bound of a 31-add sum"""
    for batched in (False, True):
        W.check_ssd_decode(32, dev, batched)
        W.check_retina_decode(32, dev, batched)
    W.check_ssd_loss(32, dev)
    W.check_retina_loss(32, dev)


def test_dispatch_at_the_limit_is_the_one_thread_kernel(dev):
    """every output of the seven entry points at C = 32 (FCOS: 64) has the bytes the commit before the wide kernels wrote for the same operands on an MI355X
    (SHA-256 per output, tests/golden/wide_rows_limit_sha256.json, recorded with W.sha256_of(W.limit_outputs(dev)) on that commit's build)"""
    import json
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wide_rows_limit_sha256.json')))
    got = W.sha256_of(W.limit_outputs(dev))
    assert sorted(got) == sorted(want) and len(got) > 20
    assert [k for k in got if got[k] != want[k]] == []


def test_reruns_are_bit_identical(dev):
    W.check_rerun(dev)


def test_refusal_names_the_limit(dev):
    W.check_refusals(dev)


# ---------------------------------------------------------------- the three classes at 80 classes
def _spread(gt, num_classes=80):
    """the oracles' synthetic ground truth draws 20 labels: spread them over 0 .. 79 (label 19 -> 79, the last class)"""
    gt = gt.clone()
    valid = gt[..., 0] >= 0
    gt[..., 4] = torch.where(valid, gt[..., 4] * 4 + 3, gt[..., 4])
    assert float(gt[..., 4].max()) <= num_classes - 1
    return gt


def _coco_runs(m, batches):
    r = m.evaluate(generator=batches, metric='coco')
    assert 'AP' in r and np.asarray(r['AP']).size > 0


def test_fcos_with_80_classes(dev):
    """tests/test_gpu_fcos_model.py's comparison and bounds (loss 2e-3, every gradient 1e-2 relative; detections: classes equal, scores 2e-3, boxes
    2 px + 5e-3) at num_classes = 80, on 128 x 128 images"""
    import test_gpu_fcos_model as T
    from oracle import detect_common as DC
    NR, FR = T.NR, T.FR
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(340)
    imgs = (torch.rand(2, 128, 128, 3, generator=g) * 255).round()
    gt = _spread(FR.synthetic_gt(2, 128, 341))
    p = NR.init_params(17, num_classes=80)
    kw = dict(num_classes=80, data_shape=[128, 128, 3])
    m = T._model('train', 2, T._provider([(imgs, gt)]), **kw)
    m.load_oracle_params(p)
    m.set_batch(imgs, gt)
    loss = float(m.train_step(0.001).item())
    q = {k: v.clone() for k, v in p.items()}
    masks = {}
    for name, a in m.acts.items():
        if name == 'l0' or name.endswith('.y'):
            masks[name[:-2] if name.endswith('.y') else name] = (a.t[:, :a.C].float().cpu() > 0).view(a.N, a.H, a.W, a.C).permute(0, 3, 1, 2)
    mom = {k: torch.zeros_like(v) for k, v in p.items()}
    total, data, grads = NR.train_step(q, mom, imgs, gt, 0.001, relu_masks=masks)
    print('fcos 80 classes: loss', loss, 'oracle', float(total))
    assert abs(loss - total) < 2e-3 * abs(total), (loss, total)
    for k in p:
        want = grads[k] - 1e-4 * p[k]
        if float(want.norm()) < 1e-7:
            continue
        err = float((m.get_param(k, m.G) - want).norm()) / float(want.norm())
        assert err < 1e-2, (k, err)
    # inference: lift the biases so that detections exist (tests/test_gpu_fcos_model.py)
    p = NR.init_params(19, num_classes=80)
    p['l79.b'] = p['l79.b'] + 4.0
    p['l80.b'] = p['l80.b'] + 4.0
    p['l85.w'] = p['l85.w'] * 0.05
    t = T._model('test', 1, nms_score_threshold=0.3, **kw)
    t.load_oracle_params(p)
    got = t.test_images(imgs.numpy())
    assert len(got) == 2
    with torch.no_grad():
        conf, reg, center = NR.forward(p, imgs, subtract_mean=False)
    for n in range(2):
        pconf, pbbox = FR.decode_candidates([c[n] for c in conf], [r[n] for r in reg], [z[n] for z in center])
        want = DC.per_class_nms(pconf, pbbox, 79, 0.3, 10, 0.45)
        print(f'fcos 80 classes image {n}: {len(want[0])} detections, classes up to {int(want[2].max()) if len(want[2]) else -1}')
        assert len(want[0]) > 0 and len(got[n][0]) == len(want[0])
        assert np.array_equal(got[n][2], want[2].numpy())
        np.testing.assert_allclose(got[n][0], want[0].numpy(), atol=2e-3)
        w = want[1].numpy()
        assert ((np.abs(got[n][1] - w) <= 2.0 + 5e-3 * np.abs(w)).all(axis=1)).mean() >= 0.95
    _coco_runs(t, [(imgs, gt)])


def _gap_threshold(conf, lo, hi):
    """a score threshold in [lo, hi] in the middle of the lowest gap of more than 2e-3 between neighbouring oracle confidences: no candidate flips on the
    engine's round-off (the model tests hold scores to 5e-4 .. 2e-3 of the oracle's)"""
    v = np.sort(conf[(conf > lo) & (conf < hi)])
    wide = np.nonzero(np.diff(v) > 4e-3)[0]
    assert wide.size > 0, v.size
    i = int(wide[0])
    return float((v[i] + v[i + 1]) / 2)


# ---- SSD300.  oracle/ssd300_ref.py builds its six heads 25 columns wide whatever the class count is (its loss, decode and detect take the count): the heads
# are restated here from the oracle's own convolution and batch norm on the oracle's feature maps.
def _ssd_head_params(p, seed, C):
    from oracle import ssd300_ref as R
    g = torch.Generator().manual_seed(seed)
    q = {k: v for k, v in p.items() if not k.startswith('pred')}
    for i, (ch, a) in enumerate(zip(R.FEAT_CH, R.ANCHORS_PER_CELL)):
        name, co = f'pred{i + 1}', a * (C + 4)
        q[name + '.w'] = torch.randn(co, 3, 3, ch, generator=g) * (2.0 / (ch * 9)) ** 0.5
        q[name + '.b'] = torch.zeros(co)
        q[name + '.gamma'], q[name + '.beta'] = torch.ones(co), torch.zeros(co)
        q[name + '.mmean'], q[name + '.mvar'] = torch.zeros(co), torch.ones(co)
    return q


def _ssd_forward(p25, q, imgs, training, C, stats=None, subtract_mean=True):
    """pred [N, 8828, C + 4]: the oracle's trunk (p25: the same trunk parameters with the oracle's own heads, whose output is dropped), then the heads of q"""
    from oracle import ssd300_ref as R
    taps = {}
    R.forward(dict(p25, **{k: v for k, v in q.items() if not k.startswith('pred')}), imgs, training, stats, taps=taps, subtract_mean=subtract_mean)
    preds = []
    for i, n in enumerate(['feat1'] + R.FEATS[1:]):
        name = f'pred{i + 1}'
        z = R.conv2d_same(taps[n].permute(0, 3, 1, 2), q[name + '.w'], q[name + '.b'])
        z = R.batch_norm(z, q, name, training, stats).permute(0, 2, 3, 1)
        preds.append(z.reshape(z.shape[0], -1, C + 4))
    return torch.cat(preds, dim=1)


def test_ssd300_with_80_classes(dev):
    """the bounds of tests/test_gpu_ssd300.py / test_gpu_ssd300_b32.py at num_classes = 80: predictions 1e-3 of the largest, data loss 2e-3, every gradient 3e-2
    (relative Frobenius); detections: classes equal, scores 5e-4, boxes 0.1 px"""
    import odtk
    from oracle import ssd300_ref as R
    torch.set_num_threads(16)
    C, B, wd = 81, 2, 1e-4
    cfg = {'mode': 'train', 'data_format': 'channels_last', 'num_classes': 80, 'weight_decay': wd, 'keep_prob': 0.5, 'batch_size': B,
           'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': '', 'verbose': False, 'use_graph': False,
           'compute_dtype': 'f32'}
    imgs, gt = R.synthetic_batch(B, 411)
    gt = _spread(gt)
    p25 = R.init_params(5)
    q = _ssd_head_params(p25, 6, C)
    prov = {'data_shape': [300, 300, 3], 'num_train': B, 'num_val': 0, 'train_generator': [(imgs, gt)], 'val_generator': None}
    m = odtk.SSD300(cfg, prov)
    assert m.num_classes == C and m.row == C + 4
    m.load_oracle_params(q)
    m.set_batch(imgs, gt)
    m._step_front()
    m._backward()
    torch.cuda.synchronize()
    names = [k for k in R.trainable_names(q)]
    for k in names:
        q[k].requires_grad_(True)
    pred_ref = _ssd_forward(p25, q, imgs, True, C)
    loss_ref = R.batch_loss(pred_ref, R.priors(), gt, C)
    loss_ref.backward()
    loss_ref = loss_ref.detach()
    pred = m.pred.float().cpu()[..., : C + 4]
    scale = max(1.0, float(pred_ref.detach().abs().max()))
    print('ssd300 80 classes: prediction error', float((pred - pred_ref.detach()).abs().max()), 'of', scale)
    assert float((pred - pred_ref.detach()).abs().max()) < 1e-3 * scale
    loss = float(m.loss_parts[:, 3].sum().item()) / B
    print('ssd300 80 classes: loss', loss, 'oracle', float(loss_ref))
    assert abs(loss - float(loss_ref)) <= 2e-3 * abs(float(loss_ref)), (loss, float(loss_ref))
    worst = ('', 0.0)
    for name in m.pinfo:
        if name.endswith('.b') and (name[:-2] + '.gamma') in q:
            continue                                   # a bias in front of a batch norm: exactly-zero gradient
        t = m.param(name, m.G)
        got = (t[..., : m.convs[name[:-2]].cin] if name.endswith('.w') else t).detach().float().cpu()
        want = q[name].grad.reshape(got.shape)
        err = float((got - want).norm()) / (float(want.norm()) + 1e-30)
        worst = max(worst, (name, err), key=lambda v: v[1])
        assert err < 3e-2, (name, err)
    print('ssd300 80 classes: worst relative gradient error', worst)
    assert np.isfinite(float(m.train_step(0.01)))
    # inference: moving statistics from a training-mode pass over the raw pixels (test mode feeds raw pixels: tests/test_gpu_ssd300.py)
    for k in names:
        q[k].requires_grad_(False)
        q[k].grad = None
    stats = {}
    with torch.no_grad():
        _ssd_forward(p25, q, imgs, True, C, stats, subtract_mean=False)
        for name, (mean, unb) in stats.items():
            if name + '.mmean' in q:
                q[name + '.mmean'], q[name + '.mvar'] = mean.clone(), unb.clone()
        pred_t = _ssd_forward(p25, q, imgs, False, C, subtract_mean=False)
    conf_all = np.concatenate([R.decode(pred_t[n], R.priors(), C)[0].numpy().ravel() for n in range(B)])
    thr = _gap_threshold(conf_all, 0.05, 0.5)
    t = odtk.SSD300(dict(cfg, mode='test', test_batch_size=2, nms_score_threshold=thr), None)
    t.load_oracle_params(q)
    got = t.test_images(imgs.numpy())
    assert len(got) == B
    total = 0
    for n in range(B):
        s_ref, b_ref, c_ref = (x.numpy() for x in R.detect(pred_t[n], R.priors(), thr, 20, 0.5, C))
        s, b, c = got[n]
        print(f'ssd300 80 classes image {n}: {len(s_ref)} detections at threshold {thr:.4f}, classes up to {int(c_ref.max()) if len(c_ref) else -1}')
        assert c.tolist() == c_ref.tolist()
        total += len(s_ref)
        if len(s_ref):
            assert float(np.abs(s - s_ref).max()) < 5e-4 and float(np.abs(b - b_ref).max()) < 0.1, (float(np.abs(s - s_ref).max()), float(np.abs(b - b_ref).max()))
    assert total > 0
    _coco_runs(t, [(imgs, gt)])


def test_retinanet_with_80_classes(dev):
    """the bounds of tests/test_gpu_retinanet_model.py at num_classes = 80, on its 160 x 160 images: predictions 2e-3, loss 2e-3, every gradient 5e-3; detections
    equal to the oracle's tail on the engine's own logits (scores 1e-5, boxes 0.05 px) and, against the free-running oracle, classes equal, scores 2e-3, 95 % of
    the boxes within 2 px + 5e-3.  oracle/retinanet_ref.batch_loss fixes 21 classes: the batch mean of one_image_loss(num_classes=81) stands in for it."""
    import test_gpu_retinanet_model as T
    from oracle import detect_common as DC
    NR, RR = T.NR, T.RR
    torch.set_num_threads(16)
    C, size = 81, 160            # (at 128 x 128 the coarsest level is one cell: batch statistics over two values; 160 is the 20-class test's size)
    imgs, gt = T._batch(2, size, 90)
    gt = _spread(gt)
    p = NR.init_params(7, num_classes=C)
    m = T._model('train', 'f32', 2, size, T._provider([(imgs, gt)]), num_classes=80)
    assert tuple(m.pconf.shape[2:]) == (C,)
    m.load_oracle_params(p)
    m.set_batch(imgs, gt)
    loss = float(m.train_step(0.01).item())
    masks = {}
    for name, *_ in NR.layer_specs(num_classes=C):
        a = m.acts[name if name == 'l0' else name + '.y']
        masks[name] = (a.t[:, :a.C].float().cpu() > 0).view(a.N, a.H, a.W, a.C).permute(0, 3, 1, 2)
    q = {k: v.clone() for k, v in p.items()}
    names = NR.trainable_names(q)
    for k in names:
        q[k].requires_grad_(True)
    pc, pb = NR.forward(q, imgs, True, relu_masks=masks)
    anc = RR.anchors([size, size, 3], RR.pyramid_shapes(size, size))
    data = sum(RR.one_image_loss(pb[i, :, :2], pb[i, :, 2:], pc[i], anc, gt[i], 0.25, 2.0, num_classes=C) for i in range(2)) / 2
    total = data + 1e-4 * sum((q[k] ** 2).sum() / 2 for k in names)
    total.backward()
    e_conf, e_box = float((m.pconf.cpu() - pc.detach()).abs().max()), float((m.pbox.cpu() - pb.detach()).abs().max())
    print(f'retinanet 80 classes: prediction error class {e_conf:.3e}, box {e_box:.3e}; loss {loss} oracle {float(total)}')
    assert e_conf < 2e-3 * (float(pc.abs().max()) + 1) and e_box < 2e-3 * (float(pb.abs().max()) + 1)
    assert abs(loss - float(total)) < 2e-3 * abs(float(total)), (loss, float(total))
    worst = ('', 0.0)
    for k in names:
        if k == 'l0.b':
            continue
        got, want = m.get_param(k, m.G), q[k].grad - 1e-4 * p[k]
        if k.endswith('.b') and float(want.norm()) < 1e-4 * float(q[k[:-2] + '.w'].grad.norm()):
            continue                                   # a bias in front of a batch norm: both sides hold round-off
        err = float((got - want).norm()) / (float(want.norm()) + 1e-8)
        worst = max(worst, (k, err), key=lambda v: v[1])
        assert err < 5e-3, (k, err)
    print('retinanet 80 classes: worst relative gradient error', worst)
    # inference (tests/test_gpu_retinanet_model.py::test_f32_inference_detections_equal_oracle)
    p = NR.init_params(13, num_classes=C)
    stats = {}
    with torch.no_grad():
        NR.forward(p, imgs + 20 * torch.randn(imgs.shape, generator=torch.Generator().manual_seed(2)), True, stats, subtract_mean=False)
    for k, (mean, var) in stats.items():
        p[k + '.mmean'], p[k + '.mvar'] = mean.clone(), var.clone()
    for i in (81, 91, 101, 111, 121):
        p[f'l{i}.w'] = p[f'l{i}.w'] * 0.02
    with torch.no_grad():
        pc, pb = NR.forward(p, imgs, False, subtract_mean=False)
    kept = [RR.decode_candidates(pb[n, :, :2], pb[n, :, 2:], pc[n], anc, 0.0, num_classes=C) for n in range(2)]
    conf_all = np.concatenate([c[k].numpy().ravel() for c, _, k, _ in kept])
    thr = _gap_threshold(conf_all, 0.04, 0.5)
    t = T._model('test', 'f32', 1, size, num_classes=80, test_batch_size=2, nms_score_threshold=thr)
    t.load_oracle_params(p)
    got = t.test_images(imgs.numpy())
    assert len(got) == 2
    total = 0
    assert float((t.pconf.cpu() - pc).abs().max()) < 2e-3 * (float(pc.abs().max()) + 1)
    for n in range(2):
        conf, boxes, keep, _ = RR.decode_candidates(pb[n, :, :2], pb[n, :, 2:], pc[n], anc, thr, num_classes=C)
        want = DC.per_class_nms(conf, boxes, 80, thr, 10, 0.45, row_mask=keep)
        pc_e, pb_e = t.pconf.cpu()[n], t.pbox.cpu()[n]
        conf_e, boxes_e, keep_e, _ = RR.decode_candidates(pb_e[:, :2], pb_e[:, 2:], pc_e, anc, thr, num_classes=C)
        same = DC.per_class_nms(conf_e, boxes_e, 80, thr, 10, 0.45, row_mask=keep_e)
        print(f'retinanet 80 classes image {n}: {len(want[0])} detections at threshold {thr:.4f}, classes up to {int(want[2].max()) if len(want[2]) else -1}')
        assert len(got[n][0]) == len(same[0]) == len(want[0])
        total += len(want[0])
        if len(want[0]) == 0:
            continue
        assert np.array_equal(got[n][2], same[2].numpy()) and np.array_equal(got[n][2], want[2].numpy())
        np.testing.assert_allclose(got[n][0], same[0].numpy(), atol=1e-5)
        assert float(np.abs(got[n][1] - same[1].numpy()).max()) <= 0.05 + 1e-5 * float(np.abs(same[1].numpy()).max())
        np.testing.assert_allclose(got[n][0], want[0].numpy(), atol=2e-3)
        w = want[1].numpy()
        assert ((np.abs(got[n][1] - w) <= 2.0 + 5e-3 * np.abs(w)).all(axis=1)).mean() >= 0.95
    assert total > 0
    _coco_runs(t, [(imgs, gt)])
