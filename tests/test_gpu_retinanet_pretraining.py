"""RetinaNet classification pre-training (`is_pretraining: True`, RetinaNet.py:120-135) on the MI355X:
  * the head kernels (odtk_gap_softmax_ce_fwd / _bwd) against float64 torch -- the same bodies run on the CPU through the emulation of the
    kernel source (tests/test_cpu_retinanet_pretrain.py);
  * one training step of the class (exact f32 engine at 128 x 128 / batch 4 from the fixture's parameters, f32 and f32x3 at the ImageNet geometry
    224 x 224 / batch 8) against tests/retinanet_pretrain_ref.py, which tests/golden/retinanet_pretrain.npz pins on the reference's own class;
  * the class surface (train_one_epoch, test_one_image), the hand-over of a saved backbone to a detection model in both checkpoint formats,
    and run-to-run bit equality."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, 'golden')
DEV = 'cuda:0'
GRAD_X3 = 1e-2         # f32x3 (bf16 products by operand splitting) against the restatement at 224 x 224 / batch 8, measured: gradient median 1.5e-4,
                       # worst 1.6e-3 (l0.gamma), update worst 1.7e-3 (exact-f32 engine: 7.1e-5 / 1.3e-3 / 1.4e-3)

import retinanet_pretrain_ref as PR      # noqa: E402

CONFIG = {'is_bottleneck': True, 'residual_block_list': [3, 4, 6, 3], 'init_conv_filters': 16, 'mode': 'train', 'is_pretraining': True,
          'data_shape': [128, 128, 3], 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'data_format': 'channels_last', 'batch_size': 4,
          'gamma': 2.0, 'alpha': 0.25, 'nms_score_threshold': 0.8, 'nms_max_boxes': 10, 'nms_iou_threshold': 0.45, 'verbose': False}


# ------------------------------------------------------------------------------------------------ head kernels
def _bf16_ulp(v):
    a = v.abs().clamp_min(1e-30)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def check_head_kernels(dev, dt, N, HW, C, ld, seed):
    """odtk_gap_softmax_ce_fwd / _bwd on rows [N * HW][ld] of `dt` against float64: logits and loss 1e-6 (relative to the image's logit scale),
    dx 1e-6 (f32) / one bf16 ulp (bf16), pred / correct exact (first index on a constructed tie), pad columns of dx zero, accumulate,
    inference call (no labels), and bit equality on a second run"""
    from odtk import ops
    tdt = torch.float32 if dt == 'f32' else torch.bfloat16
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N * HW, ld, generator=g) * 2
    x[:, C:] = 1e4                                                    # pad columns: never read
    a, b = (5, 69) if C > 69 else (1, 2)                              # image 0: a tie between two channels (two waves when C > 69) above the rest
    r0 = slice(0, HW)
    x[r0, a] = x[r0, a] + 30
    x[r0, b] = x[r0, a]
    labels = torch.randint(0, C, (N,), generator=g, dtype=torch.int32)
    labels[0] = a
    if N > 1:
        labels[1] = 0
    if N != 2:
        labels[-1] = C - 1
    xs = x.to(tdt)
    xd = xs.double()[:, :C].view(N, HW, C)
    z = xd.sum(1) / HW
    lse = torch.logsumexp(z, 1)
    loss_ref = lse - z.gather(1, labels.long().view(-1, 1)).squeeze(1)
    gs = 1.0 / N
    dlog_ref = (torch.softmax(z, 1) - torch.nn.functional.one_hot(labels.long(), C).double()) * gs
    dx_ref = (dlog_ref / HW).repeat_interleave(HW, 0)
    pred_ref = z.argmax(1)
    assert int(pred_ref[0]) == a

    def run():
        xg, lg = xs.to(dev), labels.to(dev)
        out = dict(logits=torch.full((N, C), 7., device=dev), loss=torch.full((N,), 7., device=dev), pred=torch.full((N,), -1, dtype=torch.int32, device=dev),
                   correct=torch.full((N,), 7., device=dev), dlogits=torch.full((N, C), 7., device=dev))
        ops.gap_softmax_ce_fwd(xg, ld, N, HW, C, lg, gs, out['logits'], out['loss'], out['pred'], out['correct'], out['dlogits'])
        dx = torch.full((N * HW, ld), 3., dtype=tdt, device=dev)
        ops.gap_softmax_ce_bwd(out['dlogits'], N, HW, C, dx, ld, False)
        acc0 = (torch.randn(N * HW, ld, generator=g)).to(tdt)
        acc = acc0.to(dev)
        ops.gap_softmax_ce_bwd(out['dlogits'], N, HW, C, acc, ld, True)
        inf = dict(logits=torch.zeros(N, C, device=dev), pred=torch.full((N,), -1, dtype=torch.int32, device=dev))
        ops.gap_softmax_ce_fwd(xg, ld, N, HW, C, None, 0., inf['logits'], None, inf['pred'], None, None)
        torch.cuda.synchronize()
        out = {k: v.cpu() for k, v in out.items()}
        return out, dx.cpu(), acc0, acc.cpu(), {k: v.cpu() for k, v in inf.items()}
    out, dx, acc0, acc, inf = run()
    scale = z.abs().amax(1)
    e_logit = float(((out['logits'].double() - z).abs().amax(1) / scale).max())
    e_loss = float(((out['loss'].double() - loss_ref).abs() / torch.maximum(loss_ref.abs(), scale)).max())
    print(f'{dt} N={N} HW={HW} C={C} ld={ld}: logits {e_logit:.2e}, loss {e_loss:.2e} (relative to the logit scale)')
    assert e_logit < 1e-6 and e_loss < 1e-6, (e_logit, e_loss)
    assert torch.equal(out['pred'].long(), pred_ref) and torch.equal(out['pred'].long(), out['logits'].argmax(1))
    assert torch.equal(out['correct'], (pred_ref == labels.long()).float())
    e_dlog = float((out['dlogits'].double() - dlog_ref).abs().max()) / float(dlog_ref.abs().max())
    assert e_dlog < 1e-6, e_dlog
    assert torch.equal(dx[:, C:].float(), torch.zeros(N * HW, ld - C)) and torch.equal(acc[:, C:].float(), torch.zeros(N * HW, ld - C))
    want_acc = acc0[:, :C].double() + dx_ref
    if dt == 'f32':
        e_dx = float((dx[:, :C].double() - dx_ref).abs().max()) / float(dx_ref.abs().max())
        e_acc = float((acc[:, :C].double() - want_acc).abs().max()) / float(want_acc.abs().max())
        assert e_dx < 1e-6 and e_acc < 1e-6, (e_dx, e_acc)
    else:
        assert bool(((dx[:, :C].double() - dx_ref).abs() <= _bf16_ulp(dx_ref)).all()), 'dx: one bf16 ulp'
        assert bool(((acc[:, :C].double() - want_acc).abs() <= _bf16_ulp(want_acc)).all()), 'accumulated dx: one bf16 ulp'
    assert torch.equal(inf['logits'], out['logits']) and torch.equal(inf['pred'], out['pred'])
    out2, dx2, _, _, _ = run()
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    assert torch.equal(dx, dx2)


HEAD_CASES = [(4, 49, 224, 224, 1), (1, 1, 224, 232, 2), (3, 49, 100, 112, 3), (2, 16, 1024, 1024, 4), (5, 49, 7, 16, 5)]


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('N,HW,C,ld,seed', HEAD_CASES)
def test_head_kernels_against_f64(dt, N, HW, C, ld, seed):
    check_head_kernels(DEV, dt, N, HW, C, ld, seed)


def test_head_rejects_unsupported_width():
    from odtk import _lib, ops
    x = torch.zeros(2, 1040, device=DEV)
    with pytest.raises(_lib.OdtkError):
        ops.gap_softmax_ce_fwd(x, 1040, 2, 1, 1040, None, 0., torch.zeros(2, 1040, device=DEV), None, torch.zeros(2, dtype=torch.int32, device=DEV),
                               None, None)


# ------------------------------------------------------------------------------------------------ the class
def _images(seed, n, size):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, size, size, 3, generator=g) * 255).round()


def _model(mode='train', dtype='f32', batch=4, size=128, provider=None, **kw):
    import odtk
    return odtk.RetinaNet(dict(CONFIG, mode=mode, compute_dtype=dtype, batch_size=batch, data_shape=[size, size, 3], **kw), provider)


def _provider(batches):
    return {'num_train': sum(b[0].shape[0] for b in batches), 'num_val': 0, 'train_generator': batches, 'val_generator': None}


def _rel(a, b):
    return float((a - b).norm()) / (float(b.norm()) + 1e-12)


def _step_against_restatement(p, imgs, labels, engine, size):
    """one train_step of the class from parameters p against tests/retinanet_pretrain_ref.train_step on the ReLU region the GPU took"""
    torch.set_num_threads(16)
    B = imgs.shape[0]
    m = _model('train', engine, B, size, _provider([(imgs, labels)]))
    m.load_oracle_params(p)
    m.set_batch(imgs, labels)
    loss = float(m.train_step(0.01).item())
    acc = float(m.last_accuracy.item())
    masks = {}
    for name, *_ in PR.specs():
        a = m.acts[name if name == 'l0' else name + '.y']
        masks[name] = (a.t[:, :a.C].float().cpu() > 0).view(a.N, a.H, a.W, a.C).permute(0, 3, 1, 2)
    q = {k: v.clone() for k, v in p.items()}
    mom = {k: torch.zeros_like(p[k]) for k in PR.trainable_names(p)}
    total, ce, acc_ref, grads, logits = PR.train_step(q, mom, imgs, labels, 0.01, relu_masks=masks)
    e_logits = float((m.logits.cpu() - logits).abs().max()) / float(logits.abs().max())
    errs, worst = [], ('', 0.)
    for k in PR.trainable_names(p):
        want = grads[k] - 1e-4 * p[k]
        got = m.get_param(k, m.G)
        if k.endswith('.b') and float(want.norm()) < 1e-4 * float(grads[k[:-2] + '.w'].norm()):
            # a conv output that ends in a batch norm (directly or through a sum): the true bias gradient is 0, both sides hold round-off
            assert float(got.norm()) < 1e-3 * float(grads[k[:-2] + '.w'].norm()), k
            continue
        errs.append(_rel(got, want))
        worst = max(worst, (k, errs[-1]), key=lambda t: t[1])
    errs.sort()
    after = m.export_params()
    step_errs = []
    for k in PR.trainable_names(p):
        if k.endswith('.b') and float((grads[k] - 1e-4 * p[k]).norm()) < 1e-4 * float(grads[k[:-2] + '.w'].norm()):
            continue
        step = q[k] - p[k]
        step_errs.append((_rel(after[k] - p[k], step), k))
    stats_frozen = all(bool((after[k] == (0. if k.endswith('.mmean') else 1.)).all()) for k in after if k.endswith(('.mmean', '.mvar')))
    print(f'{engine} {size}x{size} b{B}: loss {loss:.6f} vs {total:.6f}, logits {e_logits:.2e}, gradient median {errs[len(errs) // 2]:.2e} worst {worst}, '
          f'step worst {max(step_errs)}, accuracy {acc} vs {acc_ref}')
    return dict(m=m, loss=loss, total=total, acc=acc, acc_ref=acc_ref, errs=errs, worst=worst, step_worst=max(step_errs)[0], frozen=stats_frozen,
                e_logits=e_logits, pred=m.pred.cpu().long(), pred_ref=logits.argmax(1))


def test_f32_step_matches_fixture_and_restatement_128():
    g = np.load(os.path.join(GOLD, 'retinanet_pretrain.npz'))
    p = PR.init_params(37)
    imgs, labels = _images(int(g['image_seeds'][0]), 4, 128), torch.from_numpy(g['labels'][0])
    r = _step_against_restatement(p, imgs, labels, 'f32', 128)
    assert abs(r['loss'] - float(g['losses'][0])) < 2e-3 * float(g['losses'][0]), (r['loss'], g['losses'])
    assert abs(r['loss'] - r['total']) < 2e-3 * abs(r['total'])
    assert r['acc'] == float(g['accuracy'][0]) == r['acc_ref']
    assert torch.equal(r['pred'], torch.from_numpy(g['pred0']))
    assert r['worst'][1] < 5e-3 and r['step_worst'] < 5e-3, (r['worst'], r['step_worst'])
    assert r['frozen'], 'the moving statistics must stay exactly 0 / 1'
    # (the fixture's parameters after the step come from the FREE-RUNNING reference: a few ReLU signs the GPU takes differently move the stem's
    # step by ~1.5 % at this size, so the update is held to the restatement on the GPU's own ReLU region above; the restatement is pinned on the
    # fixture's parameters on the CPU, tests/test_cpu_retinanet_pretrain.py)


@pytest.mark.parametrize('engine', ['f32', 'f32x3'])
def test_step_matches_restatement_224_batch8(engine):
    # the ImageNet geometry: a 7 x 7 final map; every layer of the backbone at this size must dispatch to a supported kernel
    p = PR.init_params(41)
    imgs = _images(800, 8, 224)
    labels = torch.tensor([0, 223, 5, 77, 150, 199, 1, 222], dtype=torch.int32)
    r = _step_against_restatement(p, imgs, labels, engine, 224)
    assert r['m'].feat.H == r['m'].feat.W == 7 and r['m'].feat.C == 224
    assert r['frozen'] and r['acc'] == r['acc_ref'] and torch.equal(r['pred'], r['pred_ref'])
    if engine == 'f32':
        assert abs(r['loss'] - r['total']) < 2e-3 * abs(r['total'])
        assert r['worst'][1] < 5e-3 and r['step_worst'] < 5e-3, (r['worst'], r['step_worst'])
    else:
        assert abs(r['loss'] - r['total']) < 4 * 2e-3 * abs(r['total'])
        assert r['worst'][1] < GRAD_X3 and r['errs'][len(r['errs']) // 2] < GRAD_X3 / 2 and r['step_worst'] < GRAD_X3, (r['worst'], r['step_worst'])


def test_train_one_epoch_and_test_one_image():
    torch.set_num_threads(16)
    g = np.load(os.path.join(GOLD, 'retinanet_pretrain.npz'))
    p = PR.init_params(37)
    batches = [(_images(int(g['image_seeds'][s]), 4, 128), g['labels'][s].copy()) for s in range(2)]
    a = _model('train', 'f32', 4, 128, _provider(batches))
    a.load_oracle_params(p)
    loss, acc = a.train_one_epoch(0.01)
    assert isinstance(loss, (float, np.floating)) and isinstance(acc, (float, np.floating))
    b = _model('train', 'f32', 4, 128, _provider(batches))
    b.load_oracle_params(p)
    ls, accs = [], []
    for imgs, lab in batches:
        b.set_batch(imgs, lab)
        ls.append(float(b.train_step(0.01).item()))
        accs.append(float(b.last_accuracy.item()))
    assert loss == np.mean(ls) and acc == np.mean(accs), (loss, ls, acc, accs)
    assert a.global_step == 2 and abs(ls[0] - float(g['losses'][0])) < 2e-3 * float(g['losses'][0]) and accs[0] == float(g['accuracy'][0])
    # test mode: the fixture's image through the initial parameters, moving statistics 0 / 1, the fed pixels bypass the mean subtraction
    t = _model('test', 'f32', 1, 128)
    t.load_oracle_params(p)
    img = _images(int(g['test_image_seed']), 1, 128)
    pred = t.test_one_image(img.numpy())
    assert pred.dtype == np.int64 and pred.shape == (1,)
    assert int(pred[0]) == int(g['test_pred'][0])
    np.testing.assert_allclose(t.logits.cpu().numpy()[0], g['test_logits'], rtol=0, atol=2e-5 * float(np.abs(g['test_logits']).max()))
    t2 = _model('test', 'f32', 1, 128, data_format='channels_first')
    t2.load_oracle_params(p)
    assert np.array_equal(t2.test_one_image(img.permute(0, 3, 1, 2).numpy()), pred)


@pytest.mark.parametrize('fmt', ['tf', 'torch'])
def test_pretrained_backbone_hands_over_to_a_detection_model(tmp_path, fmt):
    torch.set_num_threads(16)
    import odtk
    batches = [(_images(900 + s, 2, 128), np.asarray([3 * s, 223 - s])) for s in range(2)]
    pre = _model('train', 'f32', 2, 128, _provider(batches), checkpoint_format=fmt, seed=5)
    loss, acc = pre.train_one_epoch(0.01)
    assert np.isfinite(loss)
    pre.save_weight('latest', str(tmp_path / 'pre' / 'model'))
    path = str(tmp_path / 'pre' / 'model-2')
    assert os.path.exists(path + '.index') == (fmt == 'tf')
    det_cfg = dict(CONFIG, is_pretraining=False, batch_size=2, compute_dtype='f32', seed=9)
    from oracle import retinanet_ref as RR
    gt = RR.synthetic_gt(2, 128, 77)
    det = odtk.RetinaNet(det_cfg, _provider([(_images(910, 2, 128), gt)]))
    before = det.export_params()
    det.load_pretraining_weight(path)
    after = det.export_params()
    for k in after:
        layer = int(k[1:].split('.')[0])
        if layer < 65 and k in pre.pinfo:
            assert torch.equal(after[k], pre.get_param(k)), k
        else:
            assert torch.equal(after[k], before[k]), k
    det.set_batch(_images(910, 2, 128), gt)
    assert np.isfinite(float(det.train_step(0.01).item()))
    # the pre-training model reads its own file back
    back = _model('train', 'f32', 2, 128, _provider(batches), seed=6)
    back.load_weight(path)
    for k in pre.pinfo:
        assert torch.equal(back.get_param(k), pre.get_param(k)), k


def test_two_identical_steps_are_bit_identical():
    p = PR.init_params(43)
    imgs, labels = _images(950, 4, 128), np.asarray([1, 2, 223, 0])
    out = []
    for _ in range(2):
        m = _model('train', 'f32x3', 4, 128, _provider([(imgs, labels)]))
        m.load_oracle_params(p)
        m.set_batch(imgs, labels)
        loss = m.train_step(0.01).clone()
        torch.cuda.synchronize()
        out.append((m.P.clone(), m.Mom.clone(), loss, m.logits.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_data_parallel_is_refused():
    m = _model('train', 'f32', 2, 128, _provider([(_images(1, 2, 128), np.asarray([0, 1]))]))
    with pytest.raises(NotImplementedError):
        m.attach_data_parallel()
