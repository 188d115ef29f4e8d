"""RetinaNet classification pre-training (`is_pretraining: True`) without a GPU:
  * the head kernels' SOURCE (csrc/retina.hip: odtk_gap_softmax_ce_fwd / _bwd) run through the CPU emulation of the HIP execution model
    (tests/hip_cpu_backend.py) by the GPU test body, against float64;
  * tests/retinanet_pretrain_ref.py (the torch restatement) against the reference's own pre-training graph (tests/golden/retinanet_pretrain.npz);
  * the class's host logic with every launch replaced by a torch stand-in (tests/mock_ops.py, plus stand-ins of the two head wrappers here):
    graph, one step, frozen moving statistics, surface, checkpoints in both formats and their hand-over to a detection model.
(The file name sorts before test_hip_cpu.py on purpose: that file's last test checks that every entry point of the emulated build ran in the
process, and the two head entry points run here.)"""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, 'golden')
import hip_cpu_backend as HC             # noqa: E402
import mock_ops                          # noqa: E402
import retinanet_pretrain_ref as PR      # noqa: E402
import test_gpu_retinanet_pretraining as G   # noqa: E402


def _images(seed, n, size):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, size, size, 3, generator=g) * 255).round()


def _rel(a, b):
    return float((a - b).norm()) / (float(b.norm()) + 1e-12)


# ------------------------------------------------------------------------------------------------ kernel source through the emulation
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('N,HW,C,ld,seed', G.HEAD_CASES)
def test_head_kernels_from_source(dt, N, HW, C, ld, seed):
    with HC.installed():
        G.check_head_kernels('cpu', dt, N, HW, C, ld, seed)


# ------------------------------------------------------------------------------------------------ restatement vs the reference's class
def test_restatement_matches_reference_pretraining_graph():
    torch.set_num_threads(8)
    g = np.load(os.path.join(GOLD, 'retinanet_pretrain.npz'))
    p = PR.init_params(37)
    assert len(PR.specs()) == 65 and len(PR.trainable_names(p)) == 260
    with torch.no_grad():
        tl = PR.forward(p, _images(int(g['test_image_seed']), 1, 128), False, subtract_mean=False)
    assert float((tl[0] - torch.from_numpy(g['test_logits'])).abs().max()) < 1e-5 * float(np.abs(g['test_logits']).max())
    assert int(tl.argmax(1)[0]) == int(g['test_pred'][0])
    mom = {k: torch.zeros_like(p[k]) for k in PR.trainable_names(p)}
    for s in range(2):
        total, _, acc, _, logits = PR.train_step(p, mom, _images(int(g['image_seeds'][s]), 4, 128), torch.from_numpy(g['labels'][s]), 0.01)
        assert abs(total - g['losses'][s]) < 1e-5 * g['losses'][s], (s, total, g['losses'])
        assert acc == g['accuracy'][s]
        if s:
            continue
        assert float((logits - torch.from_numpy(g['logits0'])).abs().max()) < 1e-5 * float(np.abs(g['logits0']).max())
        assert torch.equal(logits.argmax(1), torch.from_numpy(g['pred0']))
        for key in g.files:
            if '__' in key:
                k = key.replace('__', '.')
                got = p[k].reshape(-1)
                got = got[::max(1, got.numel() // 512)].numpy()
                assert np.linalg.norm(got - g[key]) < 1e-4 * np.linalg.norm(g[key]) + 1e-8, k


def test_fixture_variables_are_the_backbone_of_the_detection_graph():
    from odtk.retinanet import reference_variable_map
    pre = json.load(open(os.path.join(GOLD, 'retinanet_pretrain_variables.json')))
    det = json.load(open(os.path.join(GOLD, 'retinanet_variables.json')))
    vm = reference_variable_map()
    names = [n for n in pre if n != 'global_step']
    assert len(names) == 390 and sum(v['trainable'] for v in pre.values()) == 260
    for n in names:
        assert int(vm[n][1:].split('.')[0]) < 65 and pre[n]['shape'] == det[n]['shape'], n


# ------------------------------------------------------------------------------------------------ host logic of the class (mocked launches)
def _gap_fwd(x, ldx, N, HW, C_, labels, grad_scale, logits, loss, pred, correct, dlogits):
    z = x[:, :C_].float().reshape(N, HW, C_).sum(1) / HW
    logits.copy_(z)
    pred.copy_(z.argmax(1).to(pred.dtype))
    if labels is not None:
        lab = labels.long()
        loss.copy_(torch.logsumexp(z, 1) - z.gather(1, lab.view(-1, 1)).squeeze(1))
        correct.copy_((pred.long() == lab).float())
        if dlogits is not None:
            dlogits.copy_((torch.softmax(z, 1) - F.one_hot(lab, C_).float()) * grad_scale)


def _gap_bwd(dlogits, N, HW, C_, dx, lddx, accumulate=False):
    v = (dlogits / HW).repeat_interleave(HW, 0)
    if accumulate:
        v = v + dx[:, :C_].float()
    dx[:, :C_] = v.to(dx.dtype)
    dx[:, C_:] = 0


@pytest.fixture()
def mocked(monkeypatch):
    import odtk  # noqa: F401
    from odtk import ops
    with mock_ops.installed():
        monkeypatch.setattr(ops, 'gap_softmax_ce_fwd', _gap_fwd)
        monkeypatch.setattr(ops, 'gap_softmax_ce_bwd', _gap_bwd)
        yield


def _cfg(**kw):
    return dict(G.CONFIG, compute_dtype='f32', device='cpu', **kw)


def _provider(batches):
    return {'num_train': sum(b[0].shape[0] for b in batches), 'num_val': 0, 'train_generator': batches, 'val_generator': None}


def test_pretraining_class_host_logic(mocked):
    import odtk
    torch.set_num_threads(8)
    g = np.load(os.path.join(GOLD, 'retinanet_pretrain.npz'))
    p = PR.init_params(37)
    imgs, labels = _images(int(g['image_seeds'][0]), 4, 128), g['labels'][0].copy()
    m = odtk.RetinaNet(_cfg(), _provider([(imgs, labels)]))
    assert sorted({k.split('.')[0] for k in m.pinfo}, key=lambda s: int(s[1:])) == [f'l{i}' for i in range(65)]
    assert len(m.pinfo) == 260 and m.num_pretraining_classes == 224 and m.feat.H == m.feat.W == 4
    assert not any(op[0] in ('pred', 'resize_add') for op in m.plan) and m.plan[-1][0] == 'gap'
    with pytest.raises(ValueError):
        m.set_batch(imgs, np.asarray([0, 1, 2, 224]))
    with pytest.raises(ValueError):
        m.set_batch(imgs, np.asarray([0, -1, 2, 3]))
    m.load_oracle_params(p)
    m.set_batch(imgs, labels)
    loss = float(m.train_step(0.01))
    assert float(m.last_accuracy) == float(g['accuracy'][0])
    masks = {}
    for name, *_ in PR.specs():
        a = m.acts[name if name == 'l0' else name + '.y']
        masks[name] = (a.t[:, :a.C] > 0).view(a.N, a.H, a.W, a.C).permute(0, 3, 1, 2)
    q = {k: v.clone() for k, v in p.items()}
    mom = {k: torch.zeros_like(p[k]) for k in PR.trainable_names(p)}
    total, _, acc, grads, _ = PR.train_step(q, mom, imgs, torch.from_numpy(labels), 0.01, relu_masks=masks)
    assert abs(loss - total) < 1e-4 * abs(total) and abs(loss - float(g['losses'][0])) < 1e-4 * float(g['losses'][0])
    live_bias = []
    for k in PR.trainable_names(p):
        want = grads[k] - 1e-4 * p[k]
        if k.endswith('.b') and float(want.norm()) < 1e-4 * float(grads[k[:-2] + '.w'].norm()):
            continue
        live_bias += [k] if k.endswith('.b') else []
        assert _rel(m.get_param(k, m.G), want) < 5e-3, k
    assert live_bias == ['l63.b', 'l64.b']              # the last unit's two convs: no batch norm behind them, the pool is linear
    after = m.export_params()
    for k in PR.trainable_names(p):
        assert _rel(after[k], q[k]) < 1e-4, k
    for k in m.sinfo:                                    # RetinaNet.py:134: no moving-statistic update in this graph
        assert torch.equal(after[k], torch.zeros_like(after[k]) if k.endswith('.mmean') else torch.ones_like(after[k])), k


def test_pretraining_surface_and_checkpoints(mocked, tmp_path):
    import odtk
    from odtk.tf_checkpoint import NewCheckpointReader
    torch.set_num_threads(8)
    batches = [(_images(60 + s, 2, 64), np.asarray([s, 223 - s], np.int64)) for s in range(2)]
    with pytest.raises(ValueError):
        odtk.RetinaNet(_cfg(batch_size=2, data_shape=[64, 64, 3]), _provider(batches)).set_batch(batches[0][0], np.asarray([0.5, 1.]))
    pre_vars = json.load(open(os.path.join(GOLD, 'retinanet_pretrain_variables.json')))
    trainable = sorted(n for n, v in pre_vars.items() if v['trainable'])
    for fmt in ('tf', 'torch'):
        m = odtk.RetinaNet(_cfg(batch_size=2, data_shape=[64, 64, 3], checkpoint_format=fmt, seed=3), _provider(batches))
        out = m.train_one_epoch(0.01)
        assert isinstance(out, tuple) and len(out) == 2 and all(np.isfinite(v) for v in out) and m.global_step == 2
        with pytest.raises(NotImplementedError):
            m.attach_data_parallel()
        m.save_weight('latest', str(tmp_path / fmt / 'model'))
        path = str(tmp_path / fmt / 'model-2')
        if fmt == 'tf':
            names = sorted(NewCheckpointReader(path).get_variable_to_shape_map())
            assert names == trainable and len(names) == 260
            for n in names:
                assert list(NewCheckpointReader(path).get_tensor(n).shape) == pre_vars[n]['shape'], n
        else:
            blob = torch.load(path, weights_only=True)
            assert blob['pretraining'] and sorted(blob['params']) == sorted(m.pinfo) and blob['global_step'] == 2
        det = odtk.RetinaNet(dict(_cfg(batch_size=2, data_shape=[128, 128, 3], seed=8), is_pretraining=False), _provider([]))
        before = det.export_params()
        det.load_pretraining_weight(path)
        after = det.export_params()
        for k in after:
            if int(k[1:].split('.')[0]) < 65 and k in m.pinfo:
                assert torch.equal(after[k], m.get_param(k)), k
            else:
                assert torch.equal(after[k], before[k]), k
        back = odtk.RetinaNet(_cfg(batch_size=2, data_shape=[64, 64, 3], seed=4), _provider(batches))
        back.load_weight(path)
        for k in m.pinfo:
            assert torch.equal(back.get_param(k), m.get_param(k)), k
        assert torch.equal(back.S, m.S)
        if fmt == 'torch':
            assert torch.equal(back.Mom, m.Mom) and back.global_step == 2
    t = odtk.RetinaNet(_cfg(mode='test', data_shape=[64, 64, 3]), None)
    pred = t.test_one_image(_images(70, 1, 64).numpy())
    assert pred.dtype == np.int64 and pred.shape == (1,) and 0 <= int(pred[0]) < 224
    with torch.no_grad():
        want = PR.forward(t.export_params(), _images(70, 1, 64), False, subtract_mean=False).argmax(1)
    assert int(pred[0]) == int(want[0])
