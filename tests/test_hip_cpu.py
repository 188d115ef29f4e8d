"""The kernel SOURCE of csrc/lhrcnn.hip (and the geometry kernels of csrc/augment.hip) executed on the CPU (tests/hip_cpu_backend.py: g++ build against an emulation
of the HIP execution model -- fibers per thread, lock-step at barriers / shuffles / ballots) through the test bodies written for the GPU (tests/test_gpu_lhrcnn.py:
the functions are called directly with their device switched to the CPU).  No GPU needed: this is the `-m "not gpu"` tier's check of what the kernels compute."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hip_cpu_backend as HC  # noqa: E402


@pytest.fixture(scope='module')
def G():
    import test_gpu_lhrcnn as mod
    old = mod.DEV
    mod.DEV = 'cpu'
    yield mod
    mod.DEV = old


def test_emulated_build_exports_the_entry_points():
    lib = HC.build()
    for n in ('odtk_depthwise_conv', 'odtk_depthwise_wgrad', 'odtk_lhrcnn_match', 'odtk_lhrcnn_rpn_loss', 'odtk_crop_and_resize_fwd', 'odtk_crop_and_resize_bwd',
              'odtk_lhrcnn_rcnn_loss', 'odtk_lhrcnn_rpn_decode', 'odtk_lhrcnn_gather_rois', 'odtk_lhrcnn_rcnn_decode', 'odtk_augment_boxes', 'odtk_augment_images'):
        assert hasattr(lib, n), n


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('kh,kw,C,H,W', [(3, 3, 144, 20, 26), (1, 15, 64, 5, 13), (15, 1, 36, 10, 4), (3, 3, 23, 9, 6)])
def test_depthwise_kernels_from_source(G, kh, kw, C, H, W, dt):
    with HC.installed():
        G.test_depthwise_kernels(kh, kw, C, H, W, dt)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_crop_and_resize_kernels_from_source(G, dt):
    with HC.installed():
        G.test_crop_and_resize_kernels(dt)


@pytest.mark.parametrize('seed,shape', [(11, (320, 416)), (13, (448, 608))])
def test_rpn_loss_chain_from_source(G, seed, shape):
    """lh_match_kernel (block reductions over shuffles, ballot-ordered compaction) and lh_rpn_loss_kernel against oracle.rpn_one_image: lists equal, loss, gradients"""
    with HC.installed():
        G.test_rpn_loss_chain_vs_oracle(seed, shape)


def test_rcnn_loss_kernel_from_source(G):
    with HC.installed():
        G.test_rcnn_loss_kernel()


LH_OPS = ('depthwise_conv', 'depthwise_wgrad', 'lhrcnn_match', 'lhrcnn_rpn_loss', 'crop_and_resize_fwd', 'crop_and_resize_bwd', 'lhrcnn_rcnn_loss',
          'lhrcnn_rpn_decode', 'lhrcnn_gather_rois', 'lhrcnn_rcnn_decode', 'nms_batched')


@pytest.fixture()
def lh_kernels_in_the_mock():
    """the whole class on the CPU: every generic launch (convolutions, batch norm, pool, optimizer) through tests/mock_ops.py, the ten Light-Head R-CNN launches
    through the emulated KERNELS (plus the oracle-backed NMS of hip_cpu_backend)"""
    import mock_ops
    import odtk  # noqa: F401
    from odtk import ops
    real = {n: getattr(ops, n) for n in LH_OPS}
    with mock_ops.installed(), HC.installed():
        mocked = {n: getattr(ops, n) for n in LH_OPS}
        for n in LH_OPS:
            if n != 'nms_batched':
                setattr(ops, n, real[n])
        try:
            yield
        finally:
            for n in LH_OPS:
                setattr(ops, n, mocked[n])


def test_whole_class_training_with_the_kernels_from_source(lh_kernels_in_the_mock):
    """two training steps of odtk.LHRCNN (320 x 416, batch 2) against oracle/lhrcnn_ref.train_step with the ten LH_RCNN launches executing the kernel source:
    what tests/test_gpu_lhrcnn.py::test_training_steps_vs_oracle checks on the GPU, here with the exact torch convolutions around the kernels"""
    import odtk
    from oracle import lhrcnn_ref as LR
    from test_models_host_logic_cpu import _lhrcnn_cfg, _rel
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(901)
    imgs = (torch.rand(2, 320, 416, 3, generator=g) * 255).round()
    gt = LR.synthetic_gt(2, 320, 416, 911)
    p = LR.init_params(71)
    m = odtk.LHRCNN(_lhrcnn_cfg('train', 2), {'data_shape': [320, 416, 3], 'num_train': 2, 'num_val': 0, 'train_generator': [(imgs, gt)], 'val_generator': None})
    m.load_oracle_params(p)
    m.set_batch(imgs, gt)
    q = {k: v.clone() for k, v in p.items()}
    mom = {k: torch.zeros_like(v) for k, v in p.items()}
    for step in range(2):
        m.train_step(0.003)
        rpn, rcnn = LR.train_step(q, mom, imgs, gt, 0.003)
        # The RPN loss is tight.  The R-CNN loss is not, for a reason that is TensorFlow's as much as ours: a proposal clamped to the picture ends at the normalised
        # coordinate 1.0 exactly, so crop_and_resize's last sample row lands on H - 1 give or take one rounding, and whether it counts as inside or is
        # extrapolated to 0 depends on the last bits of the box's OTHER corner.  The depthwise kernels differ from torch's grouped convolution in the seventh digit,
        # the batch-norm stack turns that into 1e-5 on the proposals, and a few of the ~500 crops flip their border row (given identical boxes kernel and oracle
        # agree bit for bit: test_crop_and_resize_kernels_from_source, and in situ on the GPU).
        tol = 1e-4 if step == 0 else 5e-3
        assert abs(float(m.last_losses[0]) - rpn) < tol * abs(rpn) and abs(float(m.last_losses[1]) - rcnn) < 2e-2 * abs(rcnn), (step, m.last_losses, rpn, rcnn)
        if step == 0:
            after = m.export_params()
            for k in LR.trainable_names(p, 'rpn') + [k for k in q if k.endswith(('.mmean', '.mvar'))]:
                assert _rel(after[k], q[k]) < 2e-3 or float((after[k] - q[k]).abs().max()) < 2e-6, (k, _rel(after[k], q[k]))
            for k in LR.trainable_names(p, 'rcnn'):
                du, dref = (after[k] - p[k]).double(), (q[k] - p[k]).double()
                assert float((du * dref).sum() / (du.norm() * dref.norm() + 1e-30)) > 0.97, k      # (0.989 at worst here; 0.99995 on the GPU, whose proposals sit closer to the oracle's)


def test_whole_class_inference_with_the_kernels_from_source(lh_kernels_in_the_mock):
    """the reference's 135 detections (tests/golden/lhrcnn_detect.npz) through lh_rpn_decode / lh_gather_rois / crop / lh_rcnn_decode executed from source"""
    import odtk
    from oracle import lhrcnn_ref as LR
    from test_models_host_logic_cpu import _lhrcnn_cfg
    g = np.load(os.path.join(HERE, 'golden', 'lhrcnn_detect.npz'))
    p = LR.init_params(71)
    for k in g.files:
        if k.startswith('stat__'):
            p[k[6:].replace('__', '.')] = torch.from_numpy(g[k])
    m = odtk.LHRCNN(_lhrcnn_cfg('test', 1, nms_score_threshold=float(g['score_threshold']), post_nms_proposal=int(g['post_nms_proposal'])), None)
    m.load_oracle_params(p)
    scores, bbox, cid = m.test_one_image((torch.from_numpy(g['image']).float() / 127.5 - 1.).numpy())
    assert np.array_equal(cid, g['class_id'])                       # the same 135 detections in the same order
    size = np.maximum(1.0, np.maximum(g['bbox'][:, 2] - g['bbox'][:, 0], g['bbox'][:, 3] - g['bbox'][:, 1]))[:, None]
    assert float(np.abs(scores - g['scores']).max()) < 1e-3 and float((np.abs(bbox - g['bbox']) / size).max()) < 1e-3      # the GPU test's bounds (3.5e-5 measured here)


# ------------------------------------------------------------------------------------------------------------------ csrc/augment.hip from source
class _AsDevice(torch.Tensor):
    """a CPU tensor that answers `is_cuda` like a device tensor (odtk.augment.Augmentor insists on device tensors; the emulated kernels take host pointers)"""
    @property
    def is_cuda(self):
        return True


@pytest.fixture()
def augment_on_cpu(monkeypatch):
    import odtk  # noqa: F401
    from odtk import _lib, augment
    lib = HC.build()
    for n in ('odtk_augment_workspace_bytes', 'odtk_augment_boxes', 'odtk_augment_images'):
        f = getattr(lib, n)
        f.restype, f.argtypes = _lib.SIGNATURES[n]

    def call(name, *args):
        HC.CALLED.add(name)
        rc = getattr(lib, name)(*args)
        assert rc == 0, lib.odtk_last_error().decode()

    def call_ll(name, *args):
        HC.CALLED.add(name)
        return int(getattr(lib, name)(*args))
    monkeypatch.setattr(augment, 'call', call)
    monkeypatch.setattr(augment, 'call_ll', call_ll)
    monkeypatch.setattr(augment._lib, 'load', lambda: lib)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: type('S', (), {'cuda_stream': 0})())
    monkeypatch.setattr(torch.Tensor, 'record_stream', lambda self, s: None)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    return lambda t: torch.Tensor._make_subclass(_AsDevice, t.contiguous())


@pytest.mark.parametrize('fname', ['augment.npz', 'augment_zoom_methods.npz'])
def test_augmentor_kernels_from_source_vs_reference(augment_on_cpu, fname):
    """aug_geometry / aug_colour / aug_rotate / aug_boxes executed from source on the golden cases produced by the reference's own image_augmentor (scripted draws):
    what tests/test_gpu_augment.py::test_golden_cases_vs_reference checks on the GPU -- bilinear / nearest / bicubic zoom, pad, crop, flips, colour jitter with the
    shuffle-reduced contrast mean, rotate, the ballot-compacted boxes"""
    import json
    from odtk import augment as A
    g = np.load(os.path.join(HERE, 'golden', fname))
    for m in json.loads(bytes(g['meta']).decode()):
        n = m['name']
        for u8 in (False, True):
            src = torch.from_numpy(g[f'{n}_image'])
            img = augment_on_cpu(src if u8 else src.float())
            h, w = m['hw']
            out, gt = A.image_augmentor(img, [h, w, 3], m['data_format'], ground_truth=augment_on_cpu(torch.from_numpy(g[f'{n}_gt_in'])), pad_truth_to=6,
                                        draws=m['draws'], **m['kwargs'])
            np.testing.assert_allclose(gt.numpy(), g[f'{n}_gt_out'], rtol=0, atol=1e-4, err_msg=n)
            want = g[f'{n}_aug']
            if m['kwargs'].get('rotate') is not None and m['data_format'] == 'channels_first':
                want = want.transpose(2, 0, 1)
            np.testing.assert_allclose(torch.Tensor(out).numpy(), want, rtol=0, atol=2e-3, err_msg=n)
            if m['kwargs']['fill_mode'] == 'NEAREST_NEIGHBOR' and m['kwargs'].get('color_jitter_prob') is None:
                assert np.array_equal(torch.Tensor(out).numpy(), want), n


# ------------------------------------------------------------------------------------------------------------------ the other non-MFMA files from source
# elementwise.hip (batch norm in its one / two / three-launch forms, pools with recorded arg-max, L2-norm, column sums, the fused optimizer, resize, channel copies,
# preprocess), boxes.hip WITHOUT its NMS kernels (priors, matching, SSD loss, decode), retina.hip, dense_heads.hip, refinedet.hip: the GPU test bodies, device = CPU.
CPU = torch.device('cpu')


def _run(module, name, **kw):
    mod = __import__(module)
    with HC.installed():
        getattr(mod, name)(dev=CPU, **kw)


_BN_SHAPES = {'a': ((2 * 19 * 19, 1024, True), 'f32', 'f32'), 'b': ((3 * 5 * 5, 150, False), 'bf16', 'bf16'), 'c': ((6 * 38 * 38, 100, False), 'bf16', 'f32'),
              'd': ((14 * 19 * 19, 256, True), 'bf16', 'bf16'), 'e': ((3 * 61 * 47, 16, True), 'bf16', 'bf16'), 'f': ((2 * 40 * 52, 32, True), 'bf16', 'f32'),
              'g': ((5000, 8, False), 'bf16', 'bf16')}
_BN_MODES = {'one-launch': 1, 'one-launch-64ch': 10, 'two-launches': 2, 'three-launches': 3, 'auto': 0}


@pytest.mark.parametrize('case', ['a-one-launch', 'b-one-launch', 'a-one-launch-64ch', 'a-two-launches', 'c-two-launches', 'a-three-launches', 'c-three-launches', 'd-three-launches',
                                  'a-auto', 'd-auto', 'e-three-launches', 'f-three-launches', 'g-three-launches', 'e-auto'])
def test_batchnorm_from_source(case):
    shape, mode = case.split('-', 1)
    sh, dt, ydt = _BN_SHAPES[shape]
    _run('test_gpu_kernels', 'test_batchnorm', shape=sh, dt=dt, ydt=ydt, launches=_BN_MODES[mode])


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_pools_from_source(dt):
    _run('test_gpu_kernels', 'test_maxpool', geom=(2, 19, 19, 32, 3, 1), dt=dt)
    _run('test_gpu_kernels', 'test_maxpool', geom=(1, 38, 38, 8, 2, 2), dt=dt)
    _run('test_gpu_kernels', 'test_maxpool2x2_recorded_argmax_equals_gather_path', geom=(3, 9, 13, 40), dt=dt)
    _run('test_gpu_kernels', 'test_maxpool_recorded_argmax_overlapping_windows', geom=(3, 9, 13, 40, 3, 2), dt=dt)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_l2norm_colsum_sgd_resize_copy_from_source(dt):
    _run('test_gpu_kernels', 'test_l2norm_colsum_sgd', dt=dt)
    _run('test_gpu_kernels', 'test_resize_bilinear_align_corners_any_scale', geom=(1, 10, 12, 3, 5, 16, True), dt=dt)
    _run('test_gpu_kernels', 'test_copy_channels_unaligned_concat', dt=dt)


def test_ssd_box_side_from_source():
    _run('test_gpu_kernels', 'test_preprocess')
    _run('test_gpu_kernels', 'test_priors_bit_exact')
    _run('test_gpu_kernels', 'test_match_bit_exact')
    _run('test_gpu_kernels', 'test_ssd_loss_and_grad_vs_oracle')
    _run('test_gpu_kernels', 'test_decode_and_detect_vs_oracle')
    _run('test_gpu_kernels', 'test_loss_total_and_zero', n=1000)


def test_retina_box_side_from_source():
    _run('test_gpu_retina', 'test_retina_anchors_bit_exact', data_shape=[320, 256, 3])
    _run('test_gpu_retina', 'test_retina_match_indices_bit_exact', data_shape=[320, 256, 3], seed=1)
    _run('test_gpu_retina', 'test_retina_loss_vs_reference_golden')
    _run('test_gpu_retina', 'test_retina_loss_and_grad_vs_oracle', data_shape=[320, 256, 3], gamma=2.0)
    _run('test_gpu_retina', 'test_retina_decode_candidates')


def test_dense_heads_from_source():
    for name in ('test_centernet_loss_golden_inputs', 'test_fcos_loss_golden_inputs', 'test_yolov3_loss_golden_inputs', 'test_fcos_decode_candidates',
                 'test_yolov3_decode_candidates', 'test_full_inference_tails_vs_reference', 'test_fcos_loss_config5_shape', 'test_yolov3_loss_config4_shape'):
        _run('test_gpu_dense_heads', name)
    _run('test_gpu_dense_heads', 'test_centernet_decode', img=1, shift=3.0, thr=0.1, topk=100)


def test_refinedet_box_side_from_source():
    _run('test_gpu_refinedet', 'test_anchors_bit_exact', size=320)
    _run('test_gpu_refinedet', 'test_loss_matches_reference_numbers_and_oracle_gradients')
    _run('test_gpu_refinedet', 'test_inference_tail_matches_reference_detections')


def test_tensorflow_op_test_tables_on_the_kernels_from_source(augment_on_cpu):
    """TensorFlow's own tables (tests/tf_known_answers.py) on the kernel source: the three GPU cases that have not run on hardware yet (crop_and_resize, SAME pooling,
    the momentum update), the TF-1.x resize grid, the fused batch-norm statistics -- through the bodies of tests/test_gpu_tf_known_answers.py"""
    import test_gpu_tf_known_answers as T
    with HC.installed():
        T.test_crop_and_resize_tables(CPU)
        T.test_pooling_same_padding_tables(CPU)
        T.test_momentum_optimizer_update_rule(CPU)
        T.test_fused_batch_norm_training_statistics(CPU)
        for dt in ('f32', 'bf16'):
            T.test_resize_bilinear_legacy_grid(dt, CPU)


def test_whole_class_bf16_engine_with_the_kernels_from_source(lh_kernels_in_the_mock):
    """the opt-in bf16 engine of LHRCNN (never run on hardware as a whole) for one training step and one inference with the LH_RCNN kernels executing from source on
    bf16 storage: depthwise4<bf16>, crop rows in bf16, the head's outputs widened to f32 in front of lh_rcnn_loss_kernel, the crop gradient through its f32 scratch"""
    import odtk
    from oracle import lhrcnn_ref as LR
    from test_models_host_logic_cpu import _lhrcnn_cfg
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(901)
    imgs = (torch.rand(2, 320, 416, 3, generator=g) * 255).round()
    gt = LR.synthetic_gt(2, 320, 416, 911)
    p = LR.init_params(71)
    m = odtk.LHRCNN(_lhrcnn_cfg('train', 2, compute_dtype='bf16'), {'data_shape': [320, 416, 3], 'num_train': 2, 'num_val': 0, 'train_generator': [(imgs, gt)], 'val_generator': None})
    m.load_oracle_params(p)
    m.set_batch(imgs, gt)
    before = m.P.clone()
    m.train_step(0.003)
    rpn, rcnn = LR.losses(p, imgs, gt)
    st = m.loss
    assert abs(float(m.last_losses[0]) - float(rpn)) < 0.2 * float(rpn) and 0.2 * float(rcnn) < float(m.last_losses[1]) < 5. * float(rcnn)
    assert st.roi.dtype == torch.bfloat16 and float(st.roi.float().abs().max()) > 0 and torch.equal(st.logits32, st.logits.float())
    assert torch.equal(st.d_logits.float(), st.d_logits32.to(torch.bfloat16).float()) and torch.equal(m.feat.g.float(), st.d_feat32.to(torch.bfloat16).float())
    kp, kn = [int(v) for v in st.ws['roi_counts'].sum(0)]
    assert 0 < kp <= 2 * 128 and 0 < kn and float(st.roi[256 + int(st.ws['roi_counts'][1].sum()):].float().abs().max()) == 0.0        # empty slots are zero rows
    assert bool(torch.isfinite(m.P).all()) and not torch.equal(m.P, before)
    gd = np.load(os.path.join(HERE, 'golden', 'lhrcnn_detect.npz'))
    for k in gd.files:
        if k.startswith('stat__'):
            p[k[6:].replace('__', '.')] = torch.from_numpy(gd[k])
    mt = odtk.LHRCNN(_lhrcnn_cfg('test', 1, nms_score_threshold=float(gd['score_threshold']), post_nms_proposal=int(gd['post_nms_proposal']), compute_dtype='bf16'), None)
    mt.load_oracle_params(p)
    scores, bbox, cid = mt.test_one_image((torch.from_numpy(gd['image']).float() / 127.5 - 1.).numpy())
    assert len(scores) > 0.5 * len(gd['scores']) and np.isfinite(bbox).all()


@pytest.mark.parametrize('mode', ['one-launch', 'three-launches'])
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_group_norm_from_source(dt, mode):
    """the group-norm kernels (FCOS head) against torch autograd through the GPU test's own cases"""
    import odtk  # noqa: F401
    from odtk import ops
    import test_gpu_retinanet_model as mod
    with HC.installed():
        ops.debug_set(7, 1024 if mode == 'one-launch' else 0)
        try:
            mod._group_norm_cases(ops, CPU, dt)
        finally:
            ops.debug_set(7, 1024)


def test_yolov2_box_side_from_source():
    _run('test_gpu_yolov2', 'test_loss_kernel_matches_oracle', geom=(2, 6, 7, 3, 4))
    _run('test_gpu_yolov2', 'test_loss_kernel_matches_oracle', geom=(2, 15, 15, 5, 20))
    _run('test_gpu_yolov2', 'test_decode_candidates_and_detections')


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_pyramid_glue_and_centernet_elementwise_from_source(dt):
    """add2d / upsample2x (YOLOv3's routes), the gather backward of the feature-map resize (RetinaNet / FCOS pyramids), CenterNet's preprocess_norm /
    avgpool backward / residual add + ReLU"""
    _run('test_gpu_yolov3', 'test_glue_kernels', dt=dt)
    _run('test_gpu_yolov3', 'test_resize_bilinear_feature_maps', dt=dt)
    _run('test_gpu_centernet_model', 'test_elementwise_kernels', dt=dt)


def test_adam_from_source():
    _run('test_gpu_centernet_model', 'test_adam_kernel_three_steps')


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(2 * 13 * 13, 96, True), (5000, 40, False)])
def test_global_batch_norm_entry_points_from_source(shape, dt):
    """odtk_bn_moments / _fwd_given / _bwd_sums / _bwd_given (ops.SyncBN, SURVEY.md 8e option B) with the two exchanges done by hand: two replicas with half the
    rows each compute what odtk_bn_fwd / odtk_bn_bwd compute on all rows"""
    import odtk  # noqa: F401
    from odtk import ops
    import glue_exact as GX
    GX.global_batch_norm_case(ops, CPU, shape, dt, HC.installed())          # (the same body runs on the GPU: tests/test_gpu_glue_exact.py)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_row_glue_kernels_from_source(dt):
    """exp rows (FCOS.py:363) and its chain rule, conv rows <-> f32 prediction tensors (RetinaNet.py:184-186), casts, relu(a + b) and the ReLU gradient taken
    from the output (RefineDet.py:371): each against the torch expression, pitched operands"""
    import odtk  # noqa: F401
    from odtk import ops
    tdt = torch.float32 if dt == 'f32' else torch.bfloat16
    g = torch.Generator().manual_seed(9)
    M, C, ld = 3 * 35, 4, 8
    with HC.installed():
        x = torch.randn(M, ld, generator=g).to(tdt)
        y = torch.zeros(M, C)
        ops.exp_rows_to_f32(x, ld, y, M, C)
        assert torch.allclose(y, torch.exp(x[:, :C].float()), rtol=1e-6, atol=0)
        dy = torch.randn(M, C, generator=g)
        dx = torch.full((M, ld), 7., dtype=tdt)
        ops.exp_rows_bwd(dy, y, dx, ld, M, C)
        assert torch.equal(dx[:, :C], (dy * y).to(tdt)) and not dx[:, C:].any()
        # three images of 35 rows into a prediction tensor [3][100][C] at row offset 20
        pred = torch.zeros(3, 100, C)
        ops.rows_to_f32(x, ld, pred[:, 20:], C, 35, 100 * C, M, C)
        assert torch.equal(pred[:, 20:55], x[:, :C].float().view(3, 35, C)) and not pred[:, :20].any() and not pred[:, 55:].any()
        back = torch.full((M, ld), 3., dtype=tdt)
        ops.rows_from_f32(pred[:, 20:], C, 35, 100 * C, back, ld, M, C)
        assert torch.equal(back[:, :C], x[:, :C]) and not back[:, C:].any()
        f = torch.randn(1000, generator=g)
        o = torch.zeros(1000, dtype=tdt); ops.cast_from_f32(f, o)
        assert torch.equal(o, f.to(tdt))
        w = torch.zeros(1000); ops.cast_to_f32(o, w)
        assert torch.equal(w, o.float())
        Cc, lda, ldb = 16, 24, 16
        a, b = torch.randn(50, lda, generator=g).to(tdt), torch.randn(50, ldb, generator=g).to(tdt)
        r = torch.zeros(50, Cc, dtype=tdt)
        ops.add_relu_fwd(a, lda, b, ldb, r, Cc, 50, Cc)
        assert torch.equal(r, torch.relu(a[:, :Cc].float() + b[:, :Cc].float()).to(tdt))
        d = torch.randn(50, Cc, generator=g).to(tdt)
        prev = torch.randn(50, lda, generator=g).to(tdt)
        for acc in (False, True):
            out = prev.clone()
            ops.relu_bwd(r, d, Cc, out, lda, 50, Cc, acc)
            want = torch.where(r > 0, d.float(), torch.zeros(())) + (prev[:, :Cc].float() if acc else 0.)
            assert torch.equal(out[:, :Cc], want.to(tdt)) and torch.equal(out[:, Cc:], prev[:, Cc:])


KEEP_MOCKED = ('FilterPrepareBatch', 'conv2d_fwd', 'conv2d_dgrad', 'conv2d_wgrad', 'conv2d_fwd_pool2x2', 'conv2d_fwd_pool2x2_fused', 'scratch_slot', 'nms_batched')


@contextlib.contextmanager
def _mixed_installed():
    """tests/mock_ops.installed() with everything but the MFMA convolutions and the NMS handed back to the real wrappers, which the emulation serves"""
    import mock_ops
    import odtk  # noqa: F401
    from odtk import ops
    names = [n for n, v in vars(mock_ops).items() if callable(v) and not n.startswith('_') and n not in ('installed', 'contextlib') and hasattr(ops, n)]
    real = {n: getattr(ops, n) for n in names}
    with _MOCK_INSTALLED(), HC.installed():
        mocked = {n: getattr(ops, n) for n in names}
        for n in names:
            if n not in KEEP_MOCKED:
                setattr(ops, n, real[n])

        def conv_then_pool(d, x, w, bias, y, relu, y_pool, idx):
            # odtk_conv2d_fwd_pool2x2 is ONE entry point of conv.hip; here its two halves: torch's convolution, then the pooling KERNEL, whose recorded arg-max
            # (uint16 per 16-byte output chunk) is what the emulated maxpool2x2_bwd_idx reads in the backward pass
            if idx is None or int(y_pool.shape[-1]) != int(d.ldy):
                return mocked['conv2d_fwd_pool2x2'](d, x, w, bias, y, relu, y_pool, idx)
            full = y if y is not None else torch.zeros(d.N * d.Ho * d.Wo, d.ldy, dtype=y_pool.dtype)
            mocked['conv2d_fwd'](d, x, w, bias, full, relu)
            real['maxpool2x2_fwd_idx'](full, y_pool, idx, d.N, d.Ho, d.Wo, d.K, d.ldy, (d.Ho + 1) // 2, (d.Wo + 1) // 2)
        ops.conv2d_fwd_pool2x2 = conv_then_pool
        try:
            yield
        finally:
            for n in names:
                setattr(ops, n, mocked[n])


@pytest.fixture()
def all_but_the_convolutions_from_source():
    """a whole model class on the CPU with ONLY the MFMA convolutions (exact torch convolutions, tests/mock_ops.py) and the NMS (oracle-backed, hip_cpu_backend)
    standing in: every other launch of the step executes the kernel source.  While the fixture is active `mock_ops.installed()` itself means this mix, so the
    bodies of tests/test_models_host_logic_cpu.py can be called as they are."""
    import mock_ops
    global _MOCK_INSTALLED
    _MOCK_INSTALLED = mock_ops.installed
    mock_ops.installed = _mixed_installed
    try:
        with _mixed_installed():
            yield
    finally:
        mock_ops.installed = _MOCK_INSTALLED


def test_ssd300_training_step_with_every_non_mfma_kernel_from_source(all_but_the_convolutions_from_source):
    """the headline class, one training step at 300 x 300 batch 2 against oracle/ssd300_ref.train_step (pinned on the reference's own class): preprocess, pools
    with recorded arg-max, L2-norm, the batch norms that write the prediction tensor, prior generation, matching, loss with hard-negative mining, the backward
    glue and the fused optimizer all run from csrc/*.hip; only the convolutions are torch's"""
    import odtk
    from oracle import ssd300_ref as R
    from test_models_host_logic_cpu import _rel
    torch.set_num_threads(8)
    cfg = {'mode': 'train', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 2,
           'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': '', 'verbose': False,
           'compute_dtype': 'f32', 'seed': 0, 'use_graph': False, 'device': 'cpu'}
    imgs, gt = R.synthetic_batch(2, 31)
    p = R.init_params(3)
    m = odtk.SSD300(cfg, {'data_shape': [300, 300, 3], 'num_train': 2, 'num_val': 0, 'train_generator': [], 'val_generator': None})
    m.load_oracle_params(p)
    m.set_batch(imgs, gt)
    n0 = len(HC.CALLED)
    loss = float(m.train_step(0.01))
    assert {'odtk_ssd_match', 'odtk_ssd_loss', 'odtk_bn_fwd', 'odtk_bn_bwd', 'odtk_l2norm_fwd', 'odtk_l2norm_bwd', 'odtk_sgd_momentum', 'odtk_preprocess'} <= HC.CALLED, n0
    q = {k: v.clone() for k, v in p.items()}
    mom = {k: torch.zeros_like(v) for k in R.trainable_names(p) for v in [p[k]]}
    total, _ = R.train_step(q, mom, imgs, gt, 0.01)
    assert abs(loss - total) < 1e-4 * abs(total), (loss, total)
    after = m.export_params()
    bad = []
    for k in q:
        if k.endswith('.b') and (k[:-2] + '.gamma') in q:
            continue
        step = q[k] - p[k]
        if float(step.norm()) < 1e-12:
            continue
        bad.append((k, _rel(after[k] - p[k], step)))
    bad = [b for b in bad if not b[1] < 3e-2]                  # (the bound of the mocked and of the GPU test: ReLU flips in front of a batch norm)
    assert not bad, ' '.join(f'{k}:{v:.2g}' for k, v in bad)


@pytest.mark.skipif(os.environ.get('ODTK_EMU_ALL') != '1', reason='about a minute per class: ODTK_EMU_ALL=1 runs it (profiles/r03zzzz_emulated_insitu.md has the output)')
@pytest.mark.parametrize('kind', ['yolov3', 'ssd300', 'retinanet', 'fcos', 'centernet'])
def test_every_launch_of_a_training_step_in_situ_with_the_kernels_from_source(all_but_the_convolutions_from_source, kind):
    """BASELINE.json's five model classes: every launch of a whole training step -- batch / group norm, pools, resizes, route glue, box-side losses, optimizer,
    all executing the kernel source; the convolutions are torch's -- re-executed in plain f32 PyTorch from the engine's OWN inputs of that launch (tests/insitu.py,
    the harness of the GPU in-situ tests) and compared at the f32 bounds of the GPU runs.  Per launch, not end to end: a 50-layer batch-norm stack at batch 2
    turns 2e-7 on an activation into per cents on the first layer's gradient (measured here on RetinaNet), which says nothing about any kernel."""
    import insitu
    import mock_ops
    import test_insitu_cpu as IC
    torch.set_num_threads(8)
    make, imgs, gt, lr = IC.MODELS[kind]()
    sh = insitu.Shadow()
    with sh.installed():
        m = make()
        if kind == 'retinanet':
            mock_ops.retina_loss.anchors = m.anc
        m.set_batch(imgs, gt)
        sh.recording = True
        m.train_step(lr)
        sh.recording = False
    rows = sh.check(insitu.default_tol('f32'), verbose=True, label=f'{kind}, kernels from source')
    assert sh.seq > 50 and rows          # ('stray elements' in the printout: gradients the restatement sums to exactly 0 and the kernel to 1e-9 -- two opposite terms)


def test_zz_emulation_coverage_report():
    """(runs last in this file) which C-ABI entry points of the emulated build the tests above actually executed; written to $ODTK_EMU_COVERAGE when set"""
    import odtk  # noqa: F401
    from odtk import _lib
    with HC.installed() as names:
        pass
    ran = sorted(HC.CALLED & set(names))
    out = os.environ.get('ODTK_EMU_COVERAGE')
    if out:
        with open(out, 'w') as f:
            f.write(f'{len(ran)} of {len(names)} emulated entry points executed ({len(_lib.SIGNATURES)} in the library)\n')
            f.write('executed: ' + ' '.join(ran) + '\n')
            f.write('not executed: ' + ' '.join(sorted(set(names) - set(ran))) + '\n')
    if len(HC.CALLED) > 20:                                # the whole file ran in this process
        missing = set(names) - set(ran) - {'odtk_nms_batched', 'odtk_last_error', 'odtk_version'}      # (NMS: DPP kernels, replaced -- hip_cpu_backend.py)
        assert not missing, sorted(missing)
