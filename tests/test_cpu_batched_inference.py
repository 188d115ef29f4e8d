"""CPU tier of the batched inference path.
  * the decode, compaction, gather and pack kernels of csrc/detect_batched.hip run FROM SOURCE under the fiber emulation (tests/hip_cpu_backend.py), through the
    test bodies of the GPU cases (tests/batched_inference_cases.py); the NMS stands in as hip_cpu_backend already does for odtk_nms_batched (the oracle's NMS
    behind the kernel's operand addressing).  hip_cpu_backend.KERNEL_FILES is extended for the duration of these tests only and put back afterwards;
  * host logic of evaluate(batch_size=B) over mocked launches: chunking, partial last chunk, the num_images cut-off, the per-batch_size cache of test-mode
    copies, test_batch_size validation, the fallback loop."""
import contextlib
import os
import tempfile

import numpy as np
import pytest
import torch

import batched_inference_cases as BC
import hip_cpu_backend as HC
import mock_ops


@contextlib.contextmanager
def emulated():
    """the emulation with csrc/detect_batched.hip in the build; module state of hip_cpu_backend restored on the way out (its own coverage report counts on it)"""
    from odtk import ops
    files, lib, tmp = list(HC.KERNEL_FILES), HC._LIB, tempfile.tempdir
    HC.KERNEL_FILES = files + ['detect_batched.hip']
    HC._LIB = None
    # hip_cpu_backend caches its build in the temp dir under a name made of the newest source time stamp: the extended build gets a directory of its own, or the
    # build of the plain file list would find it under the same name
    tempfile.tempdir = os.path.join(tempfile.gettempdir(), f'odtk_cpu_batched_{os.getuid()}')
    os.makedirs(tempfile.tempdir, exist_ok=True)
    try:
        with HC.installed() as names:
            assert 'odtk_detection_pack' in names and 'odtk_compact_rows' in names
            old = ops.nms_image_class
            ops.nms_image_class = mock_ops.nms_image_class_via(ops.nms_batched)
            try:
                yield
            finally:
                ops.nms_image_class = old
    finally:
        HC.KERNEL_FILES, HC._LIB, tempfile.tempdir = files, lib, tmp


@pytest.mark.parametrize('kind', ['ssd', 'retina'])
def test_emulated_tail_equals_single_image_tail(kind):
    with emulated():
        BC.check_tail(kind, 'cpu')


def test_emulated_compaction_equals_nonzero():
    with emulated():
        BC.check_compaction('cpu')


def test_emulated_pack_order_and_scan():
    """odtk_detection_pack on hand-made NMS tables: counts, exclusive scan, (image, class, pick) order"""
    from odtk import ops
    with emulated():
        N, nc, cap, n = 3, 4, 5, 50
        g = torch.Generator().manual_seed(1)
        conf = torch.rand(N, n, nc, generator=g); boxes = torch.rand(N, n, 4, generator=g)
        cnt = torch.tensor([[2, 0, 5, 1], [0, 0, 0, 0], [3, 3, 0, 4]], dtype=torch.int32)
        idx = torch.randint(0, n, (N, nc, cap), generator=g).to(torch.int32)
        K = N * nc * cap
        counts = torch.zeros(N, dtype=torch.int32); offsets = torch.zeros(N + 1, dtype=torch.int32)
        scores = torch.zeros(K); bbox = torch.zeros(K, 4); cid = torch.full((K,), -1, dtype=torch.int32)
        ops.detection_pack(idx, cnt, conf, boxes, counts, offsets, scores, bbox, cid)
        assert counts.tolist() == [8, 0, 10] and offsets.tolist() == [0, 8, 8, 18]
        k = 0
        for i in range(N):
            for c in range(nc):
                for j in range(int(cnt[i, c])):
                    r = int(idx[i, c, j])
                    assert float(scores[k]) == float(conf[i, r, c]) and torch.equal(bbox[k], boxes[i, r]) and int(cid[k]) == c
                    k += 1
        assert k == 18 and bool((cid[18:] == -1).all())


# ---------------------------------------------------------------- host logic over mocked launches
def mocked():
    """the CPU stand-in of the library (tests/mock_ops.py), the batched tail included"""
    return mock_ops.installed()


def _canned_class(dets, native):
    from odtk.heads import BatchedInference
    from odtk.voc_eval import EvaluateMixin

    class Canned(EvaluateMixin):
        NATIVE_TEST_IMAGES = native
        built = []

        def __init__(self, config, data_provider):
            self.config, self.data_provider, self.mode = config, data_provider, config['mode']
            self.dev = torch.device('cpu')
            self.batch_size = config['batch_size'] if self.mode == 'train' else BatchedInference._test_batch_size(config)
            self.calls, self.loaded = [], 0
            if self.mode == 'train':
                self.val_generator, self.num_val = data_provider['val_generator'], data_provider['num_val']
            Canned.built.append(self)

        def export_params(self):
            return {'w': 1}

        def load_oracle_params(self, p):
            self.loaded += 1

        def test_one_image(self, images):
            assert images.shape[0] == 1
            self.calls.append([int(images[0, 0, 0, 0])])
            return list(dets[int(images[0, 0, 0, 0])])

        if native:
            def test_images(self, images):
                assert 1 <= images.shape[0] <= self.batch_size, (images.shape, self.batch_size)
                self.calls.append([int(v) for v in images[:, 0, 0, 0]])
                return [list(dets[int(v)]) for v in images[:, 0, 0, 0]]
    return Canned


def test_evaluate_batch_size_chunks_cutoff_partial_and_cache():
    import odtk
    import test_cpu_voc_eval as TV
    import voc_eval_ref as R
    rng = np.random.default_rng(3)
    dets, gts = TV._random_case(rng, 21, 3, 10, 4)
    gen = TV._generator(gts, 7)                                       # 3 batches of 7 images
    cfg = {'mode': 'test', 'num_classes': 3, 'batch_size': 2, 'test_batch_size': 4}
    with TV.emulated():
        Canned = _canned_class(dets, True)
        m = Canned(cfg, None)
        r = odtk.evaluate(m, gen, num_images=18, batch_size=4)
        assert m.calls == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17]]      # regrouped across batches; the chunk before 18 cut short
        TV._check(r, R.evaluate(dets[:18], gts[:18], 3))
        m = Canned(cfg, None)
        r = odtk.evaluate(m, gen, batch_size=4)                                                          # one pass: the last chunk is partial
        assert m.calls[-1] == [20] and sum(len(c) for c in m.calls) == 21 and all(len(c) == 4 for c in m.calls[:-1])
        TV._check(r, R.evaluate(dets, gts, 3))
        m = Canned(cfg, None)
        odtk.evaluate(m, gen, num_images=8, batch_size=4)
        assert m.calls == [[0, 1, 2, 3], [4, 5, 6, 7]]
        m = Canned(cfg, None)
        r1 = odtk.evaluate(m, gen, num_images=18)                                                        # default: the per-image path
        assert m.calls == [[i] for i in range(18)]
        TV._check(r1, R.evaluate(dets[:18], gts[:18], 3))
        # the mixin's loop (a class without a native test_images), same results
        Loop = _canned_class(dets, False)
        m = Loop(cfg, None)
        r = odtk.evaluate(m, gen, num_images=18, batch_size=4)
        assert m.calls == [[i] for i in range(18)]
        TV._check(r, R.evaluate(dets[:18], gts[:18], 3))
        # a train-mode model: one test-mode copy per batch_size, weights copied before every evaluation, built with test_batch_size = B
        Canned.built.clear()
        t = Canned({'mode': 'train', 'num_classes': 3, 'batch_size': 2}, {'val_generator': gen, 'num_val': 18})
        t.evaluate(batch_size=4); t.evaluate(batch_size=4); t.evaluate(); t.evaluate(batch_size=2)
        copies = Canned.built[1:]
        assert [c.batch_size for c in copies] == [4, 1, 2] and all(c.mode == 'test' for c in copies)
        assert copies[0].loaded == 2 and t._eval_models[4] is copies[0] and t._eval_model is copies[1] and t.calls == []
        assert copies[0].calls[:5] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17]]
        with pytest.raises(ValueError, match='batch_size'):
            odtk.evaluate(m, gen, batch_size=0)
    for bad in (0, -1, 2.0, True, '4'):
        with pytest.raises(ValueError, match='test_batch_size'):
            Canned(dict(cfg, test_batch_size=bad), None)


def test_ssd300_test_images_host_logic_over_mocked_launches():
    """SSD300 in test mode with test_batch_size 3 on the CPU stand-in (mocked launches): staging of n <= B images, the tail slots discarded, images independent
    of their slot, test_one_image == test_images(...)[0], channels_first accepted, shape errors; evaluate(batch_size=3) == the hand-fed evaluator"""
    import odtk
    from oracle import ssd300_ref as SR
    cfg = {'mode': 'test', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 8,
           'nms_score_threshold': 0.06, 'nms_max_boxes': 5, 'nms_iou_threshold': 0.5, 'pretraining_weight': '', 'verbose': False, 'device': 'cpu',
           'compute_dtype': 'f32', 'test_batch_size': 3}
    torch.set_num_threads(8)
    imgs, gt = SR.synthetic_batch(4, 5)
    import test_cpu_voc_eval as TV
    with mocked():
        m = odtk.SSD300(cfg, None)
        assert m.batch_size == 3 and tuple(m.images.shape) == (3, 300, 300, 3) and tuple(m.pred.shape[:2]) == (3, 8828)
        full = m.test_images(imgs[:3].numpy())
        assert len(full) == 3 and sum(len(d[0]) for d in full) > 0
        for s, b, c in full:
            assert s.dtype == np.float32 and b.dtype == np.float32 and c.dtype == np.int32 and b.shape == (len(s), 4) and c.shape == s.shape
        part = m.test_images(imgs[1:3].numpy())                        # n < B: the tail slot (still holding image 2) is computed and discarded
        assert len(part) == 2
        for a, b in zip(part, full[1:]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        one = m.test_one_image(imgs[2:3].numpy())
        assert all(np.array_equal(x, y) for x, y in zip(one, full[2]))
        cf = odtk.SSD300(dict(cfg, data_format='channels_first'), None)
        assert all(np.array_equal(x, y) for x, y in zip(cf.test_images(imgs[:1].permute(0, 3, 1, 2).numpy())[0], full[0]))
        for bad in (imgs[:4].numpy(), imgs[:0].numpy(), imgs[:2, :299].numpy()):
            with pytest.raises(ValueError, match='test_images'):
                m.test_images(bad)
        with TV.emulated():
            r = m.evaluate(generator=[(imgs, gt)], batch_size=3)
            ev = odtk.VOCEvaluator(20, device='cpu')
            for d, g in zip(m.test_images(imgs[:3].numpy()) + m.test_images(imgs[3:].numpy()), gt.numpy()):
                ev.add(d, g)
            want = ev.result()
        assert np.array_equal(r['AP'], want['AP'], equal_nan=True) and np.array_equal(r['npos'], want['npos']) and np.array_equal(r['tp'], want['tp'])

