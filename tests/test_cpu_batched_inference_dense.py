"""CPU tier of the batched inference path of CenterNet, RefineDet320 and PFPNetR.
  * which classes are native, the two new entry points in libodtk.so and in _lib.SIGNATURES;
  * odtk_centernet_decode_batched / odtk_refinedet_decode_batched run FROM SOURCE under the fiber emulation (test_cpu_batched_inference.emulated: the build with
    csrc/detect_batched.hip), through the bodies of the GPU cases (tests/batched_dense_cases.py);
  * host logic over mocked launches: image slots by test_batch_size, its validation, staging errors, test_images against test_one_image of a model built
    without the key, the read-back layout of heads.CenterNetBatched.
The mocks of the batched entry points are tests/mock_ops.py's (per image, its single-image stand-ins)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import batched_dense_cases as DC
import test_cpu_batched_inference as TB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_which_classes_are_native():
    import odtk
    for name in ('SSD300', 'SSD512', 'YOLOv3', 'RetinaNet', 'CenterNet', 'RefineDet320', 'PFPNetR'):
        assert getattr(odtk, name).NATIVE_TEST_IMAGES is True, name
    from odtk.voc_eval import EvaluateMixin
    for name in ('FCOS', 'YOLOv2', 'LHRCNN'):
        cls = getattr(odtk, name)
        assert cls.NATIVE_TEST_IMAGES is False and cls.test_images is EvaluateMixin.test_images, name
    assert 'test_images' not in vars(odtk.PFPNetR) and odtk.PFPNetR.test_images is odtk.RefineDet320.test_images


def test_library_exports_the_batched_decodes():
    from odtk import _lib
    lib = ctypes.CDLL(os.path.join(ROOT, 'object-detection-tensorflow_amd', 'libodtk.so'))
    for name in ('odtk_centernet_decode_batched', 'odtk_refinedet_decode_batched', 'odtk_centernet_decode_workspace_bytes'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.odtk_version() >= 102
    f = lib.odtk_centernet_decode_workspace_bytes
    f.restype, f.argtypes = _lib.SIGNATURES['odtk_centernet_decode_workspace_bytes']
    assert f(3, 128, 128) == 3 * 128 * 128 * 8               # N score planes + N class planes


# ---------------------------------------------------------------- the kernels from source under the emulation
@pytest.mark.parametrize('H,W,C,top_k', [(5, 7, 3, 5), (16, 16, 20, 1)])
def test_emulated_centernet_decode_batched(H, W, C, top_k):
    with TB.emulated():
        DC.check_centernet(H, W, C, top_k, 'cpu')


def test_emulated_centernet_read_back_class():
    with TB.emulated():
        DC.check_centernet_read_back('cpu')


def test_emulated_refinedet_decode_batched_and_tail():
    with TB.emulated():
        DC.check_refinedet(3, 37, 4, 'cpu')


# ---------------------------------------------------------------- host logic over mocked launches
mocked = TB.mocked


def _config(name, **kw):
    cfg = {'mode': 'test', 'input_size': 64, 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 8,
           'verbose': False, 'compute_dtype': 'f32', 'device': 'cpu'}
    if name == 'CenterNet':
        cfg.update(score_threshold=0.3, top_k_results_output=10)
    else:
        cfg.update(nms_score_threshold=0.03, nms_max_boxes=5, nms_iou_threshold=0.45, pretraining_weight='')
    return dict(cfg, **kw)


def _same(a, b):
    """same detections in the same order; the values to the round-off of the mocked convolutions (torch on the CPU at N = 3 against N = 1: other blockings)"""
    return (len(a) == 3 and len(b) == 3 and all(x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b)) and np.array_equal(a[2], b[2])
            and np.allclose(a[0], b[0], rtol=0, atol=1e-5) and np.allclose(a[1], b[1], rtol=1e-4, atol=1e-2))


@pytest.mark.parametrize('name', ['CenterNet', 'RefineDet320', 'PFPNetR'])
def test_host_logic_over_mocked_launches(name):
    """image slots, validation of test_batch_size, staging errors, and test_images (full batch, partial batch, one image) against test_one_image of a model
    built without test_batch_size on the same weights"""
    import odtk
    torch.set_num_threads(8)
    cls = getattr(odtk, name)
    g = torch.Generator().manual_seed(3)
    imgs = torch.rand(4, 64, 64, 3, generator=g)                     # (pixels in [0, 1): a net with untrained statistics stays out of saturation)
    with mocked():
        one = cls(_config(name), None)
        m = cls(_config(name, test_batch_size=3), None)
        assert one.batch_size == 1 and tuple(one.images.shape) == (1, 64, 64, 3)
        assert m.batch_size == 3 and tuple(m.images.shape) == (3, 64, 64, 3) and all(a.N == 3 for a in m.acts.values())
        if name == 'CenterNet':
            assert tuple(m.keypoints.shape) == (3, 16, 16, 20) and tuple(m.offset.shape) == tuple(m.size.shape) == (3, 16, 16, 2)
        else:
            A = m.A
            assert A == 3 * (64 + 16 + 4 + 1) and [tuple(t.shape) for t in (m.arm_loc, m.arm_conf, m.odm_loc, m.odm_conf)] == [(3, A, 4), (3, A, 2), (3, A, 4), (3, A, 21)]
        for bad in (0, True, 2.5):
            with pytest.raises(ValueError, match='test_batch_size'):
                cls(_config(name, test_batch_size=bad), None)
        for bad in (imgs.numpy(), imgs[:0].numpy(), imgs[:2, :63].numpy()):
            with pytest.raises(ValueError, match='test_images'):
                m.test_images(bad)
        with pytest.raises(ValueError, match='test_images'):
            one.test_images(imgs[:2].numpy())
        m.load_oracle_params(one.export_params())
        want = [one.test_one_image(imgs[n: n + 1].numpy()) for n in range(3)]
        assert all(len(w[0]) > 0 for w in want)
        full = m.test_images(imgs[:3].numpy())
        assert len(full) == 3 and all(_same(a, b) for a, b in zip(full, want))
        for s, b, c in full:
            assert s.dtype == np.float32 and b.dtype == np.float32 and c.dtype == np.int32 and b.shape == (len(s), 4) and c.shape == s.shape
        m.test_images(imgs[1:4].numpy())                                 # the tail slot holds another image than in the full batch
        part = m.test_images(imgs[:2].numpy())
        assert len(part) == 2 and all(_same(a, b) for a, b in zip(part, want))
        assert _same(m.test_one_image(imgs[2:3].numpy()), want[2])     # a model with test_batch_size > 1: the batched path with one image
        assert _same(one.test_images(imgs[:1].numpy())[0], want[0])    # a model without the key: one slot
        print(name, 'detections per image', [len(w[0]) for w in want])


def test_centernet_read_back_layout_on_a_hand_filled_buffer():
    """counts | scores | bbox | class_id in one buffer of 4-byte words; an image with count 0; rows behind a count are not returned"""
    from odtk import heads
    N, K = 3, 4
    t = heads.CenterNetBatched(N, 8, 8, K, 'cpu')
    assert t.words.numel() == N + 6 * N * K and t.host is None
    w = t.words.numpy()
    w[:N] = [2, 0, 4]
    sc = np.arange(N * K, dtype=np.float32) + 0.5
    bb = 100.0 + np.arange(N * K * 4, dtype=np.float32)
    ci = 1000 + np.arange(N * K, dtype=np.int32)
    w[N: N + N * K] = sc.view(np.int32)
    w[N + N * K: N + 5 * N * K] = bb.view(np.int32)
    w[N + 5 * N * K:] = ci
    assert torch.equal(t.counts, torch.tensor([2, 0, 4], dtype=torch.int32))
    assert torch.equal(t.scores, torch.from_numpy(sc).view(N, K)) and torch.equal(t.bbox, torch.from_numpy(bb).view(N, K, 4))
    assert torch.equal(t.class_id, torch.from_numpy(ci).view(N, K))
    got = t.read()
    assert [len(d[0]) for d in got] == [2, 0, 4]
    for n, k in enumerate((2, 0, 4)):
        s, b, c = got[n]
        assert s.dtype == np.float32 and b.dtype == np.float32 and c.dtype == np.int32 and b.shape == (k, 4) and c.shape == (k,)
        assert np.array_equal(s, sc[n * K: n * K + k]) and np.array_equal(b, bb.reshape(N, K, 4)[n, :k]) and np.array_equal(c, ci[n * K: n * K + k])
    assert len(t.read(2)) == 2 and len(t.read(2)[1][0]) == 0
    got[0][0][:] = -1.0                                                 # copies: the next read-back does not change what was handed out
    assert np.array_equal(t.read()[0][0], sc[:2])
