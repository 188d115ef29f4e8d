"""CPU tier of soft-NMS: self-checks of the oracle (tests/soft_nms_cases.py), the seeds of the Gaussian cases against their preconditions, validation of the
config keys over mocked launches, the two entry points in the header / the built library / _lib.SIGNATURES, and the kernel cases of
tests/test_gpu_soft_nms.py run from the source of csrc/soft_nms.hip under the fiber emulation (tests/hip_cpu_backend.py) at the small n."""
import contextlib
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import hip_cpu_backend as HC
import mock_ops
import soft_nms_cases as SC

NEW = ('odtk_soft_nms_image_class', 'odtk_detection_pack_scored')


# ---------------------------------------------------------------- the oracle
def test_oracle_hard_equals_the_greedy_reference():
    """method 0 of the oracle against the NonMaxSuppressionV3 restatement of oracle/nms_ref.cpp (oracle.ssd300_ref.nms) on a seeded case"""
    from oracle import ssd300_ref as R
    boxes, scores, valid = SC.random_problem(3, 2, 3, 400, (1.0, 0.5, 0.1), special=False)
    total = 0
    for img in range(2):
        for c in range(3):
            rows = np.nonzero(valid[img, :, c])[0]
            want = rows[R.nms(boxes[img, rows], scores[img, rows, c], 15, 0.5).astype(np.int64)]
            picks, sc, _ = SC.soft_nms_ref(boxes[img], scores[img, :, c], valid[img, :, c] == 1, 15, 0, 0.5)
            assert np.array_equal(picks, want) and np.array_equal(sc, scores[img, picks, c]), (img, c)
            total += len(picks)
    assert total > 30


def test_oracle_linear_with_iou_threshold_1_decays_nothing():
    boxes, scores, valid = SC.random_problem(4, 1, 1, 200, (1.0,), special=False)
    picks, sc, st = SC.soft_nms_ref(boxes[0], scores[0, :, 0], valid[0, :, 0] == 1, 50, 1, 1.0, min_score=0.0)
    order = np.argsort(-scores[0, :, 0], kind='stable')[:50]
    assert np.array_equal(picks, order) and np.array_equal(sc, scores[0, order, 0]) and st['decayed'] == 0 and st['killed'] == 0


def test_oracle_gaussian_scores_do_not_increase():
    boxes, scores, valid = SC.random_problem(5, 1, 1, 300, (1.0,), special=False)
    for sigma in (0.5, 0.1):
        picks, sc, st = SC.soft_nms_ref(boxes[0], scores[0, :, 0], valid[0, :, 0] == 1, 60, 2, 0.5, sigma, 0.01)
        assert len(picks) > 10 and st['decayed'] > 0 and bool((np.diff(sc) <= 0).all())
        assert len(set(picks.tolist())) == len(picks)


@pytest.mark.parametrize('n,sigma', sorted(SC.GAUSS_SEEDS))
def test_gaussian_seeds_meet_the_preconditions(n, sigma):
    ok, gap, margin, npicks = SC.gauss_preconditions(n, sigma, SC.GAUSS_SEEDS[(n, sigma)])
    assert ok and npicks > 20, (gap, margin, npicks)


# ---------------------------------------------------------------- config keys, over mocked launches
SSD_CFG = {'mode': 'test', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 8,
           'nms_score_threshold': 0.06, 'nms_max_boxes': 5, 'nms_iou_threshold': 0.5, 'pretraining_weight': '', 'verbose': False, 'device': 'cpu',
           'compute_dtype': 'f32'}


def test_config_keys_are_validated():
    import odtk
    import test_gpu_centernet_model as TC
    bad = [('nms_method', 'soft'), ('nms_method', 1), ('nms_method', None), ('nms_method', 'Linear'),
           ('soft_nms_sigma', 0), ('soft_nms_sigma', -0.5), ('soft_nms_sigma', '0.5'), ('soft_nms_sigma', float('nan')), ('soft_nms_sigma', True),
           ('soft_nms_min_score', -0.1), ('soft_nms_min_score', 'x'), ('soft_nms_min_score', float('inf')), ('soft_nms_min_score', None)]
    with mock_ops.installed():
        for key, value in bad:
            with pytest.raises(ValueError, match=key):
                odtk.SSD300(dict(dict(SSD_CFG, nms_method='linear'), **{key: value}), None)
        m = odtk.SSD300(dict(SSD_CFG, nms_method='gaussian', soft_nms_sigma=0.25), None)
        assert (m.nms_method, m.soft_nms_sigma, m.soft_nms_min_score) == ('gaussian', 0.25, 0.06)
        m.nms_score_threshold = 0.3
        assert m.soft_nms_min_score == 0.3                                  # the default follows the score threshold
        assert m._nms_params() == dict(method='gaussian', sigma=0.25, min_score=0.3)
        m = odtk.SSD300(dict(SSD_CFG, soft_nms_min_score=0), None)
        assert (m.nms_method, m.soft_nms_sigma, m.soft_nms_min_score) == ('hard', 0.5, 0.0)
        cn = dict(TC.CONFIG, mode='test', device='cpu')
        for method in ('linear', 'gaussian', 'soft'):
            with pytest.raises(ValueError, match='nms_method'):
                odtk.CenterNet(dict(cn, nms_method=method), None)
        odtk.CenterNet(dict(cn, nms_method='hard'), None)


def test_batched_tail_allocates_the_score_table_for_soft_methods_only():
    from odtk import heads
    assert heads.BatchedTail(2, 50, 3, 5, 'cpu').out_score is None and heads.BatchedTail(2, 50, 3, 5, 'cpu', method='hard').method == 0
    t = heads.BatchedTail(2, 50, 3, 5, 'cpu', method='gaussian', sigma=0.25, min_score=0.1)
    assert tuple(t.out_score.shape) == (2, 3, 5) and (t.method, t.sigma, t.min_score) == (2, 0.25, 0.1)


def test_symbols_in_library_header_and_signatures():
    import ctypes as C
    from odtk import _lib
    exported = subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()
    header = open(os.path.join(HC.ROOT, 'include', 'odtk.h')).read()
    kinds = {'int': C.c_int, 'float': C.c_float, 'long long': C.c_longlong}
    for n in NEW:
        assert f' T {n}\n' in exported and f'{n}(' in header and n in _lib.SIGNATURES
        params = header.split(f'int {n}(')[1].split(');')[0].split(',')
        want = [C.c_void_p if '*' in p else kinds[p.strip().rsplit(' ', 1)[0]] for p in params]
        assert _lib.SIGNATURES[n] == (C.c_int, want), n


# ---------------------------------------------------------------- the kernels from source under the fiber emulation
@contextlib.contextmanager
def emulated():
    """the emulation with csrc/detect_batched.hip and csrc/soft_nms.hip in the build (the pattern of test_cpu_batched_inference.emulated); the NMS of
    boxes.hip stands in as hip_cpu_backend has it"""
    from odtk import ops
    files, lib, tmp = list(HC.KERNEL_FILES), HC._LIB, tempfile.tempdir
    HC.KERNEL_FILES = files + ['detect_batched.hip', 'soft_nms.hip']
    HC._LIB = None
    tempfile.tempdir = os.path.join(tempfile.gettempdir(), f'odtk_cpu_soft_nms_{os.getuid()}')
    os.makedirs(tempfile.tempdir, exist_ok=True)
    try:
        with HC.installed() as names:
            assert all(n in names for n in NEW)
            old = ops.nms_image_class
            ops.nms_image_class = mock_ops.nms_image_class_via(ops.nms_batched)
            try:
                yield
            finally:
                ops.nms_image_class = old
    finally:
        HC.KERNEL_FILES, HC._LIB, tempfile.tempdir = files, lib, tmp


@pytest.mark.parametrize('with_n_dev', [False, True])
@pytest.mark.parametrize('n', [1, 63, 65, 1025, 2049])
def test_emulated_hard_equals_greedy_nms(n, with_n_dev):
    """the emulation's stand-in for odtk_nms_image_class is the oracle's NonMaxSuppressionV3; 2049 takes the path above the compaction capacity"""
    with emulated():
        SC.check_hard('cpu', n, with_n_dev)


@pytest.mark.parametrize('n', [65, 1025])
def test_emulated_linear_equals_the_oracle_bit_for_bit(n):
    with emulated():
        SC.check_linear('cpu', n)


@pytest.mark.parametrize('n,sigma', sorted(SC.GAUSS_SEEDS))
def test_emulated_gaussian_within_the_derived_bound(n, sigma):
    """(here expf is the host's libm, not the device's: the same bound holds for a 1-ulp expf)"""
    with emulated():
        SC.check_gaussian('cpu', n, sigma)


def test_emulated_refusals_and_pack_scored():
    with emulated():
        assert SC.check_refusals('cpu') == 14
        SC.check_pack_scored('cpu')
