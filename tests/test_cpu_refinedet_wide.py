"""CPU tier of the wide ODM rows of RefineDet320 / PFPNetR (more than 95 object classes).
  * the kernels of csrc/refinedet.hip run FROM SOURCE under the fiber emulation (test_cpu_batched_inference.emulated), through the bodies of the GPU cases
    (tests/refinedet_wide_cases.py): C in {97, 128, 129, 200, 256} at A = 301 and A = 64 against the float64 restatements, the refusal at 257, reruns;
  * at C = 96 and C = 21 every output equals that of a build whose host cannot pick anything but the one-thread kernels;
  * host logic over mocked launches: the constructors of RefineDet320 and PFPNetR check the class count, YOLOv2's does not."""
import pytest
import torch

import refinedet_wide_cases as R
import test_cpu_batched_inference as TB


@pytest.mark.parametrize('A', R.SIZES)
@pytest.mark.parametrize('C', R.CLASSES)
@pytest.mark.parametrize('batched', [False, True])
def test_emulated_decode(C, A, batched):
    with TB.emulated():
        R.check_decode(C, A, 'cpu', batched)


@pytest.mark.parametrize('C', R.CLASSES)
def test_emulated_batched_decode_equals_two_single_calls(C):
    with TB.emulated():
        R.check_batched_equals_single(C, 301, 'cpu')


@pytest.mark.parametrize('C', R.CLASSES)
def test_emulated_first_of_two_equal_maxima_wins(C):
    with TB.emulated():
        R.check_tie_rows_are_kept(C, 301, 'cpu')


@pytest.mark.parametrize('A', R.SIZES)
@pytest.mark.parametrize('C', R.CLASSES)
def test_emulated_loss(C, A):
    with TB.emulated():
        R.check_loss(C, A, 'cpu')


def test_emulated_no_odm_negative_gives_the_nan_of_the_one_thread_kernel():
    with TB.emulated():
        R.check_nan_kind(129, 301, 'cpu')


def test_emulated_reruns_are_bit_identical():
    with TB.emulated():
        R.check_rerun('cpu')


def test_emulated_refusal_names_the_limit():
    with TB.emulated():
        R.check_refusals('cpu')


def test_library_version():
    from odtk import _lib
    assert _lib.load().odtk_version() >= 108


# The two places where the host of csrc/refinedet.hip picks a kernel from C, and what pins each to the one-thread kernel.  Every pattern must be found once.
PINS = {'refinedet.hip': [('    if (C <= RD_MAXC) hipLaunchKernelGGL(refinedet_loss_kernel,', '    if (true) hipLaunchKernelGGL(refinedet_loss_kernel,'),
                          ('    if (C <= RD_MAXC) {\n        hipLaunchKernelGGL(refinedet_decode_kernel,',
                           '    if (true) {\n        hipLaunchKernelGGL(refinedet_decode_kernel,')]}


def test_emulated_dispatch_up_to_96_logits_is_the_one_thread_kernel():
    """every output of the three entry points at C = 96 and C = 21 equals, byte for byte, what refinedet_loss_kernel and refinedet_decode_kernel give when
    the host cannot pick anything else (the pinned build of test_cpu_wide_rows, with the pins above)"""
    import hip_cpu_backend as HC
    import test_cpu_wide_rows as TW
    with TB.emulated():
        got = R.limit_outputs('cpu')
        lib, pins = HC._LIB, TW.PINS
        TW.PINS = PINS
        try:
            HC._LIB = TW._pinned_build()
            with HC.installed():
                want = R.limit_outputs('cpu')
        finally:
            HC._LIB, TW.PINS = lib, pins
    assert sorted(got) == sorted(want) and len(got) == 52
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


# ---------------------------------------------------------------- host logic over mocked launches
def _cfg(num_classes, **kw):
    cfg = {'mode': 'test', 'input_size': 320, 'data_format': 'channels_last', 'num_classes': num_classes, 'weight_decay': 1e-4, 'keep_prob': 0.5,
           'batch_size': 1, 'nms_score_threshold': 0.1, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.45, 'pretraining_weight': '', 'verbose': False,
           'compute_dtype': 'f32', 'device': 'cpu'}
    return dict(cfg, **kw)


@pytest.mark.parametrize('name', ['RefineDet320', 'PFPNetR'])
def test_constructors_refuse_more_classes_than_the_kernels_take(name):
    import odtk
    cls = getattr(odtk, name)
    with TB.mocked():
        for bad in (256, 300, 0, 2.5):
            with pytest.raises(ValueError, match=f'{cls.NAME}: num_classes={bad!r} out of range: 1..255 object classes .256 logits per row with the background'):
                cls(_cfg(bad), None)


def test_refinedet_constructs_with_120_classes_and_at_the_limit():
    import odtk
    torch.set_num_threads(8)
    with TB.mocked():
        for n in (120, 255):
            m = odtk.RefineDet320(_cfg(n), None)
            assert m.num_classes == n + 1 and tuple(m.odm_conf.shape[1:]) == (6375, n + 1)


def test_yolov2_is_not_held_to_the_row_limit():
    """YOLOv2 subclasses RefineDet320 for its plumbing but has no softmax row kernel: 300 classes construct"""
    import odtk
    from oracle import yolov2_ref as YR
    cfg = {'mode': 'test', 'is_pretraining': False, 'data_shape': [192, 224, 3], 'num_classes': 300, 'weight_decay': 1e-4, 'keep_prob': 0.5,
           'data_format': 'channels_last', 'batch_size': 1, 'coord_scale': 1, 'noobj_scale': 1, 'obj_scale': 5., 'class_scale': 1., 'nms_score_threshold': 0.5,
           'nms_max_boxes': 10, 'nms_iou_threshold': 0.5, 'rescore_confidence': False, 'priors': YR.PRIORS, 'verbose': False, 'compute_dtype': 'f32',
           'device': 'cpu'}
    with TB.mocked():
        m = odtk.YOLOv2(cfg, None)
        assert m.num_classes == 300
