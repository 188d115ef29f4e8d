"""CPU tier of the wide-row kernels (more than 31 object classes in SSD300 / SSD512 / RetinaNet, more than 64 in FCOS).
  * the kernels of csrc/boxes.hip, csrc/retina.hip, csrc/dense_heads.hip and csrc/detect_batched.hip run FROM SOURCE under the fiber emulation
    (test_cpu_batched_inference.emulated), through the bodies of the GPU cases (tests/wide_row_cases.py): C in {33, 64, 65, 81, 255, 256} against the float64
    restatements, the refusal at 257, bit-identical reruns;
  * host logic over mocked launches (tests/mock_ops.py): SSD300, RetinaNet and FCOS construct with num_classes 80, their prediction tensors have the widths
    that follows from, and the constructors raise ValueError above the limit."""
import pytest
import torch

import test_cpu_batched_inference as TB
import wide_row_cases as W


# ---------------------------------------------------------------- the kernels from source under the emulation
@pytest.mark.parametrize('C', W.CLASSES)
@pytest.mark.parametrize('batched', [False, True])
def test_emulated_ssd_decode(C, batched):
    with TB.emulated():
        W.check_ssd_decode(C, 'cpu', batched)


@pytest.mark.parametrize('C', W.CLASSES)
@pytest.mark.parametrize('batched', [False, True])
def test_emulated_retina_decode(C, batched):
    with TB.emulated():
        W.check_retina_decode(C, 'cpu', batched)


@pytest.mark.parametrize('C', W.CLASSES)
def test_emulated_ssd_loss(C):
    with TB.emulated():
        W.check_ssd_loss(C, 'cpu')


@pytest.mark.parametrize('C', W.CLASSES)
def test_emulated_retina_loss(C):
    with TB.emulated():
        W.check_retina_loss(C, 'cpu')


@pytest.mark.parametrize('C', W.CLASSES)
def test_emulated_fcos_loss(C):
    with TB.emulated():
        W.check_fcos_loss(C, 'cpu')


def test_emulated_one_thread_kernels_at_their_limit():
    """C = 32 stays on the one-thread-per-row kernels (C = 64 on FCOS's one-word kernel: in W.CLASSES): the same restatement, the bound of a 31-add sum"""
    with TB.emulated():
        for batched in (False, True):
            W.check_ssd_decode(32, 'cpu', batched)
            W.check_retina_decode(32, 'cpu', batched)
        W.check_ssd_loss(32, 'cpu')
        W.check_retina_loss(32, 'cpu')


# The four places where the host picks a kernel from C, and what pins each to the one-thread kernel.  Every pattern must be found exactly once.
PINS = {'boxes.hip': [('    if (C <= MAXC) {\n        hipLaunchKernelGGL(ssd_decode_kernel,', '    if (true) {\n        hipLaunchKernelGGL(ssd_decode_kernel,'),
                      ('    if (C <= MAXC) hipLaunchKernelGGL(ssd_loss_kernel,', '    if (true) hipLaunchKernelGGL(ssd_loss_kernel,')],
        'retina.hip': [('    if (C > RL_MAXC) {', '    if (false) {')],
        'dense_heads.hip': [('    const bool wide = C > DH_MAXC;', '    const bool wide = false;')]}


def _pinned_build():
    """the emulated build of TB.emulated() with the dispatch of the seven entry points pinned to the one-thread kernels: calling an entry point of THIS
    library is calling ssd_decode_kernel, ssd_loss_kernel, retina_loss_kernel and fcos_level_kernel directly"""
    import ctypes
    import hashlib
    import os
    import subprocess
    import tempfile
    import hip_cpu_backend as HC
    files = list(HC.KERNEL_FILES) + [f for f in ['detect_batched.hip'] if f not in HC.KERNEL_FILES]
    texts = {}
    for f in files:
        text = open(os.path.join(HC.CSRC, f)).read()
        for old, new in PINS.get(f, []):
            assert text.count(old) == 1, (f, old)
            text = text.replace(old, new)
        texts[f] = HC.DYN_SMEM.sub(lambda m: f'{m.group(1)}* {m.group(2)} = reinterpret_cast<{m.group(1)}*>(hipcpu::dynamic_smem());', text)
    extra = [os.path.join(HC.HERE, 'hip_cpu', 'stubs.cpp'), os.path.join(HC.HERE, 'hip_cpu', 'hip', 'hip_runtime.h'), os.path.join(HC.CSRC, 'wide_row.h'),
             os.path.join(HC.CSRC, 'common.h')]
    h = hashlib.sha256(''.join(texts[f] for f in files).encode())
    for f in extra:
        h.update(open(f, 'rb').read())
    so = os.path.join(tempfile.gettempdir(), f'libodtk_cpu_pinned_{os.getuid()}_{h.hexdigest()[:16]}.so')
    if not os.path.exists(so):
        work = tempfile.mkdtemp(prefix='odtk_cpu_pinned_')
        copies = []
        for f in files:
            copies.append(os.path.join(work, f + '.cpp'))
            open(copies[-1], 'w').write(texts[f])
        tmp = so + f'.{os.getpid()}.tmp'
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-I', os.path.join(HC.HERE, 'hip_cpu'), '-I', HC.CSRC]
                              + copies + [extra[0], '-o', tmp])
        os.replace(tmp, so)
    return ctypes.CDLL(so)


def test_emulated_dispatch_at_the_limit_is_the_one_thread_kernel():
    """every output of the seven entry points at C = 32 (FCOS: 64) equals, byte for byte, what the one-thread kernels give when the host cannot pick anything
    else; and one class more does NOT (the sum of exponentials changes its order there: the comparison can tell the kernels apart)"""
    import numpy as np
    import hip_cpu_backend as HC
    with TB.emulated():
        got = W.limit_outputs('cpu')
        wide33 = W.ssd_decode_run(33, 'cpu', True)[0].numpy()
        lib = HC._LIB
        HC._LIB = _pinned_build()
        try:
            with HC.installed():
                want = W.limit_outputs('cpu')
                narrow33 = W.ssd_decode_run(33, 'cpu', True)[0].numpy()
        finally:
            HC._LIB = lib
    assert sorted(got) == sorted(want) and len(got) > 20
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert not np.array_equal(wide33, narrow33)


def test_emulated_reruns_are_bit_identical():
    with TB.emulated():
        W.check_rerun('cpu')


def test_emulated_refusal_names_the_limit():
    with TB.emulated():
        W.check_refusals('cpu')


def test_library_version():
    from odtk import _lib
    assert _lib.load().odtk_version() >= 107


# ---------------------------------------------------------------- host logic over mocked launches
def _common(**kw):
    cfg = {'data_format': 'channels_last', 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 2, 'nms_score_threshold': 0.5, 'nms_max_boxes': 10,
           'nms_iou_threshold': 0.45, 'verbose': False, 'compute_dtype': 'f32', 'device': 'cpu'}
    return dict(cfg, **kw)


def _ssd_cfg(mode, num_classes):
    return _common(mode=mode, num_classes=num_classes, pretraining_weight='', use_graph=False, seed=0)


def _retina_cfg(mode, num_classes):
    return _common(mode=mode, num_classes=num_classes, is_bottleneck=True, residual_block_list=[3, 4, 6, 3], init_conv_filters=16, is_pretraining=False,
                   data_shape=[128, 128, 3], gamma=2.0, alpha=0.25)


def _fcos_cfg(mode, num_classes):
    return _common(mode=mode, num_classes=num_classes, data_shape=[128, 128, 3])


PROV = {'data_shape': [300, 300, 3], 'num_train': 2, 'num_val': 0, 'train_generator': [], 'val_generator': None}


@pytest.mark.parametrize('mode', ['train', 'test'])
def test_models_construct_with_80_classes(mode):
    import odtk
    torch.set_num_threads(8)
    prov = PROV if mode == 'train' else None
    with TB.mocked():
        m = odtk.SSD300(_ssd_cfg(mode, 80), prov)
        N = m.batch_size
        assert m.num_classes == 81 and m.row == 85 and tuple(m.pred.shape[:2]) == (N, 8828) and m.pred.shape[2] >= 85
        m = odtk.RetinaNet(_retina_cfg(mode, 80), prov)
        A = m.pconf.shape[1]
        assert m.num_classes == 81 and tuple(m.pconf.shape) == (N, A, 81) and tuple(m.pbox.shape) == (N, A, 4) and A == 9 * (256 + 64 + 16 + 4 + 1)
        m = odtk.FCOS(_fcos_cfg(mode, 80), prov)
        assert m.num_classes == 80 and [tuple(t.shape) for t in m.conf] == [(m.batch_size, s, s, 80) for s in (16, 8, 4, 2, 1)]


def test_constructors_refuse_more_classes_than_the_kernels_take():
    import odtk
    with TB.mocked():
        for cls, cfg, limit in ((odtk.SSD300, _ssd_cfg, 255), (odtk.SSD512, _ssd_cfg, 255), (odtk.RetinaNet, _retina_cfg, 255), (odtk.FCOS, _fcos_cfg, 256)):
            for bad in (limit + 1, 0, 2.5):
                with pytest.raises(ValueError, match=f'num_classes={bad!r} out of range: 1..{limit} object classes'):
                    cls(cfg('test', bad), None)
        # the limit itself constructs (FCOS: the cheapest of the three to build)
        m = odtk.FCOS(_fcos_cfg('test', 256), None)
        assert m.conf[0].shape[-1] == 256
        # RetinaNet's pre-training mode has its own 224 logits: the key plays no part there
        odtk.ops.check_num_classes('RetinaNet', 255, background=True)
        with pytest.raises(ValueError, match='256 logits per row with the background'):
            odtk.ops.check_num_classes('RetinaNet', 256, background=True)
