"""VOC mAP (csrc/voc_eval.hip, odtk.VOCEvaluator, odtk.evaluate) on the CPU tier: the NumPy restatement (tests/voc_eval_ref.py) against hand-worked
answers, the kernel source through the CPU emulation of tests/hip_cpu/ against the restatement, and the evaluator's host logic on the emulated entry
points.  The emulated library is built here, under its own file name, from hip_cpu_backend.KERNEL_FILES + voc_eval.hip (stubs.cpp needs helpers of
boxes.hip / elementwise.hip) -- not added to the shared build, whose coverage report requires every entry point to run in one process."""
import contextlib
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hip_cpu_backend as B          # noqa: E402
import voc_eval_ref as R             # noqa: E402

_LIB = None


def emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    files = B.KERNEL_FILES + ['voc_eval.hip']
    srcs = [os.path.join(B.CSRC, f) for f in files]
    deps = srcs + [os.path.join(HERE, 'hip_cpu', 'stubs.cpp'), os.path.join(HERE, 'hip_cpu', 'hip', 'hip_runtime.h'), os.path.join(B.CSRC, 'common.h'),
                   os.path.join(B.CSRC, 'augment_resize.h'), os.path.join(B.ROOT, 'include', 'odtk.h'), os.path.abspath(__file__)]
    stamp = int(max(os.path.getmtime(f) for f in deps))
    so = os.path.join(tempfile.gettempdir(), f'libodtk_cpu_voc_{os.getuid()}_{stamp}.so')
    if not os.path.exists(so):
        work = tempfile.mkdtemp(prefix='odtk_cpu_voc_build_')
        copies = []
        for f in srcs:
            text = open(f).read()
            text = B.DYN_SMEM.sub(lambda m: f'{m.group(1)}* {m.group(2)} = reinterpret_cast<{m.group(1)}*>(hipcpu::dynamic_smem());', text)
            dst = os.path.join(work, os.path.basename(f) + '.cpp')
            open(dst, 'w').write(text)
            copies.append(dst)
        tmp = so + f'.{os.getpid()}.tmp'
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-I', os.path.join(HERE, 'hip_cpu'), '-I', B.CSRC]
                              + copies + [os.path.join(HERE, 'hip_cpu', 'stubs.cpp'), '-o', tmp])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    import odtk  # noqa: F401
    from odtk import _lib
    for n in ('odtk_voc_eval', 'odtk_voc_eval_workspace_bytes', 'odtk_last_error'):
        getattr(lib, n).restype, getattr(lib, n).argtypes = _lib.SIGNATURES[n]
    _LIB = lib
    return lib


class _Proxy:
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)


@contextlib.contextmanager
def emulated():
    """odtk.ops' C-ABI call, pointer and stream helpers bound to the emulated build (host tensors stand for device memory)"""
    import odtk  # noqa: F401
    from odtk import _lib, ops
    lib = emu_lib()

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        if rc != 0:
            raise _lib.OdtkError(f'libodtk (CPU emulation) error {rc}: {lib.odtk_last_error().decode()}')
    old = (ops.call, ops._p, ops._stream, _lib.load)
    ops.call, ops._p, ops._stream = call, (lambda t: None if t is None else C.c_void_p(t.data_ptr())), (lambda: None)
    _lib.load = lambda: _Proxy(lib)
    try:
        yield lib
    finally:
        ops.call, ops._p, ops._stream, _lib.load = old


# ---------------------------------------------------------------- the restatement against hand-worked answers
def _gt(*rows):
    return np.array(rows, np.float32).reshape(-1, 5)


def _box(y1, x1, y2, x2):
    return [y1, x1, y2, x2]


def _det(scores, boxes, cls):
    return (np.array(scores, np.float32), np.array(boxes, np.float32).reshape(-1, 4), np.array(cls, np.int32))


# one image, GT of class 0 at (0, 0, 10, 10) and (20, 20, 30, 30): [yc, xc, h, w, cls]
G2 = _gt([5, 5, 10, 10, 0], [25, 25, 10, 10, 0], [-1, -1, -1, -1, -1])


def test_ref_known_answers_both_metrics():
    # ranks: 0.9 hits GT0 (TP), 0.8 duplicate on GT0 (FP), 0.7 misses (FP), 0.6 hits GT1 (TP)
    d = _det([0.9, 0.8, 0.7, 0.6], [_box(0, 0, 10, 10), _box(0, 0, 10, 9), _box(50, 50, 60, 60), _box(20, 20, 30, 30)], [0, 0, 0, 0])
    r = R.evaluate([d], [G2], 1, metric='voc07')
    assert r['tp'].tolist() == [1, 0, 0, 1] and r['npos'].tolist() == [2]
    # rec = .5 .5 .5 1, prec = 1 .5 1/3 .5: t = 0 .. 0.5 -> 1 (6 points), t = 0.6 .. 1.0 -> 0.5 (5 points)
    assert r['AP'][0] == pytest.approx((6 * 1.0 + 5 * 0.5) / 11, abs=1e-15)
    r = R.evaluate([d], [G2], 1, metric='area')
    # envelope: 1 up to rec .5, then .5 up to rec 1 -> .5 * 1 + .5 * .5
    assert r['AP'][0] == pytest.approx(0.75, abs=1e-15) and r['mAP'] == pytest.approx(0.75, abs=1e-15)


def test_ref_tie_in_score_decides_tp_vs_fp():
    # two detections of score 0.8 on the same GT: the earlier sequence number is the TP, the later one the duplicate
    d0 = _det([0.8], [_box(0, 0, 10, 9)], [0])              # image 0 (sequence 0)
    d1 = _det([0.8, 0.8], [_box(0, 0, 9, 10), _box(0, 0, 10, 10)], [0, 0])
    g = _gt([5, 5, 10, 10, 0])
    r = R.evaluate([d0, d1], [g, g], 1)
    assert r['tp'].tolist() == [1, 1, 0]
    d = _det([0.8, 0.8], [_box(0, 0, 10, 9), _box(0, 0, 10, 10)], [0, 0])
    assert R.evaluate([d], [g], 1)['tp'].tolist() == [1, 0]     # the first of the tie takes it although the second fits better
    d = _det([0.8, 0.8], [_box(0, 0, 10, 10), _box(0, 0, 10, 9)], [0, 0])
    assert R.evaluate([d], [g], 1)['tp'].tolist() == [1, 0]


def test_ref_class_without_gt_is_nan_and_class_without_detections_is_zero():
    d = _det([0.9, 0.5], [_box(0, 0, 10, 10), _box(0, 0, 10, 10)], [0, 2])
    g = _gt([5, 5, 10, 10, 0], [5, 5, 10, 10, 1])
    for metric in ('voc07', 'area'):
        r = R.evaluate([d], [g], 3, metric=metric)
        # (voc07: eleven additions of 1 / 11 make 1.0000000000000002)
        assert abs(r['AP'][0] - 1.0) <= 1e-15 and r['AP'][1] == 0.0 and math.isnan(r['AP'][2])
        assert abs(r['mAP'] - 0.5) <= 1e-15 and r['npos'].tolist() == [1, 1, 0] and r['num_detections'].tolist() == [1, 0, 1]


def test_ref_recall_edge_at_0_3():
    # npos = 10, 3 TP first: rec reaches exactly 0.3 < t_3 = 0.30000000000000004 -> the precision of that point does NOT count at t_3
    assert 3 / 10.0 < np.arange(0., 1.1, 0.1)[3]
    rows = [[5 + 20 * k, 5, 10, 10, 0] for k in range(10)]
    boxes = [_box(20 * k, 0, 20 * k + 10, 10) for k in range(3)] + [_box(500, 500, 510, 510)] + [_box(20 * k, 0, 20 * k + 10, 10) for k in range(3, 4)]
    d = _det([0.9, 0.8, 0.7, 0.6, 0.5], boxes, [0] * 5)
    r = R.evaluate([d], [_gt(*rows)], 1)
    assert r['tp'].tolist() == [1, 1, 1, 0, 1]
    # t_0..t_2 -> 1; t_3 (0.30000000000000004): only rec 0.4 qualifies (prec 4/5); t_4 = 0.4 -> 0.8; t_5.. -> 0
    assert r['AP'][0] == pytest.approx((3 * 1.0 + 2 * 0.8) / 11, abs=1e-15)


# ---------------------------------------------------------------- kernel source through the CPU emulation
def _random_case(rng, n_img, C, max_det, max_gt, levels=8):
    dets, gts = [], []
    for _ in range(n_img):
        ng = int(rng.integers(0, max_gt + 1))
        yc, xc = rng.uniform(20, 280, ng), rng.uniform(20, 280, ng)
        h, w = rng.uniform(8, 80, ng), rng.uniform(8, 80, ng)
        cls = rng.integers(0, C, ng).astype(np.float32)
        g = np.stack([yc, xc, h, w, cls], 1).astype(np.float32)
        g = np.concatenate([g, -np.ones((int(rng.integers(0, 3)), 5), np.float32)])            # padding rows
        nd = int(rng.integers(0, max_det + 1))
        boxes = np.zeros((nd, 4), np.float32)
        dcls = rng.integers(0, C, nd).astype(np.int32)
        for k in range(nd):
            if ng and rng.random() < 0.7:                            # jittered copy of a GT box (its class mostly)
                j = int(rng.integers(0, ng))
                y1, x1, y2, x2 = yc[j] - h[j] / 2, xc[j] - w[j] / 2, yc[j] + h[j] / 2, xc[j] + w[j] / 2
                jit = rng.normal(0, 0.15, 4) * np.array([h[j], w[j], h[j], w[j]])
                boxes[k] = [y1 + jit[0], x1 + jit[1], y2 + jit[2], x2 + jit[3]]
                if rng.random() < 0.8:
                    dcls[k] = int(cls[j])
            else:
                y, x = rng.uniform(0, 260, 2)
                boxes[k] = [y, x, y + rng.uniform(5, 60), x + rng.uniform(5, 60)]
        scores = (rng.integers(1, levels + 1, nd) / levels).astype(np.float32)      # quantised: many ties
        dets.append((scores, boxes, dcls))
        gts.append(g)
    return dets, gts


def _run_evaluator(dets, gts, C, metric, iou=0.5):
    import odtk
    with emulated():
        ev = odtk.VOCEvaluator(C, iou, metric, device='cpu')
        for d, g in zip(dets, gts):
            ev.add(list(d), g)
        return ev.result()


def _check(r, ref):
    assert r['tp'].tolist() == ref['tp'].tolist()
    assert r['npos'].tolist() == ref['npos'].tolist()
    assert r['num_detections'].tolist() == ref['num_detections'].tolist()
    assert np.array_equal(np.isnan(r['AP']), np.isnan(ref['AP']))
    ok = ~np.isnan(ref['AP'])
    assert np.max(np.abs(r['AP'][ok] - ref['AP'][ok]), initial=0.0) <= 1e-12
    if ok.any():
        assert abs(r['mAP'] - ref['mAP']) <= 1e-12


@pytest.mark.parametrize('seed,n_img,C,max_det,max_gt', [(0, 1, 1, 12, 4), (1, 7, 3, 30, 5), (2, 40, 5, 25, 4), (3, 300, 4, 20, 3)])
@pytest.mark.parametrize('metric', ['voc07', 'area'])
def test_emulated_kernel_vs_ref(seed, n_img, C, max_det, max_gt, metric):
    rng = np.random.default_rng(seed)
    dets, gts = _random_case(rng, n_img, C, max_det, max_gt)
    _check(_run_evaluator(dets, gts, C, metric), R.evaluate(dets, gts, C, metric=metric))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_ref_fast_matches_ref(seed):
    rng = np.random.default_rng(100 + seed)
    dets, gts = _random_case(rng, 60, 4, 25, 6, levels=4)
    for metric in ('voc07', 'area'):
        a, b = R.evaluate(dets, gts, 4, metric=metric), R.evaluate_fast(dets, gts, 4, metric=metric)
        assert a['tp'].tolist() == b['tp'].tolist() and a['npos'].tolist() == b['npos'].tolist()
        assert np.array_equal(a['AP'], b['AP'], equal_nan=True)


def test_emulated_kernel_multi_tile_sort():
    # > one radix tile (4 096) of detections, 300 images (two image digits' worth of bits: 9), 12 classes: the multi-block scatter and scans
    rng = np.random.default_rng(7)
    dets, gts = _random_case(rng, 300, 12, 30, 4, levels=5)
    assert sum(len(d[0]) for d in dets) > 4096
    for metric in ('voc07', 'area'):
        _check(_run_evaluator(dets, gts, 12, metric), R.evaluate(dets, gts, 12, metric=metric))


def test_emulated_exact_answers_and_empty():
    rng = np.random.default_rng(11)
    _, gts = _random_case(rng, 20, 4, 0, 4)
    dets = []
    for g in gts:
        real = g[g[:, 4] >= 0]
        y1, x1 = real[:, 0] - real[:, 2] / 2, real[:, 1] - real[:, 3] / 2
        y2, x2 = real[:, 0] + real[:, 2] / 2, real[:, 1] + real[:, 3] / 2
        dets.append((np.ones(len(real), np.float32), np.stack([y1, x1, y2, x2], 1).astype(np.float32), real[:, 4].astype(np.int32)))
    for metric in ('voc07', 'area'):
        r = _run_evaluator(dets, gts, 4, metric)
        has = r['npos'] > 0
        assert np.all(np.abs(r['AP'][has] - 1.0) <= 1e-15) and np.all(np.isnan(r['AP'][~has]))
        empty = [(np.zeros(0, np.float32), np.zeros((0, 4), np.float32), np.zeros(0, np.int32)) for _ in gts]
        r = _run_evaluator(empty, gts, 4, metric)
        assert np.all(r['AP'][has] == 0.0) and r['tp'].size == 0


def test_emulated_non_finite_boxes_are_misses():
    # a diverged model's decode can emit inf / NaN coordinates: IoU 0 (fminf / fmaxf ignore NaN; a union that is not > 0 gives 0), no error
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    d = _det([0.9, 0.8, 0.7, 0.6], [[-inf, 0, inf, 10], [nan, 0, 10, 10], [0, 0, inf, inf], [0, 0, 10, 10]], [0, 0, 0, 0])
    g = _gt([5, 5, 10, 10, 0])
    ref = R.evaluate([d], [g], 1)
    assert ref['tp'].tolist() == [0, 0, 0, 1] and R.evaluate_fast([d], [g], 1)['tp'].tolist() == [0, 0, 0, 1]
    for metric in ('voc07', 'area'):
        _check(_run_evaluator([d], [g], 1, metric), R.evaluate([d], [g], 1, metric=metric))


def test_emulated_capacity_errors():
    from odtk import _lib, ops
    with emulated() as lib:
        assert lib.odtk_voc_eval_workspace_bytes(8 << 20, 2 << 20, 1 << 20, 1024) > 0
        for args in [((8 << 20) + 1, 0, 1, 1), (0, (2 << 20) + 1, 1, 1), (0, 0, (1 << 20) + 1, 1), (0, 0, 1, 1025), (0, 0, 0, 1)]:
            assert lib.odtk_voc_eval_workspace_bytes(*args) == -1
            assert 'outside the supported range' in lib.odtk_last_error().decode()
        with pytest.raises(_lib.OdtkError, match='outside the supported range'):
            ops.voc_eval_workspace(0, 0, 1, 2000, 'cpu')
        e = torch.empty(0)
        ws = torch.empty(1024, dtype=torch.uint8)
        with pytest.raises(_lib.OdtkError, match='num_classes=1025'):
            ops.voc_eval(e, e.view(0, 4), e.int(), e.int(), e.view(0, 5), e.int(), 1, 1025, 0.5, 'voc07', ws, e.byte(), torch.empty(1025).int(),
                         torch.empty(1025).double())


# ---------------------------------------------------------------- VOCEvaluator / evaluate() host logic
def test_evaluator_validation_errors():
    import odtk
    with pytest.raises(ValueError):
        odtk.VOCEvaluator(3, metric='coco')
    with pytest.raises(ValueError):
        odtk.VOCEvaluator(0)
    g = _gt([5, 5, 10, 10, 0])
    good = _det([0.9], [_box(0, 0, 10, 10)], [0])
    cases = [
        (list(_det([np.nan], [_box(0, 0, 1, 1)], [0])), g, 'non-finite score'),
        (list(_det([0.5], [_box(0, 0, 1, 1)], [3])), g, r'class_id -?[0-9]+ outside \[0, 3\)'),
        (list(_det([0.5], [_box(0, 0, 1, 1)], [-1])), g, r'class_id -?[0-9]+ outside \[0, 3\)'),
        (list(good), _gt([5, 5, 10, 10, 3]), 'num_classes'),
    ]
    for d, gt, msg in cases:
        ev = odtk.VOCEvaluator(3, device='cpu')
        ev.add(d, gt)
        with pytest.raises(ValueError, match=msg):
            ev.result()
    ev = odtk.VOCEvaluator(3, device='cpu')
    with pytest.raises(ValueError):
        ev.add(list(good)[:2], g)
    with pytest.raises(ValueError):
        ev.add([good[0], good[1][:, :3], good[2]], g)
    with pytest.raises(ValueError):
        ev.add(list(good), g[:, :4])


def test_evaluator_accumulates_in_sequence_order_and_resets():
    import odtk
    rng = np.random.default_rng(5)
    dets, gts = _random_case(rng, 12, 3, 15, 4)
    ref = R.evaluate(dets, gts, 3)
    with emulated():
        ev = odtk.VOCEvaluator(3, device='cpu')
        ev.add([torch.zeros(1), torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32)], torch.zeros(1, 5))
        ev.reset()
        assert ev.num_images == 0
        for d, g in zip(dets, gts):                                  # torch and numpy inputs mixed: the same staging
            ev.add([torch.from_numpy(d[0]), d[1], torch.from_numpy(d[2])], torch.from_numpy(g))
        r1 = ev.result()
        r2 = ev.result()                                             # result() does not consume the staged images
    _check(r1, ref)
    assert r1['tp'].tolist() == r2['tp'].tolist() and np.array_equal(r1['AP'], r2['AP'], equal_nan=True)
    # padding-only ground truth of every image: every class NaN, mAP NaN
    with emulated():
        ev = odtk.VOCEvaluator(2, device='cpu')
        ev.add(list(_det([0.5], [_box(0, 0, 1, 1)], [1])), _gt([-1, -1, -1, -1, -1]))
        r = ev.result()
    assert np.all(np.isnan(r['AP'])) and math.isnan(r['mAP']) and r['tp'].tolist() == [0]


class _CannedModel:
    """stand-in for a test-mode detector: test_one_image returns canned detections, one per call, and records what it was fed"""

    def __init__(self, dets, num_classes, val_generator=None, num_val=0):
        self.dets, self.fed = list(dets), []
        self.config = {'num_classes': num_classes}
        self.mode = 'test'
        self.dev = torch.device('cpu')
        self.data_provider = {'val_generator': val_generator, 'num_val': num_val}

    def test_one_image(self, images):
        assert images.shape[0] == 1
        self.fed.append(float(images[0, 0, 0, 0]))
        return list(self.dets[len(self.fed) - 1])


def _generator(gts, B, H=4):
    batches = []
    for s in range(0, len(gts), B):
        g = gts[s: s + B]
        pad = max(len(x) for x in g)
        gt = -np.ones((len(g), pad, 5), np.float32)
        for k, x in enumerate(g):
            gt[k, : len(x)] = x
        imgs = np.zeros((len(g), H, H, 3), np.float32)
        imgs[:, 0, 0, 0] = np.arange(s, s + len(g))
        batches.append((imgs, gt))
    return batches


def test_evaluate_drives_the_model_over_the_generator():
    import odtk
    rng = np.random.default_rng(9)
    dets, gts = _random_case(rng, 10, 3, 10, 4)
    ref = R.evaluate(dets, gts, 3, metric='area')
    with emulated():
        m = _CannedModel(dets, 3)
        r = odtk.evaluate(m, _generator(gts, 4), metric='area')
        assert m.fed == list(range(10))
        _check(r, ref)
        # num_images stops inside a batch; an (initializer, iterator) pair calls the initializer once
        calls = []
        m = _CannedModel(dets, 3)
        r = odtk.evaluate(m, (lambda: calls.append(1), _generator(gts, 4)), num_images=6)
        assert m.fed == list(range(6)) and calls == [1]
        _check(r, R.evaluate(dets[:6], gts[:6], 3))
        # defaults: the data provider's val_generator and num_val
        m = _CannedModel(dets, 3, val_generator=_generator(gts, 3), num_val=5)
        r = odtk.evaluate(m)
        assert m.fed == list(range(5))
        _check(r, R.evaluate(dets[:5], gts[:5], 3))
    with pytest.raises(ValueError, match='val_generator'):
        odtk.evaluate(_CannedModel(dets, 3))
