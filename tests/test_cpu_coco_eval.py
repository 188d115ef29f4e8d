"""COCO-style AP (csrc/voc_eval.hip odtk_coco_eval, odtk.COCOEvaluator, odtk.evaluate(metric='coco')) on the CPU tier: the NumPy restatement
(tests/coco_eval_ref.py) against hand-worked answers, its two forms against each other, the kernel source through the CPU emulation of
tests/test_cpu_voc_eval.py against the restatement, and the evaluator's host logic on the emulated entry points.

Comparison rule: match and npos equal, the NaN pattern equal, |AP - ref| <= 1e-12 and the same for recall (f64; 101 terms <= 1, error <= 101 * 2^-53)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coco_eval_ref as R            # noqa: E402
import test_cpu_voc_eval as TV       # noqa: E402
import voc_eval_ref as VR            # noqa: E402

_gt, _box, _det = TV._gt, TV._box, TV._det
ALL = [[0, 1e10]]


# ---------------------------------------------------------------- hand-worked sets (shared with the emulated-kernel test)
def hand_iou_on_threshold():
    # (0, 0, 10, 10) on (0, 0, 10, 20): intersection 100, union 200 -> IoU exactly 0.5
    return [_det([0.9], [_box(0, 0, 10, 10)], [0])], [_gt([5, 10, 10, 20, 0])], 1, dict(iou_thresholds=[0.5, 0.55], area_ranges=ALL)


def hand_equal_ious():
    # (0, 5, 10, 15) overlaps (0, 0, 10, 10) and (0, 10, 10, 20) by 50 / 150 each; the second detection fits the first row only
    d = _det([0.9, 0.8], [_box(0, 5, 10, 15), _box(0, 0, 10, 10)], [0, 0])
    return [d], [_gt([5, 5, 10, 10, 0], [5, 15, 10, 10, 0])], 1, dict(iou_thresholds=[0.3], area_ranges=ALL)


def hand_small_gt():
    # image 0: a 30 x 30 row (area 900) detected by its own box; image 1: a 32 x 32 row (area exactly 1024), no detection
    d0 = _det([0.9], [_box(0, 0, 30, 30)], [0])
    d1 = _det([], [], [])
    return [d0, d1], [_gt([15, 15, 30, 30, 0]), _gt([16, 16, 32, 32, 1])], 2, dict(iou_thresholds=[0.5])


def hand_unmatched_detection():
    d = _det([0.9], [_box(100, 100, 120, 120)], [0])
    return [d], [_gt([5, 5, 10, 10, 0])], 1, dict(iou_thresholds=[0.5])


def hand_non_ignored_first():
    # range 0 = [0, 500]: the 20 x 20 row counts, the 30 x 30 row is ignored; range 1 = everything
    d = _det([0.9, 0.8], [_box(0, 0, 30, 30), _box(0, 0, 30, 30)], [0, 0])
    return [d], [_gt([10, 10, 20, 20, 0], [15, 15, 30, 30, 0])], 1, dict(iou_thresholds=[0.4], area_ranges=[[0, 500], [0, 1e10]])


def hand_max_dets():
    boxes = [_box(0, 0, 10, 10), _box(50, 50, 60, 60), _box(100, 0, 110, 10), _box(100, 0, 110, 10), _box(0, 0, 10, 10)]
    d = _det([0.9, 0.8, 0.5, 0.5, 0.1], boxes, [0] * 5)
    return [d], [_gt([5, 5, 10, 10, 0], [105, 5, 10, 10, 0])], 1, dict(iou_thresholds=[0.5], max_dets=3)


def hand_worked_ap():
    d = _det([0.9, 0.8, 0.7], [_box(0, 0, 10, 10), _box(50, 50, 60, 60), _box(20, 20, 30, 30)], [0, 0, 0])
    return [d], [TV.G2], 1, dict(iou_thresholds=[0.5], area_ranges=ALL)


def hand_class_without_gt():
    d = _det([0.9, 0.5], [_box(0, 0, 10, 10), _box(0, 0, 10, 10)], [0, 2])
    return [d], [_gt([5, 5, 10, 10, 0], [5, 5, 10, 10, 1])], 3, dict(iou_thresholds=[0.5, 0.75])


HAND = [hand_iou_on_threshold, hand_equal_ious, hand_small_gt, hand_unmatched_detection, hand_non_ignored_first, hand_max_dets, hand_worked_ap,
        hand_class_without_gt]


def _ref(case, fast=False):
    dets, gts, C, kw = case
    return (R.evaluate_fast if fast else R.evaluate)(dets, gts, C, **kw)


def test_ref_iou_on_the_threshold_is_a_true_positive():
    case = hand_iou_on_threshold()
    r = _ref(case)
    assert r['match'][0, :, 0].tolist() == [1, 0]                      # TP at 0.5 (>=), FP at 0.55
    assert VR.evaluate(case[0], case[1], 1, iou_threshold=0.5)['tp'].tolist() == [0]      # the VOC matcher's > calls it a false positive


def test_ref_equal_ious_take_the_later_row():
    r = _ref(hand_equal_ious())
    assert r['match'][0, 0].tolist() == [1, 1]                         # had the first detection taken row 0, the second one would have nothing left


def test_ref_small_gt_and_the_inclusive_range_ends():
    r = _ref(hand_small_gt())
    assert r['match'][:, 0, 0].tolist() == [1, 1, 2, 2]                # all, small: TP; medium, large: its row is ignored -> ignored
    assert r['npos'].tolist() == [[1, 1], [1, 1], [0, 1], [0, 0]]      # area 1024 counts in small AND medium


def test_ref_unmatched_detection_by_its_own_area():
    r = _ref(hand_unmatched_detection())
    assert r['match'][:, 0, 0].tolist() == [0, 0, 2, 2]                # 20 x 20: FP in all and small, ignored in medium and large


def test_ref_non_ignored_rows_come_before_ignored_ones():
    r = _ref(hand_non_ignored_first())
    assert r['match'][0, 0].tolist() == [1, 2]     # IoU 4/9 with the counted row beats IoU 1 with the ignored one; the second takes the ignored row
    assert r['match'][1, 0].tolist() == [1, 1]     # nothing ignored: IoU 1 first, the other row (4/9 >= 0.4) second
    assert r['npos'].tolist() == [[1], [2]]


def test_ref_max_dets_keeps_the_best_and_the_lower_index_of_a_tie():
    r = _ref(hand_max_dets())
    assert np.all(r['match'][:, :, 3:] == 2)                           # the two lowest: code 2 everywhere
    assert r['match'][0, 0, :3].tolist() == [1, 0, 1]                  # of the two 0.5s the lower index stays (and is the TP)
    assert np.all(_ref(hand_max_dets()[:3] + (dict(iou_thresholds=[0.5], max_dets=5),))['match'][0, 0] == [1, 0, 1, 0, 0])


def test_ref_worked_ap():
    r = _ref(hand_worked_ap())
    assert r['match'][0, 0].tolist() == [1, 0, 1] and r['npos'].tolist() == [[2]]
    # recall .5 .5 1, envelope 1 2/3 2/3: q = 1 for x <= 0.5 (51 points), else 2/3
    assert abs(r['ap'][0, 0, 0] - (51 + 50 * 2 / 3) / 101) <= 1e-15 and r['recall'][0, 0, 0] == 1.0
    assert abs(r['AP'] - (51 + 50 * 2 / 3) / 101) <= 1e-15 and math.isnan(r['AP75']) and math.isnan(r['APs'])


def test_ref_class_without_gt_is_nan_and_left_out_of_the_means():
    r = _ref(hand_class_without_gt())
    assert np.all(np.isnan(r['ap'][:, :, 2])) and np.all(np.isnan(r['recall'][:, :, 2]))
    assert np.all(np.abs(r['ap'][0, :, 0] - 1.0) <= 1e-15) and np.all(r['ap'][0, :, 1] == 0.0) and np.all(r['recall'][0, :, 1] == 0.0)
    assert abs(r['AP'] - 0.5) <= 1e-15 and abs(r['AP50'] - 0.5) <= 1e-15 and abs(r['AR'] - 0.5) <= 1e-15
    assert math.isnan(r['AP_per_class'][2]) and r['num_detections'].tolist() == [1, 0, 1]


# ---------------------------------------------------------------- the two forms of the restatement
def _same(a, b, tol=1e-12):
    assert np.array_equal(a['match'], b['match'])
    assert np.array_equal(a['npos'], b['npos'])
    for k in ('ap', 'recall'):
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
        ok = ~np.isnan(b[k])
        assert np.max(np.abs(a[k][ok] - b[k][ok]), initial=0.0) <= tol, (k, np.max(np.abs(a[k][ok] - b[k][ok])))
    for k in ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR'):
        assert math.isnan(a[k]) == math.isnan(b[k]) and (math.isnan(b[k]) or abs(a[k] - b[k]) <= tol), k


@pytest.mark.parametrize('seed', [0, 1])
def test_ref_fast_matches_ref(seed):
    dets, gts = R.random_case(200 + seed, 64, 20, 30, 4, levels=4)
    a, b = R.evaluate(dets, gts, 20, max_dets=8), R.evaluate_fast(dets, gts, 20, max_dets=8)
    _same(b, a)
    assert {0, 1, 2} <= set(np.unique(a['match'][0])) and (a['match'][0, 0] != a['match'][0, -1]).any() and (a['match'][0] != a['match'][2]).any()


@pytest.mark.parametrize('make', HAND, ids=[f.__name__ for f in HAND])
def test_ref_fast_matches_ref_on_the_hand_worked_sets(make):
    _same(_ref(make(), fast=True), _ref(make()))


# ---------------------------------------------------------------- kernel source through the CPU emulation
def _run(dets, gts, C, **kw):
    import odtk
    with TV.emulated():
        ev = odtk.COCOEvaluator(C, device='cpu', **kw)
        for d, g in zip(dets, gts):
            ev.add(list(d), g)
        return ev.result()


@pytest.mark.parametrize('make', HAND, ids=[f.__name__ for f in HAND])
def test_emulated_kernel_on_the_hand_worked_sets(make):
    dets, gts, C, kw = make()
    _same(_run(dets, gts, C, **kw), R.evaluate(dets, gts, C, **kw))


THR16 = np.linspace(0.2, 0.95, 16)
EMU_CASES = {
    '1img-3cls-40det': ((1, 1, 3, 40, 6, 4, 2), dict(max_dets=7)),     # (segments of ~13 detections: the cap bites)
    '64img-20cls-30det': ((2, 64, 20, 30, 4, 8, 2), {}),
    'one-class-5000det': ((3, 100, 1, 50, 6, 16, 1), {}),               # crosses the 2 048-position AP chunk and the 4 096-element radix tile
    '16thr-x-4ranges': ((5, 6, 3, 30, 5, 4, 2), dict(iou_thresholds=THR16)),
    '1thr-x-1range': ((6, 6, 3, 30, 5, 4, 2), dict(iou_thresholds=[0.5], area_ranges=ALL)),
}


@pytest.mark.parametrize('name', list(EMU_CASES))
def test_emulated_kernel_vs_ref(name):
    (seed, n, C, dpi, gpi, levels, cpi), kw = EMU_CASES[name]
    dets, gts = R.random_case(seed, n, C, dpi, gpi, levels, cpi)
    r, ref = _run(dets, gts, C, **kw), R.evaluate_fast(dets, gts, C, **kw)
    _same(r, ref)
    assert r['num_detections'].tolist() == ref['num_detections'].tolist() and r['match'].shape == ref['match'].shape
    if name == 'one-class-5000det':
        assert r['num_detections'][0] == 5000
    if name == '16thr-x-4ranges':
        assert r['ap'].shape == (4, 16, 3)


def test_emulated_empty_sides():
    dets, gts = R.random_case(8, 5, 3, 6, 3)
    empty = [(np.zeros(0, np.float32), np.zeros((0, 4), np.float32), np.zeros(0, np.int32)) for _ in gts]
    r = _run(empty, gts, 3)
    has = r['npos'] > 0
    assert r['match'].shape == (4, 10, 0) and has[0].any()
    assert np.all(r['ap'][np.broadcast_to(has[:, None, :], r['ap'].shape)] == 0.0) and np.all(np.isnan(r['ap'][:, 0, :][~has]))
    assert np.all(r['recall'][0][:, has[0]] == 0.0) and r['AP'] == 0.0 and r['AR'] == 0.0
    _same(r, R.evaluate(empty, gts, 3))
    no_gt = [np.zeros((0, 5), np.float32) for _ in dets]
    r = _run(dets, no_gt, 3)
    assert np.all(np.isnan(r['ap'])) and math.isnan(r['AP']) and math.isnan(r['AR']) and np.all(r['npos'] == 0)
    _same(r, R.evaluate(dets, no_gt, 3))
    assert set(np.unique(r['match'][0])) == {0}                          # nothing to match: every detection is a false positive in 'all'


def test_emulated_limits():
    from odtk import _lib, ops
    with TV.emulated() as lib:
        for n in ('odtk_coco_eval', 'odtk_coco_eval_workspace_bytes'):
            getattr(lib, n).restype, getattr(lib, n).argtypes = _lib.SIGNATURES[n]
        assert lib.odtk_coco_eval_workspace_bytes(10, 10, 1, 20, 16, 4) > 0
        for T, Rn in [(65, 1), (13, 5), (0, 1), (1, 0)]:
            assert lib.odtk_coco_eval_workspace_bytes(10, 10, 1, 20, T, Rn) == -1
            assert 'num_thr * num_areas <= 64' in lib.odtk_last_error().decode()
        assert lib.odtk_coco_eval_workspace_bytes(0, 0, 1, 1025, 1, 1) == -1 and 'outside the supported range' in lib.odtk_last_error().decode()
        e = torch.empty(0)
        ws = torch.empty(1 << 16, dtype=torch.uint8)
        out = lambda *s: torch.empty(*s, dtype=torch.float64)           # noqa: E731
        args = (e, e.view(0, 4), e.int(), e.int(), e.view(0, 5), e.int(), 1, 2)
        with pytest.raises(_lib.OdtkError, match='max_dets 0'):
            ops.coco_eval(*args, [0.5], ALL, 0, ws, e.byte(), torch.empty(1, 2).int(), out(1, 1, 2), out(1, 1, 2))
        with pytest.raises(_lib.OdtkError, match='num_thr=13 num_areas=5'):
            ops.coco_eval(*args, np.linspace(0.3, 0.9, 13), np.tile([[0, 1e10]], (5, 1)), 100, ws, e.byte(), torch.empty(5, 2).int(), out(5, 13, 2),
                          out(5, 13, 2))


# ---------------------------------------------------------------- COCOEvaluator / evaluate() host logic
def test_evaluator_validation_errors():
    import odtk
    with pytest.raises(ValueError):
        odtk.VOCEvaluator(3, metric='coco')                              # the VOC evaluator keeps refusing it
    assert odtk.voc_eval.METRICS == ('voc07', 'area')
    bad = [dict(iou_thresholds=[0.75, 0.5]), dict(iou_thresholds=[0.5, 0.5]), dict(iou_thresholds=[0.5, 1.0]), dict(iou_thresholds=[-0.1]),
           dict(iou_thresholds=[]), dict(area_ranges=[[10, 5]]), dict(area_ranges=[[0, 1, 2]]), dict(iou_thresholds=np.linspace(0.1, 0.9, 17)),
           dict(max_dets=0), dict(max_dets=-3), dict(max_dets=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            odtk.COCOEvaluator(3, device='cpu', **kw)
    with pytest.raises(ValueError):
        odtk.COCOEvaluator(0, device='cpu')
    with pytest.raises(ValueError, match='exceeds 64'):
        odtk.COCOEvaluator(3, iou_thresholds=np.linspace(0.1, 0.9, 13), area_ranges=np.tile([[0, 1e10]], (5, 1)), device='cpu')
    g = _gt([5, 5, 10, 10, 0])
    good = _det([0.9], [_box(0, 0, 10, 10)], [0])
    cases = [
        (list(_det([np.nan], [_box(0, 0, 1, 1)], [0])), g, 'non-finite score'),
        (list(_det([0.5], [_box(0, 0, 1, 1)], [3])), g, r'class_id -?[0-9]+ outside \[0, 3\)'),
        (list(good), _gt([5, 5, 10, 10, 3]), 'num_classes'),
    ]
    for d, gt, msg in cases:                                             # the messages of VOCEvaluator
        ev = odtk.COCOEvaluator(3, device='cpu')
        ev.add(d, gt)
        with pytest.raises(ValueError, match=msg):
            ev.result()
    ev = odtk.COCOEvaluator(3, device='cpu')
    with pytest.raises(ValueError):
        ev.add(list(good)[:2], g)
    with pytest.raises(ValueError):
        ev.add(list(good), g[:, :4])
    with pytest.raises(ValueError, match='iou_threshold'):
        odtk.evaluate(TV._CannedModel([good], 3), TV._generator([g], 1), metric='coco', iou_threshold=0.6)


def test_evaluator_summary_keys_and_nan_rules():
    import odtk
    dets, gts = R.random_case(9, 12, 3, 15, 4)
    keys = {'AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR', 'AP_per_class', 'ap', 'recall', 'npos', 'match', 'num_detections', 'iou_thresholds',
            'area_ranges'}
    with TV.emulated():
        ev = odtk.COCOEvaluator(3, device='cpu')
        ev.add([torch.zeros(1), torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32)], torch.zeros(1, 5))
        ev.reset()
        assert ev.num_images == 0
        for d, g in zip(dets, gts):                                      # torch and numpy inputs mixed: the same staging
            ev.add([torch.from_numpy(d[0]), d[1], torch.from_numpy(d[2])], torch.from_numpy(g))
        assert ev.num_images == 12
        r = ev.result()
    ref = R.evaluate(dets, gts, 3)
    _same(r, ref)
    assert set(r) == keys
    assert r['ap'].shape == (4, 10, 3) and r['recall'].shape == (4, 10, 3) and r['npos'].shape == (4, 3) and r['match'].shape == (4, 10, 180)
    assert r['match'].dtype == np.uint8 and r['AP_per_class'].shape == (3,)
    assert np.array_equal(r['iou_thresholds'], np.linspace(0.5, 0.95, 10).astype(np.float32))
    assert r['area_ranges'].tolist() == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]
    assert abs(r['AP'] - np.nanmean(ref['ap'][0])) <= 1e-12 and abs(r['AP50'] - np.nanmean(ref['ap'][0, 0])) <= 1e-12
    assert abs(r['AP75'] - np.nanmean(ref['ap'][0, 5])) <= 1e-12 and abs(r['APm'] - np.nanmean(ref['ap'][2])) <= 1e-12
    assert np.max(np.abs(r['AP_per_class'] - np.nanmean(ref['ap'][0], 0))) <= 1e-12
    r = _run(dets, gts, 3, iou_thresholds=[0.3, 0.6], area_ranges=[[0, 1e10], [0, 1024]])
    assert all(math.isnan(r[k]) for k in ('AP50', 'AP75', 'APs', 'APm', 'APl')) and not math.isnan(r['AP']) and not math.isnan(r['AR'])


class _CannedBatched(TV._CannedModel):
    def test_images(self, images):
        return [self.test_one_image(images[b: b + 1]) for b in range(images.shape[0])]


def test_evaluate_metric_coco_drives_the_model_and_batches_agree():
    import odtk
    dets, gts = R.random_case(10, 10, 3, 10, 4)
    with TV.emulated():
        m = TV._CannedModel(dets, 3)
        r = odtk.evaluate(m, TV._generator(gts, 4), metric='coco', max_dets=2, num_images=9)      # the cap and the image count reach the evaluator
        assert m.fed == list(range(9))
        _same(r, R.evaluate(dets[:9], gts[:9], 3, max_dets=2))
        assert (r['match'] == 2).all(axis=(0, 1)).any()
        m = _CannedBatched(dets, 3)
        rb = odtk.evaluate(m, TV._generator(gts, 4), metric='coco', max_dets=2, num_images=9, batch_size=3)
        assert m.fed == list(range(9))
        assert rb['match'].tobytes() == r['match'].tobytes() and rb['ap'].tobytes() == r['ap'].tobytes()


def test_match_at_0_5_equals_the_voc_matcher_where_the_rules_coincide():
    # GT rows in cells of their own (no two overlap); each gets at most ONE detection above 0.5 (a 5 % shift: IoU > 0.8), any number of far misses
    # (a 60 % shift: IoU 0.25) and detections of another class: then >= / >, "best untaken row" / "best row" and the ignore rules cannot differ
    import odtk
    rng = np.random.default_rng(12)
    dets, gts = [], []
    for _ in range(20):
        n = int(rng.integers(1, 6))
        cell = rng.permutation(9)[:n]
        yc, xc = 100.0 * (cell // 3) + 50, 100.0 * (cell % 3) + 50
        h, w = rng.uniform(20, 60, n), rng.uniform(20, 60, n)
        cls = rng.integers(0, 3, n)
        gts.append(np.stack([yc, xc, h, w, cls], 1).astype(np.float32))
        sc, bx, cl = [], [], []
        for k in range(n):
            shifts = ([0.05] if rng.random() < 0.7 else []) + [0.6] * int(rng.integers(0, 3))
            for s in shifts:
                bx.append([yc[k] - h[k] / 2, xc[k] - w[k] / 2 + s * w[k], yc[k] + h[k] / 2, xc[k] + w[k] / 2 + s * w[k]])
                sc.append(rng.integers(1, 9) / 8)
                cl.append(cls[k] if rng.random() < 0.85 else (cls[k] + 1) % 3)
        p = rng.permutation(len(sc))
        dets.append((np.array(sc, np.float32)[p], np.array(bx, np.float32).reshape(-1, 4)[p], np.array(cl, np.int32)[p]))
    with TV.emulated():
        ev = odtk.VOCEvaluator(3, 0.5, 'area', device='cpu')
        for d, g in zip(dets, gts):
            ev.add(list(d), g)
        voc = ev.result()
    r = _run(dets, gts, 3)
    assert voc['tp'].sum() > 10 and (voc['tp'] == 0).sum() > 10
    assert np.array_equal(r['match'][0, 0], voc['tp']) and r['npos'][0].tolist() == voc['npos'].tolist()


def test_symbols_in_library_header_and_signatures():
    from odtk import _lib
    exported = subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()
    header = open(os.path.join(TV.B.ROOT, 'include', 'odtk.h')).read()
    for n in ('odtk_coco_eval', 'odtk_coco_eval_workspace_bytes'):
        assert f' T {n}\n' in exported and f'{n}(' in header and n in _lib.SIGNATURES
    assert _lib.load().odtk_version() >= 105
