"""Ground-truth flags (VOC `difficult`, COCO ignore / crowd) on the CPU tier: the restatement tests/flag_eval_ref.py against hand-worked answers and,
without flags, against voc_eval_ref / coco_eval_ref; csrc/voc_eval.hip (odtk_voc_eval_flags, odtk_coco_eval_flags) through the CPU emulation of
tests/test_cpu_voc_eval.py against the restatement; the evaluators' host logic on the emulated entry points.  The sets are tests/flag_eval_cases.py's.

Comparison rule (that of tests/test_gpu_coco_eval.py and tests/test_gpu_voc_eval.py): match, npos, num_ignored_gt and the NaN pattern equal;
|AP - ref| <= 1e-12 and the same for recall."""
import contextlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coco_eval_ref as CR           # noqa: E402
import flag_eval_cases as K          # noqa: E402
import flag_eval_ref as F            # noqa: E402
import test_cpu_coco_eval as TC      # noqa: E402
import test_cpu_voc_eval as TV       # noqa: E402
import voc_eval_ref as VR            # noqa: E402

NEW = ('odtk_voc_eval_flags', 'odtk_coco_eval_flags')


@contextlib.contextmanager
def emulated():
    from odtk import _lib
    with TV.emulated() as lib:
        for n in NEW + ('odtk_coco_eval', 'odtk_coco_eval_workspace_bytes'):
            getattr(lib, n).restype, getattr(lib, n).argtypes = _lib.SIGNATURES[n]
        yield lib


# ---------------------------------------------------------------- what the CPU and the GPU tier share
def same_voc(r, ref):
    assert np.array_equal(r['match'], ref['match']) and np.array_equal(r['tp'], ref['tp']) and r['tp'].max(initial=0) <= 1
    assert r['npos'].tolist() == ref['npos'].tolist() and r['num_ignored_gt'].tolist() == ref['num_ignored_gt'].tolist()
    assert r['num_detections'].tolist() == ref['num_detections'].tolist()
    assert np.array_equal(np.isnan(r['AP']), np.isnan(ref['AP']))
    ok = ~np.isnan(ref['AP'])
    err = np.max(np.abs(r['AP'][ok] - ref['AP'][ok]), initial=0.0)
    print(f'VOC AP: max |AP - ref| = {err:.3e} (bound 1e-12)')
    assert err <= 1e-12
    assert math.isnan(r['mAP']) == math.isnan(ref['mAP']) and (math.isnan(ref['mAP']) or abs(r['mAP'] - ref['mAP']) <= 1e-12)


def same_coco(r, ref):
    for k in ('ap', 'recall'):
        ok = ~np.isnan(ref[k]) & ~np.isnan(r[k])
        print(f'COCO {k}: max |x - ref| = {np.max(np.abs(r[k][ok] - ref[k][ok]), initial=0.0):.3e} (bound 1e-12)')
    TC._same(r, ref)
    assert r['num_ignored_gt'].tolist() == ref['num_ignored_gt'].tolist()


def run_voc(dets, gts, flags, C, metric, device, column=False):
    import odtk
    ev = odtk.VOCEvaluator(C, 0.5, metric, device=device)
    add_all(ev, dets, gts, flags, column)
    return ev.result()


def run_coco(dets, gts, flags, C, device, column=False, **kw):
    import odtk
    ev = odtk.COCOEvaluator(C, device=device, **kw)
    add_all(ev, dets, gts, flags, column)
    return ev.result()


def add_all(ev, dets, gts, flags, column=False):
    if column:
        gts, flags = K.with_flag_column(gts, flags), None
    for k, (d, g) in enumerate(zip(dets, gts)):
        if flags is None:
            ev.add(list(d), g)
        else:
            ev.add(list(d), g, flags=flags[k])


def check_hand_voc(run, every_metric=True):
    """run(dets, gts, flags or None, C, metric) -> result: the hand-worked VOC sets (answers: flag_eval_cases.py).  every_metric=False (the emulation,
    where a call costs ten seconds whatever its size): both metrics on the flagged first set only, one each on the rest"""
    dets, gts, flags, C = K.voc_difficult()
    for metric in ('voc07', 'area'):
        r = run(dets, gts, flags, C, metric)
        assert r['match'].tolist() == [0, 2, 1, 0, 2] and r['tp'].tolist() == [0, 0, 1, 0, 0]
        assert r['npos'].tolist() == [1] and r['num_ignored_gt'].tolist() == [1]
        assert abs(r['AP'][0] - 0.5) <= 1e-12 and abs(r['mAP'] - 0.5) <= 1e-12
        if not every_metric and metric == 'area':
            continue
        r = run(dets, gts, None, C, metric)                                # the same input without flags: what the parent commit computes
        assert r['tp'].tolist() == [0, 1, 1, 0, 0] and r['npos'].tolist() == [2] and abs(r['AP'][0] - 2 / 3) <= 1e-12
    dets, gts, flags, C = K.voc_all_rows_flagged()
    for metric in ('voc07', 'area') if every_metric else ('area',):
        r = run(dets, gts, flags, C, metric)
        assert r['match'].tolist() == [1, 2, 2, 0] and r['npos'].tolist() == [1, 0] and r['num_ignored_gt'].tolist() == [0, 2]
        assert math.isnan(r['AP'][1]) and abs(r['AP'][0] - 1.0) <= 1e-12 and abs(r['mAP'] - 1.0) <= 1e-12


def check_hand_coco(run):
    """run(dets, gts, flags or None, C, **kw) -> result: the hand-worked COCO sets"""
    for flag, code, npos in [(2, 2, 0), (1, 0, 0), (0, 0, 1)]:
        dets, gts, flags, C, kw = K.coco_crowd_box(flag)
        r = run(dets, gts, flags, C, **kw)
        assert r['match'].shape == (1, 10, 2) and np.all(r['match'] == code) and r['npos'].tolist() == [[npos]]
        assert r['num_ignored_gt'].tolist() == [int(flag > 0)]
    for flag, codes in [(1, [2, 0]), (2, [2, 2])]:
        dets, gts, flags, C, kw = K.coco_ignore_row_matches_once(flag)
        r = run(dets, gts, flags, C, **kw)
        assert r['match'][0, 0].tolist() == codes and r['npos'].tolist() == [[0]] and np.all(np.isnan(r['ap']))
    dets, gts, flags, C, kw = K.coco_ordinary_row_beats_crowd()
    r = run(dets, gts, flags, C, **kw)
    assert r['match'][0, :, 0].tolist() == [1, 1, 2] and r['npos'].tolist() == [[1]]
    assert abs(r['ap'][0, 0, 0] - 1.0) <= 1e-12 and r['ap'][0, 2, 0] == 0.0
    # a row flagged 0 whose area is outside the range behaves as without flags: coco_eval_ref decides
    dets, gts, C, kw = TC.hand_small_gt()
    zeros = [np.zeros(len(g), np.int64) for g in gts]
    r, ref = run(dets, gts, zeros, C, **kw), CR.evaluate(dets, gts, C, **kw)
    TC._same(r, ref)
    assert r['match'][:, 0, 0].tolist() == [1, 1, 2, 2] and r['num_ignored_gt'].tolist() == [0, 0]


def check_random(name, device):
    """one random shape through both evaluators (both metrics, both detection caps) against the shared references; the [pad, 6] form of add() for VOC,
    flags= for COCO; the set must exercise the feature"""
    dets, gts, flags, C = K.case(name)
    start, length = K.big_segment(name)
    assert length > 64 and start // 64 != (start + length - 1) // 64        # the segment crosses a 64-position boundary of coco_match_kernel
    assert len(np.unique(np.concatenate([d[0] for d in dets]))) <= 8          # duplicate scores
    for metric in ('voc07', 'area'):
        ref, plain = K.voc_reference(name, metric), K.voc_reference(name, metric, False)
        same_voc(run_voc(dets, gts, flags, C, metric, device, column=True), ref)
        assert (ref['match'] == 2).any() and ((ref['match'] == 2) & (plain['match'] != 2)).any() and (ref['match'] == 1).any()
    for max_dets in K.MAX_DETS:
        ref, plain = K.coco_reference(name, max_dets), K.coco_reference(name, max_dets, False)
        same_coco(run_coco(dets, gts, flags, C, device, max_dets=max_dets), ref)
        assert ((ref['match'][0] == 2) & (plain['match'][0] != 2)).any()     # code 2 that only a flag explains (range 0 ignores no area)
        assert ref['max_crowd_hits'] > 1                                       # a crowd row matched more than once
        assert {1, 2} <= set(np.unique(ref['match'][0])) and (max_dets < 100 or (ref['match'][0] == 0).any())


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def check_null_flags_equal_the_plain_entry_points(device):
    """gt_flags = NULL through the _flags entry points: every output torch.equal (doubles by their bits) to odtk_voc_eval / odtk_coco_eval"""
    import odtk
    from odtk import ops
    dets, gts, _, C = K.case('40img-5cls')
    ev = odtk.COCOEvaluator(C, device=device)
    add_all(ev, dets, gts, None)
    args, _ = ev._upload()
    D, G, I = args[0].shape[0], args[4].shape[0], len(dets)
    for metric in ('voc07', 'area') if device != 'cpu' else ('area',):
        outs = []
        for flagged in (False, True):
            ws = ops.voc_eval_workspace(D, G, I, C, device)
            tp = torch.full((D,), 9, dtype=torch.uint8, device=device)
            npos = torch.full((C,), -7, dtype=torch.int32, device=device)
            nign = torch.full((C,), -7, dtype=torch.int32, device=device)
            ap = torch.full((C,), -7.0, dtype=torch.float64, device=device)
            if flagged:
                ops.voc_eval_flags(*args, None, I, C, 0.5, metric, ws, tp, npos, nign, ap)
                assert (nign == 0).all()
            else:
                ops.voc_eval(*args, I, C, 0.5, metric, ws, tp, npos, ap)
            outs.append((tp, npos, ap))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*outs)) and (outs[0][0] == 1).any()
    thr, rng = ev.iou_thresholds, ev.area_ranges
    T, R = len(thr), len(rng)
    outs = []
    for flagged in (False, True):
        ws = ops.coco_eval_workspace(D, G, I, C, T, R, device)
        match = torch.full((R, T, D), 9, dtype=torch.uint8, device=device)
        npos = torch.full((R, C), -7, dtype=torch.int32, device=device)
        ap = torch.full((R, T, C), -7.0, dtype=torch.float64, device=device)
        rec = torch.full((R, T, C), -7.0, dtype=torch.float64, device=device)
        if flagged:
            ops.coco_eval_flags(*args, None, I, C, thr, rng, 100, ws, match, npos, ap, rec)
        else:
            ops.coco_eval(*args, I, C, thr, rng, 100, ws, match, npos, ap, rec)
        outs.append((match, npos, ap, rec))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*outs)) and (outs[0][0] == 1).any()


def check_empty_sides(device):
    dets, gts, flags, C = K.case('40img-5cls')
    dets, gts, flags = dets[:6], gts[:6], flags[:6]
    empty = [(np.zeros(0, np.float32), np.zeros((0, 4), np.float32), np.zeros(0, np.int32)) for _ in gts]
    same_voc(run_voc(empty, gts, flags, C, 'area', device), F.voc_evaluate(empty, gts, C, flags, metric='area'))          # D = 0
    r = run_coco(empty, gts, flags, C, device)
    same_coco(r, F.coco_evaluate(empty, gts, C, flags))
    assert r['match'].shape == (4, 10, 0) and r['num_ignored_gt'].sum() > 0
    no_gt, no_fl = [np.zeros((0, 5), np.float32) for _ in dets], [np.zeros(0, np.int64) for _ in dets]
    r = run_voc(dets, no_gt, no_fl, C, 'voc07', device)                                                                    # G = 0
    same_voc(r, F.voc_evaluate(dets, no_gt, C, no_fl))
    assert np.all(np.isnan(r['AP'])) and not r['match'].any()
    same_coco(run_coco(dets, no_gt, no_fl, C, device), F.coco_evaluate(dets, no_gt, C, no_fl))


def check_flag_3_is_refused_by_the_library(device):
    """past the evaluators' own check: a flag byte 3 on the device reaches the C-ABI, which names the row"""
    import odtk
    from odtk import ops
    dets, gts, flags, C = K.voc_difficult()
    ev = odtk.COCOEvaluator(C, iou_thresholds=[0.5], area_ranges=K.ALL, device=device)
    add_all(ev, dets, gts, flags)
    args, _, gfl, _ = ev._upload(True)
    gfl = gfl.clone()
    gfl[1] = 3
    D, G = 5, 2
    tp, npos, nign = (torch.empty(n, dtype=t, device=device) for n, t in ((D, torch.uint8), (C, torch.int32), (C, torch.int32)))
    ap = torch.empty(C, dtype=torch.float64, device=device)
    with pytest.raises(odtk.OdtkError, match=r'voc_eval: gt_flags\[1\] is above 2'):
        ops.voc_eval_flags(*args, gfl, 1, C, 0.5, 'voc07', ops.voc_eval_workspace(D, G, 1, C, device), tp, npos, nign, ap)
    match = torch.empty(1, 1, D, dtype=torch.uint8, device=device)
    ap, rec = (torch.empty(1, 1, C, dtype=torch.float64, device=device) for _ in range(2))
    with pytest.raises(odtk.OdtkError, match=r'coco_eval: gt_flags\[1\] is above 2'):
        ops.coco_eval_flags(*args, gfl, 1, C, [0.5], K.ALL, 100, ops.coco_eval_workspace(D, G, 1, C, 1, 1, device), match, npos.view(1, C), ap, rec)
    gfl[1] = 2                                                               # and the same buffers with a valid flag pass
    ops.voc_eval_flags(*args, gfl, 1, C, 0.5, 'voc07', ops.voc_eval_workspace(D, G, 1, C, device), tp, npos, nign, ap.view(-1))
    assert tp.tolist() == [0, 2, 1, 0, 2]


# ---------------------------------------------------------------- the restatement
def test_ref_without_flags_is_the_unflagged_restatement():
    rng = np.random.default_rng(3)
    dets, gts = TV._random_case(rng, 30, 4, 20, 5)
    for metric in ('voc07', 'area'):
        a, b = F.voc_evaluate(dets, gts, 4, metric=metric), VR.evaluate(dets, gts, 4, metric=metric)
        assert np.array_equal(a['match'], b['tp']) and np.array_equal(a['tp'], b['tp']) and a['npos'].tolist() == b['npos'].tolist()
        assert np.array_equal(a['AP'], b['AP'], equal_nan=True) and a['mAP'] == b['mAP'] and not a['num_ignored_gt'].any()
    dets, gts = CR.random_case(4, 30, 6, 20, 4, levels=4)
    a, b = F.coco_evaluate(dets, gts, 6, max_dets=8), CR.evaluate(dets, gts, 6, max_dets=8)
    assert np.array_equal(a['match'], b['match']) and np.array_equal(a['npos'], b['npos'])
    assert np.array_equal(a['ap'], b['ap'], equal_nan=True) and np.array_equal(a['recall'], b['recall'], equal_nan=True)
    zeros = [np.zeros(len(g), np.int64) for g in gts]
    assert np.array_equal(F.coco_evaluate(dets, gts, 6, zeros, max_dets=8)['ap'], b['ap'], equal_nan=True)


def test_ref_hand_worked_sets():
    check_hand_voc(lambda d, g, f, C, metric: F.voc_evaluate(d, g, C, f, metric=metric))
    check_hand_coco(lambda d, g, f, C, **kw: F.coco_evaluate(d, g, C, f, **kw))


# ---------------------------------------------------------------- kernel source through the CPU emulation
def test_emulated_kernels_on_the_hand_worked_sets():
    with emulated():
        check_hand_voc(lambda d, g, f, C, metric: run_voc(d, g, f, C, metric, 'cpu'), every_metric=False)
        check_hand_coco(lambda d, g, f, C, **kw: run_coco(d, g, f, C, 'cpu', **kw))


@pytest.mark.parametrize('name', list(K.SHAPES))
def test_emulated_kernels_vs_ref(name):
    with emulated():
        check_random(name, 'cpu')


def test_emulated_null_flags_empty_sides_and_the_refused_flag():
    with emulated():
        check_null_flags_equal_the_plain_entry_points('cpu')
        check_empty_sides('cpu')
        check_flag_3_is_refused_by_the_library('cpu')


# ---------------------------------------------------------------- evaluators: host logic
def test_add_refusals():
    import odtk
    d = list(TV._det([0.9], [TV._box(0, 0, 10, 10)], [0]))
    g = TV._gt([5, 5, 10, 10, 0], [-1, -1, -1, -1, -1])
    g6 = np.concatenate([g, [[1], [-1]]], 1).astype(np.float32)
    for make in (lambda: odtk.VOCEvaluator(3, device='cpu'), lambda: odtk.COCOEvaluator(3, device='cpu')):
        ev = make()
        with pytest.raises(ValueError, match='image 0: flags given twice'):
            ev.add(d, g6, flags=[1, 0])
        with pytest.raises(ValueError, match=r'image 0: flags must be \[pad\] = \[2\]'):
            ev.add(d, g, flags=[1])
        with pytest.raises(ValueError, match='image 0: flags must be an integer or bool array'):
            ev.add(d, g, flags=np.array([1.0, 0.0]))
        with pytest.raises(ValueError):
            ev.add(d, np.zeros((2, 7), np.float32))
        assert ev.num_images == 0 and not ev.has_flags
        ev.add(d, g)                                                        # image 0: no flags
        for bad, text in [(np.array([3, 0]), 'flag 3'), (np.array([-1, 0]), 'flag -1')]:
            ev.add(d, g, flags=bad)
            with pytest.raises(ValueError, match=f'ground_truth of image 1: {text} is not 0'):
                ev.result()
            ev._dets.pop(), ev._gts.pop(), ev._flags.pop()
        ev.add(d, np.concatenate([g, [[1.5], [0]]], 1).astype(np.float32))  # a non-integer flag in the sixth column
        with pytest.raises(ValueError, match='ground_truth of image 1: flag 1.5 is not 0'):
            ev.result()


def test_add_forms_agree_and_padding_goes_with_its_flags():
    dets, gts, flags, C = K.voc_difficult()
    g = np.concatenate([gts[0][:1], -np.ones((1, 5), np.float32), gts[0][1:]])          # a padding row between the two, its flag out of range
    with emulated():
        import odtk
        packed = []
        for form in ('int', 'bool', 'torch', 'column'):                     # every form packs to the same arrays ...
            ev = odtk.VOCEvaluator(C, device='cpu')
            if form == 'column':
                ev.add(list(dets[0]), torch.from_numpy(np.concatenate([g, [[0], [7], [1]]], 1).astype(np.float32)))
            else:
                f = {'int': np.array([0, 7, 1]), 'bool': np.array([False, True, True]), 'torch': torch.tensor([0, 7, 1])}[form]
                ev.add(list(dets[0]), g, flags=f)
            packed.append(ev._pack(True))
            assert packed[-1][6].dtype == np.uint8 and packed[-1][6].tolist() == [0, 1] and packed[-1][4].shape == (2, 5)
            assert all(np.array_equal(a, b) for a, b in zip(packed[0], packed[-1]))
        r = ev.result()                                                     # ... and the last one through the kernels
        assert r['match'].tolist() == [0, 2, 1, 0, 2] and r['npos'].tolist() == [1] and r['num_ignored_gt'].tolist() == [1]
        # an evaluator that never saw flags takes the unflagged path and says so in its result
        ev = odtk.VOCEvaluator(C, device='cpu')
        ev.add(list(dets[0]), g)
        r = ev.result()
        assert r['match'].tolist() == r['tp'].tolist() == [0, 1, 1, 0, 0] and r['num_ignored_gt'].tolist() == [0] and r['npos'].tolist() == [2]
        ev = odtk.COCOEvaluator(C, device='cpu')
        ev.add(list(dets[0]), g)
        assert 'num_ignored_gt' not in ev.result()


class _Canned(TV._CannedModel):
    def test_images(self, images):
        return [self.test_one_image(images[b: b + 1]) for b in range(images.shape[0])]


def _generator6(gts6, B):
    batches = []
    for s in range(0, len(gts6), B):
        g = gts6[s: s + B]
        pad = max(len(x) for x in g)
        gt = -np.ones((len(g), pad, g[0].shape[1]), np.float32)
        for k, x in enumerate(g):
            gt[k, : len(x)] = x
        imgs = np.zeros((len(g), 4, 4, 3), np.float32)
        imgs[:, 0, 0, 0] = np.arange(s, s + len(g))
        batches.append((imgs, gt))
    return batches


def test_evaluate_over_six_column_batches():
    import odtk
    dets, gts, flags, C = K.case('40img-5cls')
    dets, gts, flags = dets[:9], gts[:9], flags[:9]
    gts6 = K.with_flag_column(gts, flags)
    with emulated():
        for metric, kw in (('voc07', {}), ('coco', dict(max_dets=3))):
            if metric == 'coco':
                by_hand = run_coco(dets, gts, flags, C, 'cpu', **kw)
            else:
                by_hand = run_voc(dets, gts, flags, C, metric, 'cpu')
            results = []
            for bs in (1, 2) if metric == 'voc07' else (2,):               # chunks of 2 out of batches of 3: re-padded rows
                m = _Canned(dets, C)
                results.append(odtk.evaluate(m, _generator6(gts6, 3), metric=metric, batch_size=bs, **kw))
                assert m.fed == list(range(9))
            for r in results:
                assert r['match'].tobytes() == by_hand['match'].tobytes() and r['npos'].tolist() == by_hand['npos'].tolist()
                assert r['num_ignored_gt'].tolist() == by_hand['num_ignored_gt'].tolist() and r['num_ignored_gt'].sum() > 0
                ap = 'ap' if metric == 'coco' else 'AP'
                assert r[ap].tobytes() == by_hand[ap].tobytes()
        mixed = _generator6(gts6[:3], 3) + TV._generator(gts[3:6], 3)
        for bs in (1, 2):
            with pytest.raises(ValueError, match='of 6 and of 5 columns in one pass'):
                odtk.evaluate(_Canned(dets, C), mixed, batch_size=bs)


def test_symbols_in_library_header_and_signatures():
    from odtk import _lib
    exported = subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()
    header = open(os.path.join(TV.B.ROOT, 'include', 'odtk.h')).read()
    for n in NEW:
        assert f' T {n}\n' in exported and f'{n}(' in header and n in _lib.SIGNATURES
    assert _lib.load().odtk_version() >= 106
