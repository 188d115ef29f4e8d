"""CPU tier of the Light-Head R-CNN edge cases (tests/lhrcnn_edge_cases.py): the box-side kernels of csrc/lhrcnn.hip run FROM SOURCE under the fiber emulation
(tests/hip_cpu_backend.py; odtk_nms_batched is the oracle's there) through the same check() the GPU tier calls.  This is where the table, its constructions
and the out-of-operand fix of lh_match_kernel (`nan_area`) are proved before anything reaches a device."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hip_cpu_backend as HC             # noqa: E402
import lhrcnn_edge_cases as LE           # noqa: E402


@pytest.mark.parametrize('group,case', LE.PARAMS, ids=[f'{g}-{c}' for g, c in LE.PARAMS])
def test_emulated_lhrcnn_edge(group, case):
    with HC.installed():
        LE.check(group, case, 'cpu')


def test_table_is_complete():
    """every case the table is meant to hold is there, at the shapes whose anchor counts take the kernel's other paths"""
    rpn = {c for g, c in LE.PARAMS if g == 'rpn'}
    assert {'one', 'dup_same_class', 'dup_other_class', 'reversed', 'one_px', 'sliver', 'whole_image', 'partly_outside', 'centre_on_edge', 'pad_minus_1',
            'all_valid', 'pad_128', 'pad_129', 'zero', 'no_overlap', 'same_best_anchor', 'exact_anchor', 'iou05_below', 'iou05_exact', 'iou05_above',
            'iou03_below', 'iou03_exact', 'iou03_above', 'many_positive', 'few_negative', 'nan_area'} <= rpn
    assert sum(LE.L in c.rejects for c in LE.RPN_CASES) <= 2 and [c.name for c in LE.RPN_CASES if LE.L in c.refused] == ['pad_129']
    assert {c.shape for c in LE.RPN_CASES} == {'big', 'mid', 'small'}
    for key, (lo, hi) in LE.A_RANGE.items():
        assert lo <= LE.family(key).A <= hi, key
    assert LE.family('small').A < 64 and LE.family('small').A % 64 != 0 and 64 < LE.family('mid').A < 256 < LE.family('big').A
    assert LE.RPN_BY_NAME['pad_128'].pad == 128 and LE.RPN_BY_NAME['pad_129'].pad == 129 and LE.RPN_BY_NAME['many_positive'].pad == 128
    assert {'empty_image', 'no_positive', 'full_and_single', 'inf_truth'} <= set(LE.RCNN_CASES)
    assert {(128, 128), (1, 0), (128, 0)} <= set(LE.RCNN_CASES['full_and_single'][0]) and (0, 0) in LE.RCNN_CASES['empty_image'][0]
    assert all(kp == 0 for kp, _ in LE.RCNN_CASES['no_positive'][0])
    assert {('gather_rois', c) for c in ('0', '1', 'cap', 'cap+5')} <= set(LE.PARAMS) and {('rcnn_decode', r) for r in ('1', '255', '257')} <= set(LE.PARAMS)
    crops = {(v[0], v[3]) for v in LE.CROP_CASES.values()}
    assert {c for c, _ in crops} == {1, 2, 7} and {c for _, c in crops} == {1, 7, 490}
    assert any(v[1] == 1 for v in LE.CROP_CASES.values()) and any(v[2] == 1 for v in LE.CROP_CASES.values()) and any(v[4] for v in LE.CROP_CASES.values())
    for n in LE.CROP_CASES:
        assert ('crop_f32', n) in LE.PARAMS and ('crop_bf16', n) in LE.PARAMS
